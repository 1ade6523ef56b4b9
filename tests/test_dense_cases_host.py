"""CPU-only: the cases of tests/helpers/dense_cases.py have the properties they are named for, and the NumPy restatements stay
inside the bounds test_hip_dense_blocks.py holds the device to, with the headroom stated here.

A device test passes just as well when its case misses the path it was built for, and a bound that the plain restatement of the
operation does not keep says nothing about a kernel; both are conditions of the cases and are asserted here, without the library.

Where a case of the issue does not have its property, the deviation is stated at the assertion:
  * kappa = 1e7 in fp32 is at the Newton-Schulz threshold, not beyond it (||G - I||_F after the first pass is 0.8e-3 ... 5.5e-3 around
    ns_max = 1.6e-3), so only fp64 asserts the path [0, 0] there; in fp32 [0, 0] is asserted under MMW_FACTOR_NO_NS=1.
  * kappa = 1e10 in fp32: the block rounded to fp32 has a condition number of 4e8 ... 1e9, inside the band where the issue itself
    leaves the path free, so only fp64 asserts that the first pass is the fallback; in fp32 the zero-column case asserts it.
  * for b <= 2 the Cholesky residual may use the whole of Higham's bound (one square root and one division are all there is); the
    restatement's share is below 0.25 from b = 31 on.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dense_cases as dc  # noqa: E402

TYPES = [("f32", np.float32), ("f64", np.float64)]


def test_gram_cases_cover_every_size_padding_and_symmetrisation():
    cases = dc.gram_cases()
    assert 55 <= len(cases) <= 65 and len(set(cases)) == len(cases)
    for K in dc.GRAM_K:
        assert {b for k, b, _, _ in cases if k == K} >= {5, 65}
    for b in dc.GRAM_B:
        assert {k for k, bb, _, _ in cases if bb == b} >= {17, 257}
    for axis, sizes in ((0, dc.GRAM_K), (1, dc.GRAM_B)):  # every K and every b meets both paddings and both values of sym
        for pick in (lambda c: c[2] - c[1], lambda c: c[3]):
            for value in {pick(c) for c in cases}:
                assert {c[axis] for c in cases if pick(c) == value} == set(sizes)


@pytest.mark.parametrize("Tname,T", TYPES)
def test_integer_blocks_are_exact_in_both_types(Tname, T):
    V = dc.int_block(1000, 129, 134, 3, T)
    assert np.all(V[:, :129] == np.round(V[:, :129])) and np.abs(V[:, :129]).max() == 8 and np.all(V[:, 129:] == dc.SENTINEL)
    assert 1000 * 64 < 2 ** 24  # every partial sum of a Gram entry is an integer that even fp32 holds; the accumulators are fp64
    assert max(dc.GEMM_B) * 64 < 2 ** 24  # ... and so is every entry of a tall product, which is stored in T
    for b in dc.GEMM_B:
        for K, n, ld, ldq in dc.gemm_cases(b):
            assert ld >= max(b, n) and ldq >= n
        assert {c[1] for c in dc.gemm_cases(b)} == set(dc.GEMM_N + [b]) and {c[0] for c in dc.gemm_cases(b)} == set(dc.GEMM_K)


@pytest.mark.parametrize("cond", dc.CHOL_COND)
@pytest.mark.parametrize("b", dc.CHOL_B)
def test_cholesky_restatement_keeps_highams_bound_with_room(b, cond):
    G = dc.spd(b, cond, 7 * b + 1)
    assert np.allclose(np.diag(G), 1.0, rtol=0, atol=4 * dc.U64)
    if b > 1:
        assert 0.5 * cond <= np.linalg.cond(G) <= 2.0 * cond
    L, dinv, ok, _ = dc.chol_restatement(G)
    assert ok
    share = dc.chol_residual_share(L, G)
    print("b %d cond %.0e: share of Higham's bound %.3f" % (b, cond, share))
    assert share <= 1.0
    if b >= 31:
        assert share < 0.25
    for p, Di in enumerate(dinv):
        assert dc.dinv_share(Di, L, p) < 0.25


@pytest.mark.parametrize("name", sorted(dc.BREAKDOWN))
def test_breakdown_cases_break_where_they_say(name):
    G, where = dc.breakdown_case(name)
    assert np.all(np.isfinite(G)) and np.array_equal(G, G.T)
    Gs, d = dc.scale_unit_diagonal(G)
    L, _, ok, at = dc.chol_restatement(Gs)
    assert not ok and at == where
    if name == "zero_diagonal":
        assert G[where, where] == 0.0 and d[where] == 0.0 and Gs[where, where] == 0.0
    else:
        assert np.all(np.diag(G) > 0) and np.linalg.eigvalsh(G)[0] < -1e-3
        # not a near miss: the pivot is negative by far more than rounding
        assert np.linalg.eigvalsh(Gs[:where + 1, :where + 1])[0] < -1e-3
    b = G.shape[0]
    if name == "panel0":
        assert where < 32
    if name == "later_full_panel":
        assert 32 <= where < 64 <= b
    if name == "partial_last_panel":
        assert where >= 64 and 64 < b < 96


def orth_ids():
    out = []
    for K, b in dc.ORTH_SHAPES:
        for pad in dc.ORTH_PAD:
            out.append((K, b, pad))
    return out


@pytest.mark.parametrize("Tname,T", TYPES)
@pytest.mark.parametrize("K,b,pad", orth_ids())
def test_orthonormalise_cases_take_their_paths_and_keep_the_bounds(K, b, pad, Tname, T):
    for kind, kappa, no_ns in dc.orth_list(Tname):
        c = dc.orth_case(K, b, pad, kind, kappa, Tname, no_ns)
        V = c["V"]
        tag = "%s kappa %.0e no_ns %d" % (kind, kappa, no_ns)
        assert np.all(V[:, b:] == dc.SENTINEL) and np.all(np.isfinite(V)), tag
        want = dc.expected_path(b, kind, kappa, Tname, no_ns)
        if want is not None:
            assert c["path"][:len(want)] == want, (tag, c["path"], c["dev2"])
        if kind == "svd" and b > 1 and T == np.float64:
            assert abs(np.linalg.cond(V[:, :b]) / kappa - 1.0) < 0.05, tag
        if kind == "svd" and b > 1 and T == np.float32 and kappa >= 1e9:  # what fp32 storage leaves of the conditioning
            assert 1e8 < np.linalg.cond(V[:, :b]) < 3e9, tag
        # away from the Newton-Schulz threshold where a path is asserted: the restatement and the device see different rounding noise
        if b > 1 and want == [0, 1]:
            assert c["dev2"] <= dc.NS_MAX[T] / 8, (tag, c["dev2"])
        if b > 1 and want == [0, 0] and not no_ns:
            assert c["dev2"] >= 100 * dc.NS_MAX[T], (tag, c["dev2"])
        if kind == "zero":
            lam, tol = dc.zero_case_spectrum(c["Q"], T)
            assert abs(lam[0]) <= tol and np.all(np.abs(lam[1:] - 1.0) <= tol), (tag, lam[:2], tol)
            assert c["err_s"] <= dc.orth_bounds(T, b, 0.0, 2)[1], tag
            continue
        if kappa > 1e10:
            assert np.all(np.isfinite(c["Q"])), tag
            assert b == 1 or c["err_o"] >= (1e-11 if kappa == 1e12 else 1e-7), (tag, c["err_o"])  # beyond the design's reach
            continue
        bo, bs = dc.orth_bounds(T, b, c["err_o"], c["path"][1])
        # headroom: in fp32 the restatement uses at most a quarter of the bound on err_o away from the Newton-Schulz threshold and
        # a fifth of the bound on err_s; in fp64 its own err_o is the bound's yardstick and is at rounding level
        assert c["err_s"] <= (bs if T == np.float64 else 0.2 * bs) or b == 1, (tag, c["err_s"], bs)
        if T == np.float32:
            assert c["err_o"] <= bo, (tag, c["err_o"], bo)
            if c["path"][1] != 1:
                assert c["err_o"] <= 0.25 * bo, (tag, c["err_o"], bo)
        elif kappa <= 1e8:
            assert c["err_o"] <= max(2e-15, b * dc.U64) + (dc.ns_term(T) if c["path"][1] == 1 else 0.0), (tag, c["err_o"])
        else:
            assert c["err_o"] <= 2e-12, (tag, c["err_o"])


@pytest.mark.parametrize("Tname,T", TYPES)
def test_cholesky_qr_restatement_gives_the_qr_factor(Tname, T):
    for K, b in dc.ORTH_SHAPES:
        for kappa in (1.0, 1e2):
            c = dc.orth_case(K, b, 0, "svd", kappa, Tname, True)
            diff = np.max(np.abs(c["Q"] - dc.qr_positive(np.array(c["V"][:, :b]))))
            assert diff <= 0.25 * dc.qr_bound(T, b, kappa), (K, b, kappa, diff)
