"""The factor's dense kernels, each as the operation it is, against NumPy in float64 (mmw_dense_gram / _gemm / _chol / _orth).

k_gram_tiles + k_gram_reduce and k_gemm_tall are held to exact integer results at every tile and slice edge and to the standard
dot-product bound on random data; k_chol_panel + k_chol_update to Higham's entrywise residual bound, in the register form and under
MMW_CHOL_LDS=1, with breakdown reported; Factorizer::orthonormalise (k_trsm_blocked, the Newton-Schulz step, the eigen fallback) to
orthonormality, span and -- where it is unique -- the QR factor itself, on the paths the cases of tests/helpers/dense_cases.py were
built for.  test_dense_cases_host.py shows on the CPU that the cases have those properties and that the NumPy restatements keep
every bound used here.

Measured on an MI355X, worst err_o(device) / max(err_o(restatement), b 2^-53) in fp64 per path of the device:
    [0, 0]  0.25   (64 x 32, kappa 1e4: both sides at the level of b 2^-53)
    [0, 1]  0.94   (200 x 40, kappa 1e5: the Newton-Schulz truncation on both sides)
    [2, 0]  0.35   for kappa <= 1e10 (65 x 33, kappa 1e10), 1.8 beyond it (64 x 32, kappa 1e14: 6.0e-6 against 3.4e-6)
so the 8 of the issue holds with room on every path.  fp32 (bounds without the restatement): worst share 0.25.

These tests found one defect, fixed with them: the eigen fallback ran its Jacobi eigensolve to 1e-14, the order of the floor 1e-14 b
that its result is divided by, and left the directions under the floor coupled.  With that tolerance the [2, 0] ratios were 10.4
(64 x 32, kappa 1e10), 20 and 33 (64 x 32, kappa 1e12 and 1e14) and 134 (65 x 33, kappa 1e14: 3.4e-4 against 2.6e-6), and
test_orthonormalise failed on [64x32-f64-svd1e+10], [64x32-f64-svd1e+12], [64x32-f64-svd1e+14] and [65x33-f64-svd1e+14] in both
paddings; the fallback now runs the eigensolve to rounding level (factor.h).

Paths are asserted as the issue lists them, with two exceptions in fp32 that test_dense_cases_host.py establishes on the CPU:
kappa = 1e7 sits at the Newton-Schulz threshold there (65 x 33: the restatement takes [0, 1], the device [0, 0]) and kappa = 1e10
keeps a condition number of only 4e8 ... 1e9 once the block is rounded to fp32 (64 x 32: the restatement's first pass is the
fallback, the device's Cholesky goes through), so in fp32 [0, 0] is asserted under MMW_FACTOR_NO_NS=1 and the fallback on the
zero-column block; the quality bounds hold on every one of these cases whatever the path.

The register form and the LDS form of k_chol_panel return the same factor and the same inverse bit for bit for b <= 32, as the
kernel's comment says.  Worst shares of the other bounds: Higham's residual bound 1.0 at b = 1 (a single square root), 0.13 from
b = 31 on; the diagonal blocks' inverses 0.03; Gram on random data 4e-4; tall GEMM 0.02 (fp64), 0.98 (fp32: the rounding of the
stored result is the bound); Cholesky-QR against numpy.linalg.qr 0.66.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dense_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

TYPES = [("f32", np.float32, _lib.F32), ("f64", np.float64, _lib.F64)]
TYPE_IDS = [t[0] for t in TYPES]


@pytest.fixture(autouse=True)
def plain_switches(monkeypatch):
    monkeypatch.delenv("MMW_CHOL_LDS", raising=False)
    monkeypatch.delenv("MMW_FACTOR_NO_NS", raising=False)


# ---- Gram -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tname,T,dt", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("K,b,ld,sym", dc.gram_cases())
def test_gram_of_integer_blocks_is_exact(K, b, ld, sym, Tname, T, dt):
    V = dc.int_block(K, b, ld, 100 * K + b, T)
    W = dc.int_block(K, b, ld, 100 * K + b + 1, T)
    G = _lib.dense_gram(V, W, b, sym, dtype=dt)
    want = V[:, :b].T @ W[:, :b]
    if sym:
        want = 0.5 * (want + want.T)
    else:
        assert b < 3 or not np.array_equal(want, want.T)  # W != V: the product is not symmetric, and is returned as it is
    assert np.array_equal(G, want), np.argwhere(G != want)[:8]
    G = _lib.dense_gram(V, V, b, sym, dtype=dt)
    assert np.array_equal(G, V[:, :b].T @ V[:, :b])


@pytest.mark.parametrize("Tname,T,dt", TYPES, ids=TYPE_IDS)
def test_gram_of_random_blocks_keeps_the_dot_product_bound(Tname, T, dt):
    K, b, ld = 1000, 129, 134
    V, W = dc.normal_block(K, b, ld, 1, T), dc.normal_block(K, b, ld, 2, T)
    Vx, Wx = V[:, :b].astype(np.longdouble), W[:, :b].astype(np.longdouble)
    want = Vx.T @ Wx
    bound = 2 * K * dc.U64 * (np.abs(Vx).T @ np.abs(Wx))
    G = _lib.dense_gram(V, W, b, 0, dtype=dt)
    share = float(np.max(np.abs(G - want) / bound))
    print("gram %s: worst share of the dot-product bound %.2e" % (Tname, share))
    assert share <= 1.0


# ---- tall GEMM --------------------------------------------------------------------------------------------------------------------
def int_matrix(b, n, ldq, seed):
    rng = np.random.default_rng(seed)
    Q = np.full((b, ldq), dc.SENTINEL)
    Q[:, :n] = rng.integers(-8, 9, size=(b, n))
    return Q


@pytest.mark.parametrize("Tname,T,dt", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("b", dc.GEMM_B)
def test_gemm_of_integer_blocks_is_exact_and_leaves_the_padding_zero(b, Tname, T, dt):
    for K, n, ld, ldq in dc.gemm_cases(b):
        V = dc.int_block(K, b, ld, 10 * K + b, T)
        Q = int_matrix(b, n, ldq, 10 * n + ldq)
        C = _lib.dense_gemm(V, Q, b, n, dtype=dt)
        tag = "K %d b %d n %d ld %d ldq %d" % (K, b, n, ld, ldq)
        assert np.array_equal(C[:, :n], V[:, :b] @ Q[:, :n]), tag
        assert np.all(C[:, n:] == 0.0), tag


@pytest.mark.parametrize("Tname,T,dt", TYPES, ids=TYPE_IDS)
def test_gemm_of_random_blocks_keeps_the_dot_product_bound(Tname, T, dt):
    K, b, n, ld, ldq = 130, 100, 65, 105, 68
    V = dc.normal_block(K, b, ld, 3, T)
    Q = dc.normal_block(b, n, ldq, 4)
    Vx, Qx = V[:, :b].astype(np.longdouble), Q[:, :n].astype(np.longdouble)
    want = Vx @ Qx
    bound = 2 * b * dc.U64 * (np.abs(Vx) @ np.abs(Qx))
    if T == np.float32:
        bound = bound + 2.0 ** -24 * np.abs(want)
    C = _lib.dense_gemm(V, Q, b, n, dtype=dt)
    share = float(np.max(np.abs(C[:, :n] - want) / bound))
    print("gemm %s: worst share of the bound %.2e" % (Tname, share))
    assert share <= 1.0 and np.all(C[:, n:] == 0.0)


# ---- Cholesky ---------------------------------------------------------------------------------------------------------------------
def check_factor(G, L, dscale, dinv, tag):
    b = G.shape[0]
    assert np.all(np.triu(L, 1) == 0.0)
    want_d = 1.0 / np.sqrt(np.diag(G))
    assert np.all(np.abs(dscale - want_d) <= 2 * dc.U64 * want_d), tag  # a square root and a division, one rounding each
    Gs = G * (dscale[:, None] * dscale[None, :])  # what k_apply_scale_sym forms, in its order
    share = dc.chol_residual_share(L, Gs)
    worst = max(dc.dinv_share(dinv[p], L, p) for p in range(dinv.shape[0]))
    print("chol %s: share of Higham's bound %.3f, of the inverse's bound %.3f" % (tag, share, worst))
    assert share <= 1.0, tag
    assert worst <= 1.0, tag
    nb = b - 32 * (dinv.shape[0] - 1)  # the last block is padded with the identity
    pad = dinv[-1].copy()
    pad[:nb, :nb] = np.eye(32)[:nb, :nb]
    assert np.array_equal(pad, np.eye(32)), tag


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("cond", dc.CHOL_COND)
@pytest.mark.parametrize("b", dc.CHOL_B)
def test_cholesky_keeps_highams_residual_bound(b, cond, lds, monkeypatch):
    if lds:
        monkeypatch.setenv("MMW_CHOL_LDS", "1")
    G = np.array(dc.spd(b, cond, 7 * b + 1))
    L, dscale, dinv, ok = _lib.dense_chol(G)
    assert ok
    check_factor(G, L, dscale, dinv, "b %d cond %.0e lds %d" % (b, cond, lds))


def test_cholesky_scales_a_gram_matrix_that_is_not_unit_diagonal():
    b = 100
    s = 2.0 ** (np.arange(b) % 7 - 3)  # powers of two: the scaled matrix is the same one, bit for bit
    G0 = np.array(dc.spd(b, 1e3, 7 * b + 1))
    G = G0 * (s[:, None] * s[None, :])
    L, dscale, dinv, ok = _lib.dense_chol(G)
    assert ok
    check_factor(G, L, dscale, dinv, "scaled b 100")


@pytest.mark.parametrize("cond", dc.CHOL_COND)
@pytest.mark.parametrize("b", [b for b in dc.CHOL_B if b <= 32])
def test_register_and_lds_panel_agree_bit_for_bit(b, cond, monkeypatch):
    G = np.array(dc.spd(b, cond, 7 * b + 1))
    L0, d0, i0, ok0 = _lib.dense_chol(G)
    monkeypatch.setenv("MMW_CHOL_LDS", "1")
    L1, d1, i1, ok1 = _lib.dense_chol(G)
    assert ok0 and ok1
    assert np.array_equal(d0, d1) and np.array_equal(L0, L1) and np.array_equal(i0, i1)


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("name", sorted(dc.BREAKDOWN))
def test_cholesky_reports_breakdown_and_recovers(name, lds, monkeypatch):
    if lds:
        monkeypatch.setenv("MMW_CHOL_LDS", "1")
    G, where = dc.breakdown_case(name)
    _, dscale, _, ok = _lib.dense_chol(G)
    assert not ok
    if name == "zero_diagonal":
        assert dscale[where] == 0.0
    good = np.array(dc.spd(G.shape[0], 1e1, 5))
    L, dscale, dinv, ok = _lib.dense_chol(good)  # the flag is reset per call
    assert ok
    check_factor(good, L, dscale, dinv, "after " + name)


# ---- orthonormalise ---------------------------------------------------------------------------------------------------------------
def orth_params():
    out = []
    for K, b in dc.ORTH_SHAPES:
        for pad in dc.ORTH_PAD:
            for Tname, T, dt in TYPES:
                for kind, kappa, no_ns in dc.orth_list(Tname):
                    out.append(pytest.param(K, b, pad, Tname, kind, kappa, no_ns,
                                            id="%dx%d+%d-%s-%s%.0e%s" % (K, b, pad, Tname, kind, kappa, "-no_ns" if no_ns else "")))
    return out


@pytest.mark.parametrize("K,b,pad,Tname,kind,kappa,no_ns", orth_params())
def test_orthonormalise(K, b, pad, Tname, kind, kappa, no_ns, monkeypatch):
    if no_ns:
        monkeypatch.setenv("MMW_FACTOR_NO_NS", "1")
    c = dc.orth_case(K, b, pad, kind, kappa, Tname, no_ns)
    T, V = c["T"], np.array(c["V"])
    out, path = _lib.dense_orth(V, b, dtype=_lib.F32 if T == np.float32 else _lib.F64)
    assert np.all(out[:, b:] == 0.0)
    Q = out[:, :b]
    assert np.all(np.isfinite(Q))
    eo, es = dc.err_o(Q), dc.err_s(V[:, :b], Q)
    print("ORTH %dx%d+%d %s %s %.0e no_ns %d: device path %s err_o %.3e err_s %.3e | restatement path %s err_o %.3e err_s %.3e | ratio %.3f"
          % (K, b, pad, Tname, kind, kappa, no_ns, path, eo, es, c["path"], c["err_o"], c["err_s"], eo / max(c["err_o"], b * dc.U64)))
    want = dc.expected_path(b, kind, kappa, Tname, no_ns)
    if want is not None:
        assert path[:len(want)] == want
    assert all(p in (0, 1, 2) for p in path) and (not no_ns or 1 not in path)
    if kind == "zero":
        lam, tol = dc.zero_case_spectrum(Q, T)
        assert abs(lam[0]) <= tol and np.all(np.abs(lam[1:] - 1.0) <= tol), (lam[:2], tol)
        assert es <= dc.orth_bounds(T, b, 0.0, 2)[1]
        return
    if kappa > 1e10:  # beyond the design's reach: no worse than the restatement by more than the 8
        assert eo <= 8.0 * c["err_o"]
        return
    bo, bs = dc.orth_bounds(T, b, c["err_o"], path[1])
    assert eo <= bo, (eo, bo)
    assert es <= bs, (es, bs)


@pytest.mark.parametrize("Tname,T,dt", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kappa", [1.0, 1e2])
@pytest.mark.parametrize("K,b", dc.ORTH_SHAPES)
def test_cholesky_qr_returns_the_qr_factor(K, b, kappa, Tname, T, dt, monkeypatch):
    monkeypatch.setenv("MMW_FACTOR_NO_NS", "1")
    V = np.array(dc.orth_case(K, b, 7, "svd", kappa, Tname, True)["V"])
    out, path = _lib.dense_orth(V, b, dtype=dt)
    assert path == [0, 0]
    diff = float(np.max(np.abs(out[:, :b] - dc.qr_positive(V[:, :b]))))
    print("qr %dx%d %s kappa %.0e: %.3e of %.3e" % (K, b, Tname, kappa, diff, dc.qr_bound(T, b, kappa)))
    assert diff <= dc.qr_bound(T, b, kappa)


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def test_malformed_arguments_are_refused_and_the_next_call_works():
    L = _lib.lib()
    V = dc.int_block(8, 4, 6, 1)
    Q = int_matrix(4, 3, 5, 2)
    G = np.array(dc.spd(4, 1e1, 3))
    pd = _lib._pd
    out = np.zeros((8, 6))
    g4, l4, d4, i4 = np.zeros((4, 4)), np.zeros((4, 4)), np.zeros(4), np.zeros((1, 32, 32))
    ok, path = _lib.C.c_int32(0), (_lib.C.c_int32 * 2)()
    okp = _lib.C.byref(ok)
    gram = lambda **k: L.mmw_dense_gram(*[k.get(n, v) for n, v in (("dev", 0), ("dt", _lib.F64), ("K", 8), ("b", 4), ("ld", 6), ("V", pd(V)), ("W", pd(V)), ("sym", 0), ("G", pd(g4)))])
    gemm = lambda **k: L.mmw_dense_gemm(*[k.get(n, v) for n, v in (("dev", 0), ("dt", _lib.F64), ("K", 8), ("b", 4), ("n", 3), ("ld", 6), ("V", pd(V)), ("ldq", 5), ("Q", pd(Q)), ("C", pd(out)))])
    chol = lambda **k: L.mmw_dense_chol(*[k.get(n, v) for n, v in (("dev", 0), ("b", 4), ("G", pd(G)), ("L", pd(l4)), ("d", pd(d4)), ("i", pd(i4)), ("ok", okp))])
    orth = lambda **k: L.mmw_dense_orth(*[k.get(n, v) for n, v in (("dev", 0), ("dt", _lib.F64), ("K", 8), ("b", 4), ("ld", 6), ("V", pd(V)), ("eps", 1e-14), ("Q", pd(out)), ("p", path))])
    shape = [{"K": 0}, {"b": 0}, {"b": 2049, "ld": 2049}, {"ld": 3}, {"dt": 7}]
    bad = [(gram, k) for k in shape + [{"V": None}, {"W": None}, {"G": None}]]
    bad += [(gemm, k) for k in shape + [{"V": None}, {"Q": None}, {"C": None}, {"n": 0}, {"ldq": 2}, {"n": 7, "ldq": 7}]]
    bad += [(chol, k) for k in [{"b": 0}, {"b": 2049}, {"G": None}, {"L": None}, {"d": None}, {"i": None}, {"ok": None}]]
    bad += [(orth, k) for k in shape + [{"V": None}, {"Q": None}, {"p": None}]]
    for call, kw in bad:
        rc = call(**kw)
        assert rc == -1, kw  # MMW_ERR_ARG
        with pytest.raises(_lib.MMWError):
            _lib.check(rc)
    with pytest.raises(_lib.MMWError):
        _lib.dense_gram(V, V, 7, 0)  # ld < b through the wrapper
    for call in (gram, gemm, chol, orth):
        assert call() == 0
    assert np.array_equal(g4, V[:, :4].T @ V[:, :4]) and np.array_equal(out[:, 4:], np.zeros((8, 2))) and ok.value == 1
    assert dc.err_o(out[:, :4]) <= 8 * 4 * dc.U64
