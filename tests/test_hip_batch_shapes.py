"""Shapes, substeps and the per-column stop of the batched fp64 solver (csrc/kernels_batch.h, `k_mmw_batch`), case by case against
SciPy's expm_multiply and the CPU oracle.

Which path of `k_mmw_batch` a case reaches follows from K, D = Z * rank_radio and the plan of exp(L/2)R:
  * the Taylor block's thread map: column tid % D, row group tid / D of NG = 512 / D groups; the 512 - NG * D threads past NG * D
    idle there (`tlive`).  NG = 1 for D > 256, 2 for 171 <= D <= 256, 3 for 128 < D <= 170;
  * `batch_sketch_rows`: lane l of a row's wave draws column pairs l + 64 i, i < 4: group i is reached by D > 128 i; an odd D draws
    its last column as the first half of a pair; rows past K leave waves idle (K < 8);
  * the plan: rho = max_i(|d_i - mu| + o_i) of L/2, then substeps nsub doubled until `plan_order(rho / nsub, tol / nsub)` fits
    max_order; no nsub <= 4 096 fits -> the fallback (4 096 substeps of order max_order).  With nsub > 1 the per-column stop
    state (c_prev, c_on) restarts at every substep and F is rescaled by e^{mu / nsub} between them;
  * the per-column stop: column c stops once ||T_{j-1} e_c||_inf + ||T_j e_c||_inf <= tol ||F e_c||_inf.

Each case names the path it reaches; (nsub, order) is the plan at the case's tol with its fixed seed (the NG / idle-thread figures
and the regime, one substep, several or the fallback, are asserted, not assumed):
  tiny                K 2,    D 4:   NG 128; waves 2..7 draw no sketch row; K < D
  d_gt_k              K 5,    D 80:  NG 6, 32 idle; D > K
  degenerate_z2 / z3  K 30,   D 4/6: E_asso = 0 (C = 2K), user 5 has only its diagonal entry, Z = 2 and 3
  odd_d               K 75,   D 3:   NG 170, 2 idle; odd D (the last column is half a pair)
  ng8                 K 243,  D 64:  NG 8
  ng3_substeps        K 300,  D 170: NG 3, 2 idle; eta 5: 2 substeps of order 14
  ng2_idle170         K 300,  D 171: NG 2, 170 idle; eta 2: one substep
  ng2_exact           K 675,  D 256: NG 2, 0 idle; sketch group 1
  ng1_group2          K 675,  D 257: NG 1, 255 idle; sketch group 2, odd D
  odd_group3          K 1000, D 511: NG 1, 1 idle; sketch group 3, odd D
  limits              K 4096, D 512: the K and D limits, nnzL 79 390 (about 72 MB of arena); sketch group 3
  substeps_norm_*     K 300,  D 24:  NG 21, 8 idle; eta 2 -> (4, 16), eta 5 -> (16, 14) at tol 1e-13; eta 2 -> (4, 13) at 1e-9
  substeps_order      K 300,  D 24:  max_order 2 -> 64 substeps of order 2
  fallback            K 300,  D 24:  max_order 1: no nsub <= 4 096 fits -> 4 096 substeps of order 1

A: the exponential alone, column by column, on an uploaded block R with an all-zero column, a column scaled by 1e-8 and a unit vector
   on the row with the most entries, against expm_multiply(L/2, R) in fp64; the plan (rho, mu, nsub, order) against a host replay.
   Bars: 1e-10 per column at tol 1e-12 / 1e-13 (the handles' fp64 shape bar; expm_multiply and a dense eigh exponential agree to
   6e-15 per column on these cases), 1e-5 at the default tol 1e-9, and for the fallback the Taylor-1 remainder bound summed over the
   4 096 substeps plus 1e-12 of rounding.
B: every loop quantity after every iteration against the oracle driven by the batch's own sketches, tol 1e-13, bar 1e-9.
C: the device sketch at every lane layout, bitwise against an fp64 handle's.
D: all case shapes in one launch, each instance bitwise the same as alone.
"""
import functools
import math

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from conftest import relerr
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

pytestmark = pytest.mark.gpu

NT = 512  # BATCH_THREADS
NSUB_MAX = 4096


def pattern_csr(b, i, vals):
    K = b.sizes[i]["K"]
    return scipy.sparse.csr_matrix((vals, b.read_i32(i, _lib.I_L_INDICES), b.read_i32(i, _lib.I_L_INDPTR)), shape=(K, K))


@functools.lru_cache(maxsize=None)
def state(name):
    if name == "er2":
        return er_contention_graph(2, 1.0, 1)
    if name == "er5":
        return er_contention_graph(5, 0.5, 1)
    if name == "degen":  # test_hip_configs.py::test_edge_cases_small_and_degenerate_graphs with the empty association relation
        S, _, h = er_contention_graph(30, 0.2, seed=3)
        S = S.tolil()
        S[5, :] = 0
        S[:, 5] = 0
        S[5, 5] = 3.7
        S = S.tocsr()
        S.eliminate_zeros()
        return S, scipy.sparse.csr_matrix((30, 30)), h
    if name.startswith("j"):
        return journal_graph(int(name[1:]), 75e-4, 0)
    if name == "er300":
        return er_contention_graph(300, 0.03, 1)
    if name == "er1000":
        return er_contention_graph(1000, 0.01, 4)
    if name == "er4096":
        return er_contention_graph(4096, 0.002, 2)
    raise KeyError(name)


# (name, state, Z, rank_radio, eta, warm-up iterations, max_order, tol of A, regime, (K, D, NG, idle threads))
CASES = [
    ("tiny", "er2", 2, 2, 0.04, 2, 16, 1e-12, "one", (2, 4, 128, 0)),
    ("d_gt_k", "er5", 40, 2, 0.04, 2, 16, 1e-12, "one", (5, 80, 6, 32)),
    ("degenerate_z2", "degen", 2, 2, 0.1, 2, 16, 1e-12, "one", (30, 4, 128, 0)),
    ("degenerate_z3", "degen", 3, 2, 0.1, 2, 16, 1e-12, "one", (30, 6, 85, 2)),
    ("odd_d", "j5", 3, 1, 0.04, 2, 16, 1e-12, "one", (75, 3, 170, 2)),
    ("ng8", "j9", 32, 2, 0.04, 2, 16, 1e-12, "one", (243, 64, 8, 0)),
    ("ng3_substeps", "er300", 85, 2, 5.0, 2, 16, 1e-12, "sub", (300, 170, 3, 2)),
    ("ng2_idle170", "er300", 171, 1, 2.0, 2, 16, 1e-12, "one", (300, 171, 2, 170)),
    ("ng2_exact", "j15", 128, 2, 0.04, 2, 16, 1e-12, "one", (675, 256, 2, 0)),
    ("ng1_group2", "j15", 257, 1, 0.04, 2, 16, 1e-12, "one", (675, 257, 1, 255)),
    ("odd_group3", "er1000", 511, 1, 0.4, 2, 16, 1e-12, "one", (1000, 511, 1, 1)),
    ("limits", "er4096", 256, 2, 0.4, 1, 16, 1e-12, "one", (4096, 512, 1, 0)),
    ("substeps_norm_eta2", "er300", 12, 2, 2.0, 2, 16, 1e-13, "sub", (300, 24, 21, 8)),
    ("substeps_norm_eta5", "er300", 12, 2, 5.0, 2, 16, 1e-13, "sub", (300, 24, 21, 8)),
    ("substeps_norm_default_tol", "er300", 12, 2, 2.0, 2, 16, 1e-9, "sub", (300, 24, 21, 8)),
    ("substeps_order", "er300", 12, 2, 0.04, 2, 2, 1e-13, "sub", (300, 24, 21, 8)),
    ("fallback", "er300", 12, 2, 0.04, 2, 1, 1e-13, "fallback", (300, 24, 21, 8)),
]
IDS = [c[0] for c in CASES]


def seed_of(case):
    """One Philox seed per instance (state, Z, rank_radio, eta): cases that differ only in the exponential's settings, and A and B of
    one case, see the same L."""
    return 100 + [c[1:5] for c in CASES].index(case[1:5])


# B runs every case at tol 1e-13; the default-tol case is then the eta 2 one
B_CASES = [c for c in CASES if c[0] != "substeps_norm_default_tol"]
FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_EXPM_INFO)


# ---- host replay of the kernel's plan (kernels_expm.h plan_order, Taylor branch; kernels_batch.h's doubling loop and fallback)
def plan_order(rho, tol, max_order):
    term = 1.0
    er = math.exp(2.0 * rho)
    for m in range(1, max_order + 1):
        term *= rho / m
        if term * rho / (m + 1) * er <= tol:
            return m
    return -1


def plan(rho, tol, max_order):
    nsub = 1
    while nsub <= NSUB_MAX:
        m = plan_order(rho / nsub, tol / nsub, max_order)
        if m > 0:
            return nsub, m
        nsub *= 2
    return NSUB_MAX, max_order


def rho_mu(L):
    """rho = max_i(|d_i - mu| + o_i) and mu = tr / K of A = L/2, as the kernel takes them from A's row sums."""
    A = scipy.sparse.csr_matrix(0.5 * L)
    K = A.shape[0]
    rows = np.repeat(np.arange(K), np.diff(A.indptr))
    on = A.indices == rows
    d = np.bincount(rows[on], weights=A.data[on], minlength=K)
    o = np.bincount(rows[~on], weights=np.abs(A.data[~on]), minlength=K)
    mu = d.sum() / K
    return max(np.max(d + o) - mu, np.max(o - d) + mu), mu


def check_regime(info, regime, name):
    nsub, order = int(info[2]), int(info[1])
    if regime == "one":
        assert nsub == 1, (name, info)
    elif regime == "sub":
        assert 1 < nsub < NSUB_MAX, (name, info)
    else:
        assert nsub == NSUB_MAX and order == 1, (name, info)


def check_shape(b, case):
    name, K, D, NG, idle = case[0], *case[9]
    assert (b.sizes[0]["K"], b.sizes[0]["D"]) == (K, D), name
    assert (NT // D, NT - (NT // D) * D) == (NG, idle), name


def new_batch(case, nit, tol):
    name, st, Z, rr, eta, warm, mo = case[:7]
    b = _lib.BatchSolver([Z], [state(st)], nit, eta, rank_radio=rr)
    b.set_expm(mo, tol)
    check_shape(b, case)
    return b


def special_block(K, D, L, seed):
    """Row-normalised Gaussian except: column D-1 all zero, column D//2 scaled by 1e-8, column 0 the unit vector on the row of L with
    the most entries."""
    R = orc.sketch_rows(np.random.default_rng(seed).standard_normal((K, D)))
    zero, tiny, unit = D - 1, D // 2, 0
    assert len({zero, tiny, unit}) == 3
    R[:, zero] = 0.0
    R[:, tiny] *= 1e-8
    R[:, unit] = 0.0
    R[int(np.argmax(np.diff(L.indptr))), unit] = 1.0
    return R, zero


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exponential_per_column_against_scipy(case):
    name, st, Z, rr, eta, warm, mo, tol, regime, _ = case
    K, D = case[9][:2]
    seed = seed_of(case)
    b = new_batch(case, warm + 1, tol)
    b.iterate(warm, None, [seed])
    R, zero = special_block(K, D, pattern_csr(b, 0, b.read(0, _lib.F_LVAL)), seed)
    b.iterate(1, [R[None]])
    assert np.array_equal(b.read(0, _lib.F_SKETCH), R)
    L = pattern_csr(b, 0, b.read(0, _lib.F_LVAL))
    got = b.read(0, _lib.F_XHALF)
    info = b.read(0, _lib.F_EXPM_INFO)
    b.close()
    # the plan
    rho, mu = rho_mu(L)
    assert abs(info[0] - rho) <= 1e-12 * rho and abs(info[3] - mu) <= 1e-12 * abs(mu), (name, info, rho, mu)
    want = plan(rho, tol, mo)
    # a condition on the inputs: the host rho is not within 1e-9 relative of a plan threshold (the plan is monotone in rho)
    assert plan(rho * (1 - 1e-9), tol, mo) == want == plan(rho * (1 + 1e-9), tol, mo), (name, rho)
    assert int(info[2]) == want[0], (name, info, want)
    assert 1 <= int(info[1]) <= want[1], (name, info, want)
    check_regime(info, regime, name)
    # the block, column by column
    ref = scipy.sparse.linalg.expm_multiply(0.5 * L, R)
    if regime == "fallback":
        n, r = NSUB_MAX, float(info[0])
        bar = n * (r / n) ** 2 / 2 * math.exp(2 * r) + 1e-12
    else:
        bar = 1e-10 if tol <= 1e-12 else 1e-5
    assert np.all(got[:, zero] == 0.0), name
    errs = np.array([np.linalg.norm(got[:, c] - ref[:, c]) / np.linalg.norm(ref[:, c]) for c in range(D) if c != zero])
    print("[batch-shapes] A %-26s K %4d D %3d plan (%d, %d) rho %.4g  max column error %.2e (bar %.1e)"
          % (name, K, D, int(info[2]), int(info[1]), info[0], errs.max(), bar))
    assert errs.max() < bar, (name, info, errs.max(), int(np.argmax(errs)))


def snapshot(b):
    f = {k: b.read(0, w) for k, w in (("e_this", _lib.F_E_THIS), ("e_accu", _lib.F_E_ACCU), ("Y", _lib.F_Y), ("lval", _lib.F_LVAL),
                                       ("xval", _lib.F_XVAL), ("X_half", _lib.F_XHALF))}
    f["xsum"] = b.read(0, _lib.F_XAVG) + f["xval"]  # the sums hold X_0 .. X_{i-1}; the oracle's when iteration i + 1 starts
    f["ysum"] = b.read(0, _lib.F_YAVG) + f["Y"]
    return f


SNAP = ("e_this", "e_accu", "Y", "lval", "xval", "X_half", "xsum", "ysum")


def oracle_for(b, i, st, Z, rr, eta, nit, seed):
    sk = [b.sketch(i, seed, it) for it in range(nit)]
    o = orc.MMWOracle(nit=nit, eta=eta, rank_radio=rr)
    o.run(Z, st, lambda it, K, D: sk[it], keep_trace=True, factor=False)
    return o


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", B_CASES, ids=[c[0] for c in B_CASES])
def test_every_iteration_follows_the_oracle(case):
    name, st, Z, rr, eta, warm, mo, _, regime, _ = case
    nit, seed = warm + 1, seed_of(case)
    b = new_batch(case, nit, 1e-13)
    o = oracle_for(b, 0, state(st), Z, rr, eta, nit, seed)
    worst = 0.0
    for i in range(nit):
        b.iterate(1, None, [seed])
        f = snapshot(b)
        for k in SNAP:
            e = relerr(f[k], o.trace[k][i])
            worst = max(worst, e)
            assert e < 1e-9, (name, i, k, e)
    info = b.read(0, _lib.F_EXPM_INFO)
    print("[batch-shapes] B %-26s plan (%d, %d)  worst field error %.2e" % (name, int(info[2]), int(info[1]), worst))
    check_regime(info, regime, name)
    if st == "degen":  # export -> factor -> round, as test_edge_cases_small_and_degenerate_graphs does for handles
        h = _lib.Solver(Z, state(st), nit, eta, dtype=_lib.F64)
        b.export(0, h)
        rank = min(29, 2 * (Z - 1))
        X = h.factor(rank)
        ref = orc.factor_xavg(o.pattern.csr(o.xavg), rank)
        assert relerr(orc.projector(X), orc.projector(ref)) < 1e-6
        rv = np.random.default_rng(1).standard_normal((2, Z, rank))
        rv /= np.linalg.norm(rv, axis=2, keepdims=True)
        z, rem = h.round(Z, X, rv)
        for a in range(2):
            zo, _, remo, _ = orc.rounding_one_attempt(Z, X, state(st), rv[a], randint=lambda Zs, size: np.full(size, -1))
            assert int(rem[a]) == remo and np.array_equal(z[a], zo.astype(np.int32))
        h.close()
    b.close()


@pytest.mark.timeout(300)
def test_set_slots_repacks_across_the_case_shapes():
    """One batch of two instances through set_slots: D = 24 -> 512 -> 3 -> 170 for the first, the reverse order for the second (rank_radio
    1, so D = Z); every leg relays out the whole arena and must match a fresh oracle run after every iteration."""
    names = ("er300", "j5")
    legs = [(24, 170), (512, 3), (3, 512), (170, 24)]
    nit, eta = 3, 0.04
    seeds = [31, 32]
    b = _lib.BatchSolver(list(legs[0]), [state(n) for n in names], nit, eta, rank_radio=1)
    b.set_expm(16, 1e-13)
    for leg, Zs in enumerate(legs):
        if leg:
            b.set_slots(list(Zs), nit)
        assert [b.sizes[i]["D"] for i in range(2)] == list(Zs)
        orcs = [oracle_for(b, i, state(n), Zs[i], 1, eta, nit, seeds[i]) for i, n in enumerate(names)]
        b.iterate(nit, None, seeds)
        for i in range(2):
            t = orcs[i].trace
            got = {"e_this": b.read(i, _lib.F_E_THIS), "e_accu": b.read(i, _lib.F_E_ACCU), "Y": b.read(i, _lib.F_Y), "lval": b.read(i, _lib.F_LVAL),
                   "xval": b.read(i, _lib.F_XVAL), "X_half": b.read(i, _lib.F_XHALF)}
            got["xsum"] = b.read(i, _lib.F_XAVG) + got["xval"]
            got["ysum"] = b.read(i, _lib.F_YAVG) + got["Y"]
            for k in SNAP:
                assert relerr(got[k], t[k][-1]) < 1e-9, (leg, i, k)
    b.close()


SKETCH_K = {2: 1.0, 5: 0.5, 7: 0.5, 9: 0.5, 600: 0.01}  # K: ER density


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D", [2, 3, 127, 129, 255, 257, 511, 512])
def test_sketch_at_every_lane_layout(D):
    """K in {2, 5, 7, 9, 600} (waves without a row, one wave of rows and a ragged tail, many rows): the device sketch is bitwise an fp64
    handle's, F_SKETCH after a device-RNG iteration is bitwise that sketch, rows have unit 2-norm and no column is left undrawn.  Odd D
    and D = 2 use rank_radio 1 (Z >= 2), the others rank_radio 2."""
    rr = 1 if D % 2 or D == 2 else 2
    Z = D // rr
    Ks = sorted(SKETCH_K)
    states = [er_contention_graph(K, SKETCH_K[K], 1) for K in Ks]
    seeds = np.array([7 + K for K in Ks], dtype=np.uint64)
    b = _lib.BatchSolver([Z] * len(Ks), states, 2, 0.04, rank_radio=rr)
    assert all(b.sizes[i]["D"] == D for i in range(len(Ks)))
    for i, (K, st) in enumerate(zip(Ks, states)):
        s = _lib.Solver(Z, st, 2, 0.04, rank_radio=rr, dtype=_lib.F64)
        for it in (0, 5):
            a = b.sketch(i, int(seeds[i]), it)
            assert a.shape == (K, D)
            assert np.array_equal(a, s.sketch(int(seeds[i]), it)), (K, D, it)
            assert np.max(np.abs(np.linalg.norm(a, axis=1) - 1.0)) <= 1e-14, (K, D, it)
            assert np.all(np.any(a != 0.0, axis=0)), (K, D, it)  # every column drawn, the last one of an odd D included
        s.close()
    b.iterate(1, None, seeds)
    for i, K in enumerate(Ks):
        assert np.array_equal(b.read(i, _lib.F_SKETCH), b.sketch(i, int(seeds[i]), 0)), (K, D)
    b.close()


@pytest.mark.timeout(300)
def test_all_case_shapes_in_one_launch_are_bitwise_alone():
    """Every case instance in ONE batch (heterogeneous K and D, per-instance eta), each bitwise the same as the instance alone.  The
    batch's rank_radio is one for all instances, so every case runs here with rank_radio 1 and Z = its D: the (K, D) shapes are the
    cases'."""
    seen, insts = set(), []
    for c in CASES:
        key = (c[1], c[9][1], c[4])
        if key not in seen:
            seen.add(key)
            insts.append((c[1], c[9][1], c[4]))
    nit, tol = 3, 1e-13
    seeds = np.arange(500, 500 + len(insts), dtype=np.uint64)
    big = _lib.BatchSolver([D for _, D, _ in insts], [state(n) for n, _, _ in insts], nit, 0.04, rank_radio=1)
    big.set_eta([eta for _, _, eta in insts])
    big.set_expm(16, tol)
    big.iterate(1, None, seeds)
    big.iterate(nit - 1, None, seeds)
    for i, (n, D, eta) in enumerate(insts):
        one = _lib.BatchSolver([D], [state(n)], nit, eta, rank_radio=1)
        one.set_expm(16, tol)
        one.iterate(nit, None, seeds[i:i + 1])
        assert big.iterations_done(i) == one.iterations_done(0) == nit
        for f in FIELDS:
            assert np.array_equal(big.read(i, f), one.read(0, f)), (n, D, eta, f)
        one.close()
    big.close()
