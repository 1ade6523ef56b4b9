"""The epilogue of a probe inside the batch (csrc/kernels_batch_epilogue.h): `k_batch_factor` against the CPU oracle's svds factor and
on designed spectra, `k_batch_round` slot for slot against the oracle's rounding on the kernel's own draws, independence of the batch
neighbours, reuse, and the lockstep search on top of both.

Loops run on device sketches at `set_expm(16, 1e-13)`.  The factor bar: the projector X_half X_half^T of a rank cut moves by
eps sigma_1 / gap under a perturbation eps of Xbar, so every comparison with the oracle first asserts that the cut is well-posed,
(sigma_rank - sigma_rank+1) >= 1e-4 sigma_1 by `numpy.linalg.eigvalsh` of the oracle's Xbar; then relerr(projector) < 1e-9 and the
squared column norms are the oracle's singular values, ascending, to 1e-9 relative.

The factor shapes (all of them also sit in ONE batch, where each must be bitwise what it is alone):
  k2        K 2,    Z 2,  rank 1,  nit 3   the smallest K: one pair, one round
  k5_bye    K 5,    Z 40, rank 4,  nit 3   odd K: five rounds with a bye; rank K - 1; D = 80 > K
  j5_small  K 75,   Z 6,  rank 10, nit 20  small rank, odd K
  j5_full   K 75,   Z 40, rank 74, nit 20  rank K - 1
  j7        K 147,  Z 12, rank 22, nit 20  K not a multiple of 64 (three row elements per lane, the last one ragged)
  j15       K 675,  Z 45, rank 88, nit 6   the largest sweep size: more rows than threads, 11 row elements per lane
  max_k     K 1024, Z 8,  rank 14, nit 2   MMW_BATCH_EPILOGUE_MAX_K itself: 16 row elements per lane, even K, no bye

Search: Z of `search_many(..., epilogue="batch")` minus Z of `epilogue="handle"` on the 16 sweep states, seen on the MI355X:
[0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1, -2, 0] (the two factor by different methods and round with different draws, so the
colourings differ); the test bounds it by +-2.
"""
import functools

import numpy as np
import pytest
import scipy.sparse

from conftest import relerr
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph
from test_hip_batch import colouring_remainder, sweep_states
from test_hip_batch_shapes import FIELDS

pytestmark = pytest.mark.gpu

ETA = 0.04
MAX_K = _lib.BATCH_EPILOGUE_MAX_K


@functools.lru_cache(maxsize=None)
def state(name):
    if name == "er2":
        return er_contention_graph(2, 1.0, 1)
    if name == "er5":  # test_hip_batch_shapes' tiny odd state
        return er_contention_graph(5, 0.5, 1)
    if name == "ermax":
        return er_contention_graph(MAX_K, 0.01, 4)
    if name == "erover":
        return er_contention_graph(MAX_K + 1, 0.01, 4)
    return journal_graph(int(name[1:]), 75e-4, 0)


# (name, state, Z, nit, rank the default must give)
SHAPES = [
    ("k2", "er2", 2, 3, 1),
    ("k5_bye", "er5", 40, 3, 4),
    ("j5_small", "j5", 6, 20, 10),
    ("j5_full", "j5", 40, 20, 74),
    ("j7", "j7", 12, 20, 22),
    ("j15", "j15", 45, 6, 88),
    ("max_k", "ermax", 8, 2, 14),
]
IDS = [s[0] for s in SHAPES]
SEEDS = np.arange(900, 900 + len(SHAPES), dtype=np.uint64)
NATT = 3


def new_batch(Zs, states, nit):
    b = _lib.BatchSolver(list(Zs), list(states), nit, ETA)
    b.set_expm(16, 1e-13)
    return b


def epilogue_of(b, n, seeds, nattempt=NATT, stop=False):
    """factor + round of a finished batch: per instance (X_half, info, slots[nattempt, K], rem[nattempt], used)."""
    b.factor()
    z, rem, used = b.round(nattempt, seeds, stop_at_first=stop)
    return [(b.read_factor(i), b.factor_info(i), z[i].copy(), rem[i].copy(), int(used[i])) for i in range(n)]


class AllShapes:
    """Every factor shape in ONE batch, run, factored and rounded once; the tests below share it and leave it unchanged."""

    def __init__(self):
        self.b = new_batch([s[2] for s in SHAPES], [state(s[1]) for s in SHAPES], [s[3] for s in SHAPES])
        self.b.iterate(max(s[3] for s in SHAPES), None, SEEDS)
        self.before = [[self.b.read(i, f) for f in FIELDS] for i in range(len(SHAPES))]
        self.res = epilogue_of(self.b, len(SHAPES), SEEDS)


@pytest.fixture(scope="module")
def shapes():
    s = AllShapes()
    yield s
    s.b.close()


def sigma(xbar_dense):
    return np.sort(np.abs(np.linalg.eigvalsh(xbar_dense)))[::-1]


def assert_well_posed(sig, rank, what):
    nxt = sig[rank] if rank < sig.size else 0.0
    gap = (sig[rank - 1] - nxt) / sig[0]
    assert gap >= 1e-4, (what, "the cut of the reference is ill-posed: change the seed, not the bar", gap)
    return gap


def check_factor(Xh, ref, what):
    e = relerr(orc.projector(Xh), orc.projector(ref))
    s, sref = np.sum(Xh * Xh, axis=0), np.sum(ref * ref, axis=0)
    es = np.max(np.abs(s - sref) / sref)
    assert np.all(np.diff(sref) >= 0), what  # svds hands them out ascending
    return e, es


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_factor_against_the_oracle(shapes, k):
    name, st, Z, nit, rank = SHAPES[k]
    b = shapes.b
    o = orc.MMWOracle(nit=nit, eta=ETA)
    o.run(Z, state(st), lambda it, K, D: b.sketch(k, int(SEEDS[k]), it), factor=False)
    xbar = o.pattern.csr(o.xavg)
    gap = assert_well_posed(sigma(xbar.toarray()), rank, name)
    ref = orc.factor_xavg(xbar, rank)
    Xh, info = shapes.res[k][0], shapes.res[k][1]
    assert Xh.shape == ref.shape == (state(st)[0].shape[0], rank) and info["rank"] == rank, name
    e, es = check_factor(Xh, ref, name)
    sig = np.sum(ref * ref, axis=0)
    print("[batch-epilogue] factor %-9s K %4d rank %3d gap %.1e: %d sweeps, last max|cos| %.1e, projector %.2e, singular values %.2e"
          % (name, Xh.shape[0], rank, gap, info["sweeps"], info["max_cos"], e, es))
    assert e < 1e-9 and es < 1e-9, (name, e, es)
    assert abs(info["sigma_rank"] - sig[0]) <= 1e-9 * sig[0], name
    assert info["sweeps"] < 30, (name, info)  # ended on a sweep without a rotation, not at the cap


# ---- designed Xbar on the cell-5 pattern (parity mode)
def cell5():
    b = new_batch([6], [state("j5")], 1)
    K = b.sizes[0]["K"]
    indptr, col = b.read_i32(0, _lib.I_L_INDPTR), b.read_i32(0, _lib.I_L_INDICES)
    row = np.repeat(np.arange(K), np.diff(indptr))
    return b, K, row, col, indptr


def dense_of(K, row, col, vals):
    A = np.zeros((K, K))
    A[row, col] = vals
    return A


def test_designed_negative_spectrum():
    """(a) Symmetric random values with the diagonal at -3: the spectrum lies in about [-7.3, 1.2], so the kept set by |lambda| is the
    most negative end.  A sort by signed lambda keeps the other end."""
    b, K, row, col, indptr = cell5()
    M = np.random.default_rng(5).standard_normal((K, K)) * 0.3
    M = M + M.T
    vals = M[row, col]
    vals[row == col] = -3.0
    A = dense_of(K, row, col, vals)
    lam = np.linalg.eigvalsh(A)
    rank = 10
    kept = lam[np.argsort(-np.abs(lam))[:rank]]
    assert np.sum(kept < 0) > rank // 2 and set(kept) != set(np.sort(lam)[::-1][:rank])
    assert_well_posed(sigma(A), rank, "negative spectrum")
    with pytest.raises(_lib.MMWError, match="iterations"):
        b.factor()  # the run has not ended; parity mode is the one case where that is allowed
    b.factor(xavg=[vals])
    Xh = b.read_factor(0)
    e, es = check_factor(Xh, orc.factor_xavg(scipy.sparse.csr_matrix((vals, col, indptr), shape=(K, K)), rank), "negative spectrum")
    print("[batch-epilogue] designed (a): %d of %d kept eigenvalues negative, projector %.2e, singular values %.2e"
          % (int(np.sum(kept < 0)), rank, e, es))
    assert e < 1e-9 and es < 1e-9, (e, es)
    b.close()


def test_designed_zero_rows_give_a_zero_column():
    """(b) Two users' rows and columns all zero, rank K - 1: one singular value 0 is kept.  Finite, and its column exactly zero."""
    b, K, row, col, indptr = cell5()
    M = np.random.default_rng(6).standard_normal((K, K)) * 0.3
    M = M + M.T
    vals = M[row, col]
    vals[row == col] = 2.0
    dead = (7, 40)
    vals[np.isin(row, dead) | np.isin(col, dead)] = 0.0
    b.factor(ranks=[K - 1], xavg=[vals])
    Xh, info = b.read_factor(0), b.factor_info(0)
    assert Xh.shape == (K, K - 1) and np.all(np.isfinite(Xh))
    assert np.all(Xh[:, 0] == 0.0) and np.all(np.any(Xh[:, 1:] != 0.0, axis=0))
    assert info["sigma_rank"] == 0.0 and info["sigma_next"] == 0.0
    A = dense_of(K, row, col, vals)
    lam, V = np.linalg.eigh(A)
    assert relerr(orc.projector(Xh), (V * np.abs(lam)) @ V.T) < 1e-9  # all non-zero singular values are kept
    b.close()


@pytest.mark.parametrize("rank", [1, 10, 74, 75])
def test_designed_identity_gives_projectors(rank):
    """(c) Xbar = I on the diagonal only: every X_half X_half^T is a rank-`rank` projector (idempotent to 1e-12), not the oracle's."""
    b, K, row, col, indptr = cell5()
    vals = (row == col).astype(np.float64)
    b.factor(ranks=[rank], xavg=[vals])
    Xh, info = b.read_factor(0), b.factor_info(0)
    P = orc.projector(Xh)
    assert np.max(np.abs(P @ P - P)) <= 1e-12 and abs(np.trace(P) - rank) <= 1e-12, rank
    assert info["sweeps"] == 1 and info["max_cos"] == 0.0 and info["sigma_rank"] == 1.0
    assert info["sigma_next"] == (1.0 if rank < K else 0.0)
    b.close()


# ---- rounding
ROUND_RUNS = 4  # every (cell, Z) under this many sketch / rounding seeds: which attempt first leaves nobody over depends on the draws


def rounding_batch():
    bs = binary_search_relaxation()
    states, Zs = [], []
    for _ in range(ROUND_RUNS):
        for cell in (5, 6, 7):
            st = state("j%d" % cell)
            lb, _ = bs.set_bounds(st)
            for Z in range(lb - 1, lb + 6):
                states.append(st)
                Zs.append(Z)
    return states, Zs


def test_rounding_is_the_oracles_slot_for_slot():
    """Cell 5, 6 and 7 at Z = lb - 1 ... lb + 5 (each under four seeds) in one batch, 10 attempts: every attempt's slots and remainder
    are the oracle's `rounding_one_attempt` on the batch's own factor and draws; stop_at_first is the prefix of that run up to its
    first zero.  (On the MI355X the first of the four seed sets alone had no instance whose first zero came after attempt 0.)"""
    states, Zs = rounding_batch()
    n, natt = len(states), 10
    seeds = np.arange(1000, 1000 + n, dtype=np.uint64)
    b = new_batch(Zs, states, 40)
    b.iterate(40, None, seeds)
    full = epilogue_of(b, n, seeds, natt, stop=False)
    first = []
    for i in range(n):
        Xh, _, z, rem, used = full[i]
        assert used == natt and np.all(z >= -1)
        for a in range(natt):
            rv = b.round_randv(i, int(seeds[i]), a)
            assert rv.shape == (Zs[i], Xh.shape[1]) and np.max(np.abs(np.linalg.norm(rv, axis=1) - 1.0)) <= 1e-14
            zo, _, remo, un = orc.rounding_one_attempt(Zs[i], Xh, states[i], rv)
            zo = np.where(un, -1, zo).astype(np.int32)
            assert int(rem[a]) == remo and np.array_equal(z[a], zo), (i, Zs[i], a)
        zero = np.flatnonzero(rem == 0)
        first.append(int(zero[0]) if zero.size else -1)
    print("[batch-epilogue] rounding: first attempt with remainder 0 per instance (per seed set: Z = lb-1 ... lb+5 per cell):", first)
    # the condition that makes the next block a test of the stop: both a late first zero and no zero at all occur
    assert any(f >= 1 for f in first) and any(f < 0 for f in first), first
    z, rem, used = b.round(natt, seeds, stop_at_first=True)
    for i in range(n):
        u = first[i] + 1 if first[i] >= 0 else natt
        assert int(used[i]) == u, (i, first[i])
        assert np.array_equal(z[i][:u], full[i][2][:u]) and np.array_equal(rem[i][:u], full[i][3][:u]), i
        assert np.all(z[i][u:] == -2) and np.all(rem[i][u:] == -1), i
    # take: only the flagged instances are rounded, the others report nothing
    take = [i % 3 == 0 for i in range(n)]
    z, rem, used = b.round(natt, seeds, take=take, stop_at_first=False)
    for i in range(n):
        if take[i]:
            assert np.array_equal(z[i], full[i][2]) and np.array_equal(rem[i], full[i][3]) and used[i] == natt
        else:
            assert z[i] is None and np.all(rem[i] == -1) and used[i] == 0
    b.close()


# ---- independence and reuse
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_each_shape_alone_is_bitwise_the_shape_in_the_batch(shapes, k):
    name, st, Z, nit, _ = SHAPES[k]
    one = new_batch([Z], [state(st)], nit)
    one.iterate(nit, None, SEEDS[k:k + 1])
    Xh, info, z, rem, used = epilogue_of(one, 1, SEEDS[k:k + 1])[0]
    one.close()
    w = shapes.res[k]
    assert np.array_equal(Xh, w[0]) and info == w[1], name
    assert np.array_equal(z, w[2]) and np.array_equal(rem, w[3]) and used == w[4], name


def test_second_call_repeats_and_every_field_is_untouched(shapes):
    again = epilogue_of(shapes.b, len(SHAPES), SEEDS)
    for k, (name, *_) in enumerate(SHAPES):
        for x, y in zip(again[k], shapes.res[k]):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, name
        for f, was in zip(FIELDS, shapes.before[k]):
            assert np.array_equal(shapes.b.read(k, f), was), (name, f)


def test_set_slots_then_epilogue_equals_a_fresh_batch():
    """Stale work space and a changed rank: other slot counts on the same batch, run, factor and round, against a fresh batch."""
    names, Z0, Z1, nit = ("j5", "j7", "er5"), (6, 12, 40), (9, 7, 2), 5
    seeds = np.array([41, 42, 43], dtype=np.uint64)
    sts = [state(n) for n in names]
    b = new_batch(Z0, sts, nit)
    b.iterate(nit, None, seeds)
    first = epilogue_of(b, 3, seeds)
    b.set_slots(list(Z1), nit)
    with pytest.raises(_lib.MMWError):
        b.read_factor(0)  # the factors of the old slot counts are gone
    b.iterate(nit, None, seeds)
    got = epilogue_of(b, 3, seeds)
    b.close()
    fresh = new_batch(Z1, sts, nit)
    fresh.iterate(nit, None, seeds)
    want = epilogue_of(fresh, 3, seeds)
    fresh.close()
    for i in range(3):
        assert got[i][0].shape == want[i][0].shape and np.array_equal(got[i][0], want[i][0]), names[i]
        assert got[i][1] == want[i][1] and np.array_equal(got[i][2], want[i][2]) and np.array_equal(got[i][3], want[i][3]), names[i]
    assert [g[1]["rank"] for g in first] == [10, 22, 4] and [g[1]["rank"] for g in got] == [16, 12, 2]


# ---- the search on top
@pytest.mark.timeout(300)
def test_search_with_the_batch_epilogue():
    states = sweep_states((5, 6, 7, 8), seeds=(0, 1, 2, 3))
    kw = dict(nit=40, eta=0.04, seed=7)
    results = batch.search_many(states, epilogue="batch", **kw)
    for i, st in enumerate(states):
        one = batch.single(st, index=i, epilogue="batch", **kw)
        bs = binary_search_relaxation()
        bs.verbose = False
        bs.feasibility_check_alg = one
        z_vec, Z_fin, rem = bs.run(st)
        assert results[i]["probes"] == one.probes, i
        assert results[i]["Z"] == Z_fin, i
        assert results[i]["remainder"] == 0 and rem == 0, i
        assert np.array_equal(results[i]["z_vec"], z_vec), i
        assert colouring_remainder(results[i]["z_vec"], results[i]["Z"], st) == 0, i
        one.close()
    handle = batch.search_many(states, epilogue="handle", **kw)
    diff = [results[i]["Z"] - handle[i]["Z"] for i in range(len(states))]
    print("[batch-epilogue] search: Z(batch) - Z(handle) per state:", diff)
    for i, st in enumerate(states):
        lb, ub = results[i]["bounds"]
        assert lb <= results[i]["Z"] <= ub and abs(diff[i]) <= 2, (i, diff[i])


# ---- errors
def test_factor_before_the_run_has_ended_is_refused():
    b = new_batch([6, 12], [state("j5"), state("j7")], 4)
    b.iterate(3, None, [1, 2])
    with pytest.raises(_lib.MMWError, match="instance 0 has run 3 of its 4 iterations"):
        b.factor()
    with pytest.raises(_lib.MMWError):
        b.round(2, [1, 2])  # no factor to round
    b.iterate(1, None, [1, 2])
    b.factor()
    with pytest.raises(_lib.MMWError, match="rank"):
        b.factor(ranks=[76, 5])
    b.close()


def test_an_instance_over_the_limit_is_refused_by_name_and_routed_to_a_handle():
    sts = [state("j5"), state("erover")]
    b = new_batch([6, 8], sts, 2)
    b.iterate(2, None, [1, 2])
    with pytest.raises(_lib.MMWError, match="instance 1: K = %d exceeds the epilogue limit %d" % (MAX_K + 1, MAX_K)):
        b.factor()
    with pytest.raises(_lib.MMWError):
        b.read_factor(0)  # refused before anything ran
    b.factor(take=[True, False])
    assert b.read_factor(0).shape == (75, 10)
    b.close()
    out = batch.run_with_state_many(0, [6, 8], sts, nit=2, eta=ETA, epilogue="batch")
    assert [x[1].shape for x in out] == [(75, 10), (MAX_K + 1, 14)]
    res = batch.search_many(sts, nit=2, eta=ETA, seed=3, nattempt=2, epilogue="batch")
    assert all(r is not None and r["remainder"] == 0 for r in res)
