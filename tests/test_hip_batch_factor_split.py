"""The split of the batch factor (`BatchSolver.set_factor_split`, csrc/kernels_batch_factor_split.h): the dense Jacobi as one launch
per tournament round with several workgroups per instance must give, bit for bit, what the single launch `k_batch_factor` gives --
the factor, all five entries of its record, and the slots and remainders of the rounding that follows.

Every instance runs nit = 3 iterations on device sketches, so the run's own Xbar is factored.  The shapes and what they reach:

  K 2, 3, 5               one pair per round; the bye of an odd K
  K 31, 32, 33, 34        16 / 17 pairs: the pass boundary of a workgroup (16 pairs at a time)
  K 256, 257, 512, 513,   the boundaries of 4 / 8 / 12 / 16 row elements per lane
    768, 769
  K 300                   a journal instance
  K 1024                  the limit, once at 32 parts

No tolerance anywhere: the claim is bit equality and the comparator is the existing kernel.
"""
import functools

import numpy as np
import pytest

from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

pytestmark = pytest.mark.gpu

ETA, NIT, NATT = 0.04, 3, 3
SMALL = [2, 3, 5, 31, 32, 33, 34, 256, 257, 300, 512, 513]
LARGE = [768, 769]
CASES = [(K, p) for K in SMALL + LARGE for p in ((2, 3, 7, 32) if K < 513 else (3, 32))] + [(1024, 32)]


@functools.lru_cache(maxsize=None)
def state(K):
    if K == 300:
        return journal_graph(10, 75e-4, 0)
    return er_contention_graph(K, 1.0 if K <= 3 else 0.5 if K <= 5 else 0.2 if K <= 34 else 0.01 if K == 1024 else 0.02, 1)


def slots_of(K):
    return 2 if K <= 3 else 3 if K == 5 else 4 if K <= 34 else 12 if K == 300 else 6


def seed_of(K):
    return 500 + K


def rounds_of(K):
    return K + (K & 1) - 1


def epilogue(b, idx, take=None):
    """factor + round of a finished batch: per instance of idx (factor bytes, shape, record, slots, remainders, attempts run)."""
    b.factor(take=take)
    seeds = [seed_of(s["K"]) for s in b.sizes]
    z, rem, used = b.round(NATT, seeds, take=take, stop_at_first=False)
    out = []
    for i in idx:
        Xh = b.read_factor(i)
        out.append((Xh.tobytes(), Xh.shape, b.read(i, _lib.F_FACTOR_INFO, 5).tobytes(), b.factor_info(i), z[i].copy(), rem[i].copy(), int(used[i])))
    return out


def assert_same(got, want, what):
    assert got[1] == want[1] and got[0] == want[0], (what, "factor")
    assert got[2] == want[2], (what, "record", got[3], want[3])
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]) and got[6] == want[6], (what, "rounding")


_open = {}


def alone(K):
    """A batch of the one shape, run; left open for the cases of that shape."""
    if K not in _open:
        assert state(K)[0].shape[0] == K
        b = _lib.BatchSolver([slots_of(K)], [state(K)], NIT, ETA)
        b.iterate(NIT, None, [seed_of(K)])
        _open[K] = b
    return _open[K]


@functools.lru_cache(maxsize=None)
def single_launch(K):
    b = alone(K)
    b.set_factor_split(None)
    res = epilogue(b, [0])[0]
    assert b.factor_call() == {"path": 0, "launches": 1, "sweeps": 0, "widest": 1}
    return res


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    for b in _open.values():
        b.close()
    _open.clear()


# ---- 1. bitwise per shape
@pytest.mark.parametrize("K,parts", CASES)
def test_split_factor_is_bitwise_the_single_launch(K, parts):
    want = single_launch(K)
    b = alone(K)
    b.set_factor_split(parts)
    assert b.factor_split_parts == [parts]
    got = epilogue(b, [0])[0]
    call = b.factor_call()
    items = _lib.BatchSolver.factor_items(K, parts)
    sweeps = got[3]["sweeps"]
    print("[batch-factor-split] K %4d parts %2d: %2d items, %2d sweeps, %5d launches" % (K, parts, len(items), sweeps, call["launches"]))
    assert_same(got, want, (K, parts))
    assert 1 <= sweeps < 30
    assert call == {"path": 1, "launches": 2 + sweeps * (rounds_of(K) + 1), "sweeps": sweeps, "widest": len(items)}
    if K == 1024:
        assert parts == _lib.BATCH_MAX_PARTS and len(items) == 32


# ---- 2. one batch of all shapes up to 513
def test_mixed_batch_each_instance_is_bitwise_alone_and_the_single_launch():
    Ks = SMALL
    parts = [[1, 2, 32, 3][i % 4] for i in range(len(Ks))]
    take = [i not in (1, 8) for i in range(len(Ks))]  # K = 3 and K = 257 are left out
    idx = [i for i in range(len(Ks)) if take[i]]
    b = _lib.BatchSolver([slots_of(K) for K in Ks], [state(K) for K in Ks], NIT, ETA)
    b.iterate(NIT, None, [seed_of(K) for K in Ks])
    b.set_factor_split(parts)
    got = epilogue(b, idx, take)
    call = b.factor_call()
    assert call["path"] == 1 and call["widest"] == sum(len(_lib.BatchSolver.factor_items(Ks[i], parts[i])) for i in idx)
    for i in (1, 8):
        with pytest.raises(_lib.MMWError, match="no factor"):
            b.read_factor(i)
    b.set_factor_split(None)
    one = epilogue(b, idx, take)
    assert b.factor_call()["path"] == 0
    b.close()
    sweeps = []
    for g, o, i in zip(got, one, idx):
        assert_same(g, o, ("mixed against the single launch", Ks[i], parts[i]))
        assert_same(g, single_launch(Ks[i]), ("mixed against alone", Ks[i], parts[i]))
        sweeps.append(g[3]["sweeps"])
    print("[batch-factor-split] mixed batch: sweeps per instance", dict(zip([Ks[i] for i in idx], sweeps)))
    assert len(set(sweeps)) > 1  # instances end after different numbers of sweeps, each reporting its own
    assert call["sweeps"] == max(sweeps)


# ---- 3. parity mode
def cell5():
    b = _lib.BatchSolver([6], [journal_graph(5, 75e-4, 0)], 1, ETA)
    K = b.sizes[0]["K"]
    indptr, col = b.read_i32(0, _lib.I_L_INDPTR), b.read_i32(0, _lib.I_L_INDICES)
    return b, K, np.repeat(np.arange(K), np.diff(indptr)), col


def parity(b, parts, vals, rank):
    b.set_factor_split(parts)
    b.factor(ranks=[rank], xavg=[vals])
    return b.read_factor(0), b.read(0, _lib.F_FACTOR_INFO, 5), b.factor_info(0), b.factor_call()["path"]


def test_parity_mode_under_the_split():
    b, K, row, col = cell5()
    M = np.random.default_rng(6).standard_normal((K, K)) * 0.3
    M = M + M.T
    # the identity on the diagonal: one sweep, no rotation
    eye = (row == col).astype(np.float64)
    Xh, rec, info, path = parity(b, 3, eye, 10)
    Xh1, rec1, _, path1 = parity(b, None, eye, 10)
    assert (path, path1) == (1, 0) and info["sweeps"] == 1 and info["max_cos"] == 0.0 and info["sigma_rank"] == 1.0
    assert Xh.tobytes() == Xh1.tobytes() and rec.tobytes() == rec1.tobytes()
    # two users' rows and columns all zero, rank K - 1: a zero column in X_half
    vals = M[row, col]
    vals[row == col] = 2.0
    vals[np.isin(row, (7, 40)) | np.isin(col, (7, 40))] = 0.0
    Xh, rec, info, path = parity(b, 7, vals, K - 1)
    Xh1, rec1, _, path1 = parity(b, None, vals, K - 1)
    assert (path, path1) == (1, 0) and np.all(Xh[:, 0] == 0.0) and info["sigma_rank"] == 0.0
    assert Xh.tobytes() == Xh1.tobytes() and rec.tobytes() == rec1.tobytes()
    # rank = K
    vals = M[row, col]
    vals[row == col] = -3.0
    Xh, rec, info, path = parity(b, 32, vals, K)
    Xh1, rec1, _, path1 = parity(b, None, vals, K)
    assert (path, path1) == (1, 0) and Xh.shape == (K, K) and info["rank"] == K and info["sigma_next"] == 0.0
    assert Xh.tobytes() == Xh1.tobytes() and rec.tobytes() == rec1.tobytes()
    b.close()


# ---- 4. the setting
def test_the_setting_refusals_and_what_it_survives():
    K = 33
    want = single_launch(K)
    b = _lib.BatchSolver([slots_of(K)], [state(K)], NIT, ETA)
    seed = [seed_of(K)]
    b.set_factor_split(3)
    for bad in (0, _lib.BATCH_MAX_PARTS + 1):
        with pytest.raises(_lib.MMWError, match="instance 0"):
            b.set_factor_split(bad)
        assert b.factor_split_parts == [3]
    b.iterate(NIT, None, seed)
    assert_same(epilogue(b, [0])[0], want, "after the refusals")
    assert b.factor_call()["path"] == 1
    # it survives reset
    b.reset(NIT)
    b.iterate(NIT, None, seed)
    assert_same(epilogue(b, [0])[0], want, "after reset")
    assert b.factor_split_parts == [3] and b.factor_call()["path"] == 1
    # with the iterations' split on as well
    b.reset(NIT)
    b.set_split(2)
    b.iterate(NIT, None, seed)
    assert_same(epilogue(b, [0])[0], want, "with set_split")
    assert b.factor_call()["path"] == 1
    b.set_split(None)
    # all ones and None: the single launch
    for off in ([1], None):
        b.set_factor_split(off)
        assert b.factor_split_parts is None
        assert_same(epilogue(b, [0])[0], want, ("off", off))
        assert b.factor_call()["path"] == 0
    # it survives set_slots
    b.set_factor_split(3)
    b.set_slots([7], NIT)
    b.iterate(NIT, None, seed)
    got = epilogue(b, [0])[0]
    assert b.factor_split_parts == [3] and b.factor_call()["path"] == 1
    b.set_factor_split(None)
    assert_same(got, epilogue(b, [0])[0], "after set_slots")
    assert got[1] == (K, 12)
    # "auto" follows the slot counts' active instances
    b.set_factor_split("auto")
    assert b.factor_split_parts == [2]
    b.close()


# ---- 5. end to end
def search_states():
    return [journal_graph(c, 75e-4, s) for c in (5, 6, 7) for s in (0, 1)]


SEARCH_KW = dict(nit=150, eta=0.04, seed=7)


def test_search_many_under_the_factor_split():
    want = batch.search_many(search_states(), epilogue="batch", **SEARCH_KW)
    got = batch.search_many(search_states(), epilogue="batch", factor_split="auto", **SEARCH_KW)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["probes"] == w["probes"] and g["Z"] == w["Z"] and g["remainder"] == w["remainder"], i
        assert np.array_equal(g["z_vec"], w["z_vec"]), i


def test_single_under_the_factor_split():
    st = search_states()[2]
    res = []
    for fs in (None, 4):
        one = batch.single(st, index=2, epilogue="batch", factor_split=fs, **SEARCH_KW)
        bs = binary_search_relaxation()
        bs.verbose = False
        bs.feasibility_check_alg = one
        z_vec, Z, rem = bs.run(st)
        res.append((z_vec, Z, rem, list(one.probes), one._b.factor_call()["path"]))
        one.close()
    assert (res[0][4], res[1][4]) == (0, 1)
    assert res[0][1:4] == res[1][1:4] and np.array_equal(res[0][0], res[1][0])
