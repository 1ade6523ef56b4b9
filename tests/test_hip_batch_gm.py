"""The sweeps' baselines inside the batch (csrc/kernels_batch_gm.h, mmw_batch_gm / mmw_batch_env_gm / mmw_batch_factor_random):
MAX_GAIN / MAX_ASSO in the stable order, one workgroup per instance, against the CPU restatement (tests/helpers/gm_restate.py), the
device GreedyHandle and the host-only batch -- slots, ZZ and remainder equal, keys bitwise --, on the batch's own states and on a
BatchEnv after a second move; the random embedding as the resident factor, rounded slot for slot against the oracle (in the index
order that the batch gives a block of unit rows, see `index_ordered`); and the Python
layer (`batch.compare_many`, `batch.online_greedy_many`) against the same steps done by hand.

The shapes are test_hip_batch_online.py's (all of them in ONE call, and each alone):
  one_ap    K 2,    A 1    everybody shares one group
  empty_ap  K 3,    A 4    APs without members, distance 0, 60 lanes idle
  j5        K 75,   A 25   cell 5
  j7        K 147,  A 49   K not a multiple of 64
  j10       K 300,  A 100  more than 64 groups
  j15       K 675,  A 225  more users than threads
  max_k     K 1024, A 64   the limit
  over      K 1025         refused by name, nothing launched
The tight slot bounds were picked by running R.slot_major on the CPU: they leave users over in every shape, for both kinds, on the
first and on the second positions.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import gm_restate as R  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import mobile_drop  # noqa: E402
from test_hip_batch_online import ETA, MSINR, RHO, SHAPES, ZS, geometry, host_state, moved_positions, new_env  # noqa: E402
from test_hip_batch_shapes import FIELDS  # noqa: E402

pytestmark = pytest.mark.gpu

BOUNDS = {"roomy": [4, 4, 20, 20, 30, 30, 64], "tight": [1, 1, 4, 4, 5, 5, 18], "unbounded": [0, -1, 0, -1, 0, -1, 0]}
KEYS = [R.gain_key, R.asso_key]
CASES = [(kind, bound, natt) for kind in (0, 1) for bound in BOUNDS for natt in (1, 3)]
IDS = ["%s-%s-natt%d" % (("gain", "asso")[k], b, n) for k, b, n in CASES]


def nofill(high, size):
    return np.full(size, -1)


class Source:
    """The shapes as one device batch (2 iterations run, so every resident field is live), the same states as a host-only batch, and
    the restatement's answers, computed once per case and shared."""

    def __init__(self, states, gm, close):
        self.states, self.gm, self.close_gm = states, gm, close
        self.host = _lib.BatchSolver(ZS, states, 2, ETA, device=-1)
        self._ref = {}

    def ref(self, case):
        if case not in self._ref:
            kind, bound, natt = case
            out = []
            for st, Z in zip(self.states, BOUNDS[bound]):
                key = KEYS[kind](st)
                z, ZZ, rem, _ = R.slot_major(key, Z, st, natt, Z <= 0, stable=True, randint=nofill)
                out.append((key, z.astype(np.int32), ZZ, rem))
            self._ref[case] = out
        return self._ref[case]

    def close(self):
        self.host.close()
        self.close_gm()


@pytest.fixture(scope="module")
def own():
    states = [host_state(*geometry(n)) for n in SHAPES]
    b = _lib.BatchSolver(ZS, states, 2, ETA)
    b.iterate(2, None, np.arange(len(SHAPES), dtype=np.uint64))
    s = Source(states, b.gm, b.close)
    s.b = b
    yield s
    s.close()


@pytest.fixture(scope="module")
def moved():
    env = new_env(SHAPES)
    env.move([geometry(n)[0] for n in SHAPES])
    env.move([moved_positions(n) for n in SHAPES])
    s = Source([env.state(i) for i in range(len(SHAPES))], env.gm, env.close)
    s.env = env
    yield s
    s.close()


def check_case(src, case, handles):
    kind, bound, natt = case
    Zs = BOUNDS[bound]
    z, ZZ, rem, keys = src.gm(kind, Zs, natt, keys=True)
    zh, ZZh, remh, keysh = src.host.gm(kind, Zs, natt, keys=True)
    for i, (st, (key, ze, ZZe, reme)) in enumerate(zip(src.states, src.ref(case))):
        n = SHAPES[i]
        assert np.array_equal(keys[i], key) and np.array_equal(keysh[i], key), (n, "key")
        print("[batch-gm] %s %s: ZZ %d (restatement %d), left over %d (%d)" % (IDS[CASES.index(case)], n, ZZ[i], ZZe, rem[i], reme))
        assert np.array_equal(z[i], ze) and ZZ[i] == ZZe and rem[i] == reme, n
        assert np.array_equal(z[i], zh[i]) and ZZ[i] == ZZh[i] and rem[i] == remh[i], n
        if handles:
            g = _lib.GreedyHandle(st)
            zg, ZZg, remg = g.run(key, Zs[i] if Zs[i] > 0 else st[0].shape[0], natt)
            g.close()
            assert np.array_equal(z[i], zg) and ZZ[i] == ZZg and rem[i] == remg, n
        R.check_slots(st, z[i], z[i] >= 0)
        assert (rem[i] > 0) == (bound == "tight"), n
    return z, ZZ, rem, keys


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_own_states_match_the_restatement_the_handle_and_the_host_batch(own, case):
    check_case(own, case, handles=True)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_moved_environment_matches_the_restatement_and_the_host_batch(moved, case):
    check_case(moved, case, handles=case[2] == 1)


def test_each_shape_alone_and_a_partial_take_are_bitwise_the_full_call(own, moved):
    Zs = BOUNDS["tight"]
    for kind in (0, 1):
        full = own.gm(kind, Zs, 3, keys=True)
        fenv = moved.gm(kind, Zs, 3, keys=True)
        for i, n in enumerate(SHAPES):
            one = _lib.BatchSolver([ZS[i]], [own.states[i]], 2, ETA)
            z1, ZZ1, rem1, k1 = one.gm(kind, [Zs[i]], 3, keys=True)
            one.close()
            assert np.array_equal(z1[0], full[0][i]) and ZZ1[0] == full[1][i] and rem1[0] == full[2][i] and np.array_equal(k1[0], full[3][i]), n
            env = new_env([n])
            env.move([moved_positions(n)])
            z1, ZZ1, rem1, k1 = env.gm(kind, [Zs[i]], 3, keys=True)
            env.close()
            assert np.array_equal(z1[0], fenv[0][i]) and ZZ1[0] == fenv[1][i] and rem1[0] == fenv[2][i] and np.array_equal(k1[0], fenv[3][i]), n
        take = [True, False, True, False, False, True, True]
        for src, ful in ((own, full), (moved, fenv)):
            z, ZZ, rem, keys = src.gm(kind, Zs, 3, take=take, keys=True)
            for i, t in enumerate(take):
                if t:
                    assert np.array_equal(z[i], ful[0][i]) and ZZ[i] == ful[1][i] and rem[i] == ful[2][i] and np.array_equal(keys[i], ful[3][i])
                else:
                    assert z[i] is None and keys[i] is None and ZZ[i] == -1 and rem[i] == -1


def test_refusals_by_name(own, moved):
    with pytest.raises(_lib.MMWError, match="kind must be 0"):
        own.gm(2, 4)
    with pytest.raises(_lib.MMWError, match="nattempt must be >= 1"):
        moved.gm(0, 4, 0)
    with pytest.raises(_lib.MMWError, match="no instance takes part"):
        moved.gm(0, 4, 1, take=[False] * len(SHAPES))
    env = new_env(["j5"])
    with pytest.raises(_lib.MMWError, match="no positions yet"):
        env.gm(0, 4)
    env.close()
    # over the limit: the batch itself holds K = 1025, its gm and factor_random do not
    over = _lib.BatchSolver([6, 8], [own.states[2], host_state(*geometry("over"))], 2, ETA)
    with pytest.raises(_lib.MMWError, match="instance 1: K = 1025 exceeds the limit 1024"):
        over.gm(0, 8)
    with pytest.raises(_lib.MMWError, match="instance 1: K = 1025 exceeds the epilogue limit 1024"):
        over.factor_random([1, 2])
    z, ZZ, rem = over.gm(0, 8, take=[True, False])
    assert np.array_equal(z[0], own.gm(0, 8, take=[False, False, True, False, False, False, False])[0][2]) and z[1] is None
    over.close()


# ---- the random embedding as the resident factor
RAND = ["one_ap", "j7", "j15"]


def index_ordered(fac):
    """The block as the oracle has to be given it.  Every row of the embedding has norm 1 to the last bit or two, so the oracle's
    visiting order `argsort(-norm)` sorts rounding noise with an unstable sort: it is no property of the block (it changes with the
    summation order of the norm and with NumPy's sort).  The batch visits such a block in index order (ties to the lower index,
    kernels_batch_epilogue.h).  Row k scaled by 2^(K/2 - k) states that order to the oracle and nothing else: a power of two scales
    every product and every sum of column k of `inprod` exactly, so each user's preference order is bitwise the unscaled block's."""
    K = fac.shape[0]
    assert np.max(np.abs(np.linalg.norm(fac, axis=1) - 1.0)) <= 1e-15 and K // 2 + 1 < 500  # 2^(2 * 500) is still a double
    return np.ldexp(fac, (K // 2 - np.arange(K))[:, None])



def test_factor_random_is_the_sketch_and_rounds_like_the_oracle_and_nothing_else_moves(own, moved):
    idx = [SHAPES.index(n) for n in RAND]
    take = [i in idx for i in range(len(SHAPES))]
    b = own.b
    before = [[b.read(i, f) for f in FIELDS] for i in range(len(SHAPES))]
    seeds = np.arange(900, 900 + len(SHAPES), dtype=np.uint64)
    b.gm(0, BOUNDS["tight"], 3)
    b.factor_random(seeds, take=take)
    natt = 2
    fac = {}
    for i in idx:
        sz = b.sizes[i]
        fac[i] = b.read_factor(i)
        assert fac[i].shape == (sz["K"], sz["D"]) and np.array_equal(fac[i], b.sketch(i, int(seeds[i]), 0)), SHAPES[i]
        assert b.factor_info(i) == {"sweeps": 0, "max_cos": 0.0, "rank": sz["D"], "sigma_rank": 0.0, "sigma_next": 0.0}
    assert b.sizes[idx[0]]["D"] > b.sizes[idx[0]]["K"]  # one_ap: D = 4 columns for K = 2 users
    with pytest.raises(_lib.MMWError, match="instance 2 has no factor"):
        b.round(natt, seeds, take=[False, False, True] + [False] * 4)
    for states, res in ((own.states, b.round(natt, seeds, take=take, stop_at_first=False)),
                        (moved.states, b.round_env(moved.env, natt, seeds, take=take, stop_at_first=False))):
        z, rem, used = res
        for i in idx:
            assert used[i] == natt
            for a in range(natt):
                rv = b.round_randv(i, int(seeds[i]), a)
                zo, _, remo, un = orc.rounding_one_attempt(ZS[i], index_ordered(fac[i]), states[i], rv)
                zo = np.where(un, -1, zo).astype(np.int32)
                print("[batch-gm] rand %s attempt %d: left over %d (oracle %d), %d slots differ" % (SHAPES[i], a, rem[i][a], remo, int(np.sum(z[i][a] != zo))))
                assert int(rem[i][a]) == remo and np.array_equal(z[i][a], zo), (SHAPES[i], a)
    for i in range(len(SHAPES)):
        for f, was in zip(FIELDS, before[i]):
            assert np.array_equal(b.read(i, f), was), (SHAPES[i], f)
    # a factor of the run replaces the embedding, and the other way round
    b.factor(take=take)
    assert b.read_factor(idx[1]).shape[1] == b.factor_info(idx[1])["rank"] < b.sizes[idx[1]]["D"]
    b.factor_random(seeds, take=take)
    assert np.array_equal(b.read_factor(idx[1]), fac[idx[1]])


# ---- the Python layer
def drops():
    return [mobile_drop(5, RHO, 3), mobile_drop(7, RHO, 1)]


def test_compare_many_is_the_same_steps_done_by_hand():
    kw = dict(nit=20, eta=ETA, seed=5, nattempt=10)
    res = batch.compare_many(drops(), **kw)
    hand = drops()
    B = len(hand)
    env = _lib.BatchEnv([d.ap_locs for d in hand], [d.K for d in hand], min_sinr=MSINR)
    env.move([d.sta_locs for d in hand])
    states = [env.state(i) for i in range(B)]
    found = batch.search_many(states, epilogue="batch", **kw)
    Zs = [r["Z"] for r in found]
    b = _lib.BatchSolver(Zs, states, 20, ETA)
    zs = {"mmw": [r["z_vec"] for r in found]}
    sd = [np.array([batch.probe_seed(5, i, 0x40000 | m) for i in range(B)], dtype=np.uint64) for m in range(3)]
    b.factor_random(sd[0])
    z, rem, used = b.round_env(env, 10, sd[0])
    zs["rand"] = [batch._finish(z, rem, used, i, Zs[i], int(sd[0][i]))[0] for i in range(B)]
    for m, name in ((1, "mgain"), (2, "masso")):
        slot, _, rem = env.gm(m - 1, Zs, 1)
        zs[name] = []
        for i in range(B):
            zv = slot[i].astype(np.float64)
            un = slot[i] < 0
            zv[un] = np.random.default_rng(int(sd[m][i])).integers(0, Zs[i], int(un.sum()))
            zs[name].append(zv)
    for i in range(B):
        assert res[i]["Z"] == Zs[i] and res[i]["probes"] == found[i]["probes"] and sorted(res[i]["bler"]) == ["masso", "mgain", "mmw", "rand"]
    for name in ("mmw", "rand", "mgain", "masso"):
        _, bler = env.evaluate(zs[name], Zs)
        for i in range(B):
            assert np.all((0 <= zs[name][i]) & (zs[name][i] < Zs[i]))
            assert np.array_equal(res[i]["bler"][name], bler[i]), (name, i)
    # baselines_many on the batch's own states: the same methods through `round` and `BatchSolver.gm`
    base = batch.baselines_many(b, Zs, seed=5)
    z, rem, used = b.round(10, sd[0])
    slot, _, remg = b.gm(0, Zs, 1)
    for i in range(B):
        f = batch._finish(z, rem, used, i, Zs[i], int(sd[0][i]))
        assert np.array_equal(base[i]["rand"][0], f[0]) and base[i]["rand"][1:] == f[1:]
        assert base[i]["mgain"][1:] == (Zs[i], int(remg[i])) and np.array_equal(base[i]["mgain"][0][slot[i] >= 0], slot[i][slot[i] >= 0])
    b.close()
    env.close()


def test_online_greedy_many_is_the_same_steps_done_by_hand():
    npts, step, spd = 3, 1e6, 20.0
    moving = drops()
    timings = []
    res = batch.online_greedy_many(moving, n_points=npts, step_us=step, mob_spd_meter_s=spd, seed=5, timings=timings)
    hand = drops()
    B = len(hand)
    env = _lib.BatchEnv([d.ap_locs for d in hand], [d.K for d in hand], min_sinr=MSINR)
    env.move([d.sta_locs for d in hand])
    slot, ZZ, rem = env.gm(0, [-1] * B)
    st = [env.state(i) for i in range(B)]
    zv = []
    for i in range(B):
        key = R.gain_key(st[i])
        ze, ZZe, reme, _ = R.slot_major(key, -1, st[i], 1, True, stable=True, randint=nofill)
        assert np.array_equal(slot[i], ze.astype(np.int32)) and ZZ[i] == ZZe and rem[i] == reme
        v = slot[i].astype(np.float64)
        un = slot[i] < 0
        v[un] = np.random.default_rng(batch.probe_seed(5, i, 0x40000 | 1)).integers(0, int(ZZ[i]), int(un.sum()))
        zv.append(v)
    for p in range(npts):
        env.move([d.sta_locs for d in hand])
        _, bler = env.evaluate(zv, [int(x) for x in ZZ])
        for i in range(B):
            assert np.array_equal(res[i]["z_vec"][p], zv[i]) and res[i]["remainder"][p] == rem[i] and np.array_equal(res[i]["bler"][p], bler[i]), (p, i)
        for d in hand:
            d.step_time(step, spd, 1e4)
    env.close()
    for i in range(B):
        assert res[i]["Z"] == ZZ[i] and res[i]["probes"] == [] and res[i]["bler"].shape == (npts, hand[i].K)
    assert len(timings) == npts and all(np.array_equal(d.sta_locs, h.sta_locs) for d, h in zip(moving, hand))
