"""The online sweeps inside the batch (csrc/kernels_batch_env.h, mmw_batch_round_env): the generator and the scorer with one
workgroup per instance against the single-instance device path (bitwise), the host restatement (patterns equal, values 1e-12: the
bar of test_hip_env.py) and the reference's own outputs (tests/golden/online.npz); the batch's rounding on MOVED states slot for
slot against the oracle on the kernel's own factor and draws; independence of the batch neighbours; and `batch.online_many`
against the same steps done by hand.

The shapes (all of them sit in ONE BatchEnv, and each also runs alone):
  one_ap    K 2,    A 1    Q is the 2-clique; every user is in every row
  empty_ap  K 3,    A 4    hand-placed: two APs without a member, one station exactly on an AP (distance 0), 60 lanes idle
  j5        K 75,   A 25   cell 5
  j7        K 147,  A 49   K not a multiple of 64
  j10       K 300,  A 100  A > 64: a second trip of the lane loop (the online sweeps' size)
  j15       K 675,  A 225  more users than threads
  max_k     K 1024, A 64   the limit: a uniform drop on the cell-8 grid, seed 4
  over      K 1025         refused by name, nothing launched
"""
import functools

import numpy as np
import pytest

from conftest import load_golden
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib, batch, scorer
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation
from sig_sdp_mmw_amd.graphs import _state_at, journal_geometry, min_sinr_dec, mobile_drop
from test_hip_batch_shapes import FIELDS
from test_hip_env import assert_scores_match, same_csr

pytestmark = pytest.mark.gpu

RHO = 75e-4
ETA = 0.04
MAX_K = _lib.BATCH_EPILOGUE_MAX_K
MSINR = min_sinr_dec()


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(sta_locs, ap_locs) of a shape; the arrays are shared and left unchanged."""
    if name == "one_ap":
        return np.array([[3.0, 4.0], [15.5, 12.25]]), np.array([[10.0, 10.0]])
    if name == "empty_ap":
        ap = np.array([[10.0, 10.0], [30.0, 10.0], [10.0, 30.0], [30.0, 30.0]])
        return np.array([[10.0, 10.0], [12.0, 11.0], [29.0, 33.0]]), ap
    if name in ("max_k", "over"):
        K = MAX_K + (name == "over")
        return np.random.default_rng(4).uniform(0.0, 160.0, size=(K, 2)), journal_geometry(8, RHO, 0)[1]
    cell, seed = {"j5": (5, 3), "j7": (7, 1), "j10": (10, 0), "j15": (15, 0)}[name]
    return journal_geometry(cell, RHO, seed)


SHAPES = ["one_ap", "empty_ap", "j5", "j7", "j10", "j15", "max_k"]
ZS = [2, 2, 6, 12, 12, 20, 8]  # slot counts for the scorer and for the rounding of every shape


def new_env(names):
    return _lib.BatchEnv([geometry(n)[1] for n in names], [geometry(n)[0].shape[0] for n in names], min_sinr=MSINR)


def moved_positions(name):
    """Where the stations of a shape stand for the second move: the reference's cell-5 walk at 50 m/s for j5, a walk of the drop's own
    for the other cells, the hand-placed ones shifted."""
    sta, _ = geometry(name)
    if name == "j5":
        return load_golden("online")["c5s3_sta_locs"][2]
    if name[0] == "j":
        cell, seed = {"j7": (7, 1), "j10": (10, 0), "j15": (15, 0)}[name]
        d = mobile_drop(cell, RHO, seed)
        d.step_time(3e6, 50.0)
        return d.sta_locs
    return sta[::-1] + 1.5


def host_state(sta, ap):
    return _state_at(np.asarray(sta), np.asarray(ap))[0]


def bitwise_state(a, b):
    return all(np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices) and np.array_equal(x.data, y.data)
               for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2], b[2])


def colouring(name, Z):
    K = geometry(name)[0].shape[0]
    z = np.random.default_rng(K).integers(0, Z, size=K).astype(float)
    z[::7] = Z + 2  # users outside every slot keep the floor value
    if K > 2:
        z[1] = -1.0
    return z


class AllShapes:
    """Every shape in ONE BatchEnv, moved once and scored once; the tests below share it and do not move it."""

    def __init__(self):
        self.env = new_env(SHAPES)
        self.env.move([geometry(n)[0] for n in SHAPES])
        self.states = [self.env.state(i) for i in range(len(SHAPES))]
        self.z = [colouring(n, Z) for n, Z in zip(SHAPES, ZS)]
        self.sinr, self.bler = self.env.evaluate(self.z, ZS)


@pytest.fixture(scope="module")
def shapes():
    s = AllShapes()
    yield s
    s.env.close()


# ---- generator
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPES)
def test_state_is_the_single_instance_generators_and_the_hosts(shapes, k):
    sta, ap = geometry(SHAPES[k])
    one = _lib.DeviceEnv(sta, ap, min_sinr=MSINR)
    assert bitwise_state(shapes.states[k], one.state()), SHAPES[k]  # the same device arithmetic
    one.close()
    S, Q, h = shapes.states[k]
    S0, Q0, h0 = host_state(sta, ap)
    same_csr(S, S0, 1e-12)
    same_csr(Q, Q0, 0)
    np.testing.assert_allclose(h, h0, rtol=1e-12)
    assert S.has_sorted_indices and Q.has_sorted_indices
    sz = shapes.env.sizes(k)
    assert (sz["K"], sz["A"], sz["nnzS"], sz["nnzQ"]) == (sta.shape[0], ap.shape[0], S0.nnz, Q0.nnz)


def test_hand_placed_shapes_are_what_they_claim():
    S, Q, h = host_state(*geometry("one_ap"))
    assert Q.toarray().tolist() == [[0, 1], [1, 0]] and S.nnz == 4
    sta, ap = geometry("empty_ap")
    rx = scorer.receive_power(sta, ap)
    assert sorted(set(np.argmax(rx, axis=1))) == [0, 3] and np.array_equal(sta[0], ap[0])


def test_a_second_and_a_third_move_equal_a_fresh_environment():
    """The lists change size with every move (grow-only arena): away and back again, so every instance that changes size both grows
    and shrinks; each time the states are bitwise those of an environment that never held anything else."""
    env = new_env(SHAPES)
    first = [geometry(n)[0] for n in SHAPES]
    second = [moved_positions(n) for n in SHAPES]
    nnz = []
    for pos in (first, second, first, second):
        env.move(pos)
        fresh = new_env(SHAPES)
        fresh.move(pos)
        for i, n in enumerate(SHAPES):
            assert bitwise_state(env.state(i), fresh.state(i)), n
        fresh.close()
        nnz.append([env.sizes(i)["nnzS"] for i in range(len(SHAPES))])
    env.close()
    S0 = host_state(second[2], geometry("j5")[1])[0]
    assert nnz[1][2] == S0.nnz
    grew = [b > a for a, b in zip(nnz[0], nnz[1])]
    shrank = [b < a for a, b in zip(nnz[0], nnz[1])]
    print("[batch-online] nnz(S) per shape, first positions:", nnz[0], "second:", nnz[1])
    assert (any(grew) or any(shrank)) and nnz[2] == nnz[0] and nnz[3] == nnz[1]


def test_nothing_answers_before_the_first_move_and_over_the_limit_is_refused_by_name():
    env = new_env(["j5"])
    for call in (lambda: env.state(0), lambda: env.sizes(0), lambda: env.evaluate([np.zeros(75)], [3])):
        with pytest.raises(_lib.MMWError, match="no positions yet"):
            call()
    env.close()
    with pytest.raises(_lib.MMWError, match="instance 1: K = %d exceeds the limit %d" % (MAX_K + 1, MAX_K)):
        new_env(["j5", "over"])


# ---- scorer
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPES)
def test_scores_match_the_host_scorer(shapes, k):
    sta, ap = geometry(SHAPES[k])
    rx = scorer.receive_power(sta, ap)
    z, Z = shapes.z[k], ZS[k]
    assert np.any(z >= Z)
    assert_scores_match(np.argmax(rx, axis=1), z, Z, shapes.sinr[k], shapes.bler[k], scorer.evaluate_sinr(rx, z, Z), scorer.evaluate_bler(rx, z, Z))
    one = _lib.DeviceEnv(sta, ap, min_sinr=MSINR)
    s1, b1 = one.evaluate(z, Z)
    one.close()
    # the SINR is rounded sums and one division in both kernels, so it is the single-instance scorer's bit for bit (the model on top
    # of it leaves its multiply-adds to the compiler: held to the rule above only)
    assert np.array_equal(s1, shapes.sinr[k]), SHAPES[k]


def test_scores_match_the_reference_on_its_moved_stations():
    g = load_golden("online")
    names = ["c5s3", "c5s0"]
    env = _lib.BatchEnv([g[n + "_ap_locs"] for n in names], [75, 75], min_sinr=MSINR)
    K = 75
    for p in range(int(g["calls"]) + 1):
        pos = [g[n + "_sta_locs"][p] for n in names]
        env.move(pos)
        for suffix, zs, Zs in (("", [g[n + "_z_vec"][p] for n in names], [int(g[n + "_Z"]) for n in names]),
                               ("_bad", [(np.arange(K) % 3).astype(float)] * 2, [3, 3])):
            sinr, bler = env.evaluate(zs, Zs)
            for i, n in enumerate(names):
                asso = np.argmax(scorer.receive_power(pos[i], g[n + "_ap_locs"]), axis=1)
                assert_scores_match(asso, np.asarray(zs[i]), Zs[i], sinr[i], bler[i], g[n + "_sinr" + suffix][p], g[n + "_bler" + suffix][p])
    env.close()


# ---- rounding on a moved state
def test_rounding_on_moved_states_is_the_oracles_and_leaves_the_batch_alone():
    """j5 (seed 3, walking at 20 m/s) and j7 (seed 1, at 1 m/s) at Z = lower bound + 3, factored once at the drop; then four moves of
    3 s each.  Every point, every one of 10 attempts: slots and remainder are the oracle's `rounding_one_attempt` on the batch's
    own factor and draws and the MOVED state; stop_at_first is the prefix up to the first zero."""
    drops = [mobile_drop(5, RHO, 3), mobile_drop(7, RHO, 1)]
    speeds = [20.0, 1.0]
    states = [d.state() for d in drops]
    bs = binary_search_relaxation()
    Zs = [bs.set_bounds(st)[0] + 3 for st in states]
    seeds = np.array([77, 78], dtype=np.uint64)
    natt = 10
    b = _lib.BatchSolver(Zs, states, 40, ETA)
    b.set_expm(16, 1e-13)
    b.iterate(40, None, seeds)
    b.factor()
    Xh = [b.read_factor(i) for i in range(2)]
    before = [[b.read(i, f) for f in FIELDS] for i in range(2)]
    own = b.round(natt, seeds, stop_at_first=False)
    env = _lib.BatchEnv([d.ap_locs for d in drops], [d.K for d in drops], min_sinr=MSINR)
    rems = []
    for p in range(4):
        for d, v in zip(drops, speeds):
            d.step_time(3e6, v)
        env.move([d.sta_locs for d in drops])
        sd = seeds + np.uint64(100 * (p + 1))
        z, rem, used = b.round_env(env, natt, sd, stop_at_first=False)
        zs, rs, us = b.round_env(env, natt, sd, stop_at_first=True)
        for i in range(2):
            moved = drops[i].state()
            same_csr(env.state(i)[0], moved[0], 1e-12)
            assert used[i] == natt and np.all(z[i] >= -1)
            for a in range(natt):
                rv = b.round_randv(i, int(sd[i]), a)
                zo, _, remo, un = orc.rounding_one_attempt(Zs[i], Xh[i], env.state(i), rv)
                zo = np.where(un, -1, zo).astype(np.int32)
                assert int(rem[i][a]) == remo and np.array_equal(z[i][a], zo), (p, i, a)
            zero = np.flatnonzero(rem[i] == 0)
            u = int(zero[0]) + 1 if zero.size else natt
            assert int(us[i]) == u and np.array_equal(zs[i][:u], z[i][:u]) and np.array_equal(rs[i][:u], rem[i][:u]), (p, i)
            assert np.all(zs[i][u:] == -2) and np.all(rs[i][u:] == -1), (p, i)
            rems.append(rem[i].copy())
    rems = np.concatenate(rems)
    print("[batch-online] remainders over 4 points x 2 drops x 10 attempts: %d zero, %d non-zero" % (np.sum(rems == 0), np.sum(rems > 0)))
    assert np.any(rems == 0) and np.any(rems > 0)
    # the batch is as it was: every field, the factor, and its own rounding
    for i in range(2):
        for f, was in zip(FIELDS, before[i]):
            assert np.array_equal(b.read(i, f), was), (i, f)
        assert np.array_equal(b.read_factor(i), Xh[i])
    again = b.round(natt, seeds, stop_at_first=False)
    assert all(np.array_equal(x, y) for x, y in zip(again[0], own[0])) and np.array_equal(again[1], own[1]) and np.array_equal(again[2], own[2])
    # an environment of other users is refused by name
    other = _lib.BatchEnv([drops[1].ap_locs, drops[1].ap_locs], [147, 147], min_sinr=MSINR)
    other.move([drops[1].sta_locs, drops[1].sta_locs])
    with pytest.raises(_lib.MMWError, match="instance 0: K = 75 in the batch, 147 in the environment"):
        b.round_env(other, natt, seeds)
    z1, _, _ = b.round_env(other, natt, seeds, take=[False, True], stop_at_first=False)
    z2, _, _ = b.round_env(env, natt, seeds, take=[False, True], stop_at_first=False)
    assert z1[0] is None and np.array_equal(z1[1], z2[1])
    other.close()
    env.close()
    b.close()


# ---- independence
class Rounded:
    """A batch of the given shapes built from their host states, run 2 iterations, factored, and rounded against a BatchEnv of the
    same shapes at their SECOND positions."""

    def __init__(self, names, Zs, seeds):
        self.b = _lib.BatchSolver(Zs, [host_state(*geometry(n)) for n in names], 2, ETA)
        self.b.iterate(2, None, seeds)
        self.b.factor()
        self.env = new_env(names)
        self.env.move([moved_positions(n) for n in names])
        self.z, self.rem, self.used = self.b.round_env(self.env, 2, seeds, stop_at_first=False)
        self.state = [self.env.state(i) for i in range(len(names))]

    def close(self):
        self.env.close()
        self.b.close()


@pytest.fixture(scope="module")
def rounded():
    r = Rounded(SHAPES, ZS, np.arange(300, 300 + len(SHAPES), dtype=np.uint64))
    yield r
    r.close()


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPES)
def test_each_shape_alone_is_bitwise_the_shape_in_the_batch(shapes, rounded, k):
    n = SHAPES[k]
    env = new_env([n])
    env.move([geometry(n)[0]])
    assert bitwise_state(env.state(0), shapes.states[k]), n
    sinr, bler = env.evaluate([shapes.z[k]], [ZS[k]])
    assert np.array_equal(sinr[0], shapes.sinr[k]) and np.array_equal(bler[0], shapes.bler[k]), n
    env.close()
    one = Rounded([n], [ZS[k]], np.array([300 + k], dtype=np.uint64))
    assert bitwise_state(one.state[0], rounded.state[k]), n
    assert np.array_equal(one.z[0], rounded.z[k]) and np.array_equal(one.rem[0], rounded.rem[k]) and one.used[0] == rounded.used[k], n
    assert np.all(one.z[0] >= -1)
    one.close()


# ---- online_many
def online_drops():
    return [mobile_drop(c, RHO, s) for c in (5, 7) for s in range(4)]


def test_online_many_is_the_same_steps_done_by_hand():
    kw = dict(nit=30, eta=ETA, seed=5, nattempt=10)
    npts, step, spd = 3, 1e6, 20.0
    drops = online_drops()
    start = [d.sta_locs.copy() for d in drops]
    res = batch.online_many(drops, n_points=npts, step_us=step, mob_spd_meter_s=spd, **kw)
    assert all(not np.array_equal(d.sta_locs, s) for d, s in zip(drops, start))  # the drops walked
    # by hand
    hand = online_drops()
    B = len(hand)
    states = [d.state() for d in hand]
    found = batch.search_many(states, epilogue="batch", **kw)
    Zs = [r["Z"] for r in found]
    for i in range(B):
        assert res[i]["Z"] == Zs[i] and res[i]["probes"] == found[i]["probes"], i
        assert res[i]["z_vec"].shape == res[i]["bler"].shape == (npts, hand[i].K) and res[i]["remainder"].shape == (npts,)
    b = _lib.BatchSolver(Zs, states, kw["nit"], ETA)
    b.iterate(kw["nit"], None, np.array([batch.probe_seed(5, i, len(found[i]["probes"])) for i in range(B)], dtype=np.uint64))
    b.factor()
    env = _lib.BatchEnv([d.ap_locs for d in hand], [d.K for d in hand], min_sinr=MSINR)
    for p in range(npts):
        env.move([d.sta_locs for d in hand])
        seeds = np.array([batch.probe_seed(5, i, 0x80000 | p) for i in range(B)], dtype=np.uint64)
        z, rem, used = b.round_env(env, 10, seeds)
        fin = [batch._finish(z, rem, used, i, Zs[i], int(seeds[i])) for i in range(B)]
        _, bler = env.evaluate([f[0] for f in fin], Zs)
        for i in range(B):
            assert np.array_equal(res[i]["z_vec"][p], fin[i][0]) and res[i]["remainder"][p] == fin[i][2], (p, i)
            assert np.array_equal(res[i]["bler"][p], bler[i]), (p, i)
            assert np.all((0 <= fin[i][0]) & (fin[i][0] < Zs[i]))
        for d in hand:
            d.step_time(step, spd)
    env.close()
    b.close()
    assert all(np.array_equal(d.sta_locs, h.sta_locs) for d, h in zip(drops, hand))


def test_online_many_with_step_zero_leaves_the_positions_untouched():
    drops = online_drops()[:2] + online_drops()[4:6]
    start = [(d.sta_locs.copy(), d.sta_dirs.copy()) for d in drops]
    res = batch.online_many(drops, n_points=2, step_us=0, mob_spd_meter_s=20.0, nit=30, eta=ETA, seed=5)
    for d, (loc, dr) in zip(drops, start):
        assert np.array_equal(d.sta_locs, loc) and np.array_equal(d.sta_dirs, dr)
    found = batch.search_many([d.state() for d in drops], nit=30, eta=ETA, seed=5, epilogue="batch")
    assert [r["Z"] for r in res] == [r["Z"] for r in found] and [r["probes"] for r in res] == [r["probes"] for r in found]
    # per-instance step: only the instances given a time walk
    batch.online_many(drops, n_points=1, step_us=[0, 1e6, 0, 1e6], mob_spd_meter_s=20.0, nit=30, eta=ETA, seed=5)
    walked = [not np.array_equal(d.sta_locs, loc) for d, (loc, _) in zip(drops, start)]
    assert walked == [False, True, False, True]
