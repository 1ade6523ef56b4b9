"""GPU: MAX_RAND with its draws on the device (mmw_gm_rand, mmw_batch_gm_rand, mmw_batch_env_gm_rand).

Two comparators, neither the kernels under test: the device = -1 handle (plain C++, the draw through the host form of the same
functions) and the NumPy restatement of the draw fed to the reference's own greedy (`gm_rand_cases.reference`: `gm_restate.max_rand`
on the order and preference NumPy forms).  Draws are compared bit for bit, slots and counts as integers; every colouring is checked
slot by slot (`gm_restate.check_slots`).  Shapes: the one-AP pair, a wave and one user more, several blocks, env300 on either side of
its feasibility edge, an ER state, Z = 1, the widest Z; in the batch six instances of K = 2 ... 1024 in one launch.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import gm_rand_cases as GR  # noqa: E402
import gm_restate as R  # noqa: E402
import online_cases as OC  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch, gm, online  # noqa: E402
from sig_sdp_mmw_amd.graphs import _NOISE_FLOOR_DBM, min_sinr_dec  # noqa: E402

pytestmark = pytest.mark.gpu

ARG = -1
SEED = GR.DRAW_SEEDS[1]


@pytest.fixture(scope="module")
def pair():
    hs = {}

    def get(name):
        if name not in hs:
            hs[name] = (_lib.GreedyHandle(GR.state(name), device=0), _lib.GreedyHandle(GR.state(name), device=-1))
        return hs[name]
    yield get
    for d, h in hs.values():
        d.close()
        h.close()


@pytest.mark.parametrize("K,Z", GR.DRAW_SHAPES + ((2, 4800),))
def test_device_draw_is_the_host_form_and_the_restatement_bit_for_bit(pair, K, Z):
    dev, host = pair(GR.STATE_OF_K[K])
    for seed in GR.DRAW_SEEDS:
        for a in GR.DRAW_ATTEMPTS:
            pv, key = dev.rand_draw(Z, seed, a)
            hv, hk = host.rand_draw(Z, seed, a)
            rv, rk = GR.draw(K, Z, seed, a)
            diff = int(np.sum(pv != hv)) + int(np.sum(key != hk))
            print("[gm-rand] K %d Z %d seed %#x attempt %d: %d values differ from the host form, largest difference %.2e"
                  % (K, Z, seed, a, diff, max(np.max(np.abs(pv - hv)), np.max(np.abs(key - hk)))))
            assert pv.tobytes() == hv.tobytes() and key.tobytes() == hk.tobytes(), (seed, a)
            assert pv.tobytes() == rv.tobytes() and key.tobytes() == rk.tobytes(), (seed, a)


# env300's feasibility edge by the restatement: no attempt succeeds at 10 slots, the third alone at 11, all at 13
SLOT_CASES = [("one_ap", 1), ("one_ap", 2), ("er64", 2), ("er65", 9), ("j8", 1), ("j8", 7), ("j8", 14), ("env300", 10), ("env300", 11), ("env300", 13),
              ("er120", 6), ("j15", 9)]


@pytest.mark.parametrize("name,Z", SLOT_CASES)
def test_device_slots_are_the_host_form_and_the_reference_greedy(pair, name, Z):
    dev, host = pair(name)
    st, natt = GR.state(name), 3
    want, rem_want = GR.reference(Z, st, SEED, natt)
    for rule, pick in ((0, "first"), (1, "fewest")):
        z, rem, got = dev.rand(Z, natt, SEED, pick)
        zh, remh, goth = host.rand(Z, natt, SEED, pick)
        assert np.array_equal(z, zh) and rem.tolist() == remh.tolist() and got == goth, (rule, rem.tolist(), remh.tolist())
        assert rem.tolist() == rem_want and got == GR.pick_of(rem_want, rule) and np.array_equal(z, want[got]), (rule, rem.tolist(), rem_want)
        assert int(np.sum(z < 0)) == rem[got]
        R.check_slots(st, z, z >= 0)
    again = dev.rand(Z, natt, SEED, "fewest")
    assert np.array_equal(again[0], z) and again[1].tolist() == rem.tolist()  # the handle's buffers are reused, the answer is not


def test_the_feasibility_edge_of_env300_is_on_both_sides():
    st = GR.state("env300")
    at11 = GR.reference(11, st, SEED, 3)[1]
    assert min(GR.reference(10, st, SEED, 3)[1]) > 0 and at11[0] > 0 and at11[2] == 0 and max(GR.reference(13, st, SEED, 3)[1]) == 0


def test_widest_slot_count_and_the_one_beyond(pair):
    dev, host = pair("one_ap")
    z, rem, got = dev.rand(4800, 2, 9)
    zh, remh, _ = host.rand(4800, 2, 9)
    assert np.array_equal(z, zh) and rem.tolist() == remh.tolist() == [0, 0] and got == 0 and np.all((z >= 0) & (z < 4800))
    zz, rr, gg = np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int32), C.c_int32(-7)
    assert _lib.lib().mmw_gm_rand(dev._h, 4801, 2, 9, 0, _lib._pi(zz), _lib._pi(rr), C.byref(gg)) == ARG
    assert "Z = 4801" in _lib.lib().mmw_last_error().decode() and np.all(zz == -7) and np.all(rr == -7) and gg.value == -7


def test_handle_from_a_moved_environment_is_the_host_state_handle():
    name = "k192"
    ap, p0, p1 = OC.positions(name)
    env = _lib.DeviceEnv(p0, ap, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)
    env.move(p1)
    st = env.state()
    g, h = _lib.GreedyHandle.from_env(env), _lib.GreedyHandle(st, device=0)
    try:
        for Z in (5, OC.CASES[name][3] + 3):
            a, b = g.rand(Z, 3, SEED, "fewest"), h.rand(Z, 3, SEED, "fewest")
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
            want, rem_want = GR.reference(Z, st, SEED, 3)
            assert a[1].tolist() == rem_want and np.array_equal(a[0], want[a[2]])
            da, db = g.rand_draw(Z, SEED, 1), h.rand_draw(Z, SEED, 1)
            assert da[0].tobytes() == db[0].tobytes() and da[1].tobytes() == db[1].tobytes()
        # gm.MAX_RAND on the device-resident state takes the same route
        np.random.seed(3)
        a = gm.MAX_RAND.run(12, env.device_state(), draws="device")
        np.random.seed(3)
        b = gm.MAX_RAND.run(12, st, draws="device")
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    finally:
        g.close()
        h.close()
        env.close()


# ---- the batch -----------------------------------------------------------------------------------------------------------------------
BATCH_KS = (2, 64, 65, 192, 675, 1024)
BATCH_Z = [2, 4, 9, 7, 10, 12]
BATCH_SEEDS = [21, 22, SEED, 24, 25, 26]


@pytest.fixture(scope="module")
def db():
    names = [GR.STATE_OF_K[k] for k in BATCH_KS]
    b = _lib.BatchSolver([4] * len(names), [GR.state(n) for n in names], 1, 0.04, device=0)
    assert [s["K"] for s in b.sizes] == list(BATCH_KS)
    yield b, names
    b.close()


@pytest.fixture(scope="module")
def batch_all(db):
    b, _ = db
    return b.gm_rand(BATCH_Z, BATCH_SEEDS, 3, stop_at_first=False)


def test_batch_instance_is_the_handle(db, batch_all, pair):
    b, names = db
    z, rem, used = batch_all
    assert used.tolist() == [3] * b.B
    for i, name in enumerate(names):
        dev, host = pair(name)
        for rule, pick in ((0, "first"), (1, "fewest")):
            zh, remh, got = dev.rand(BATCH_Z[i], 3, BATCH_SEEDS[i], pick)
            assert remh.tolist() == rem[i].tolist() and zh.tobytes() == np.ascontiguousarray(z[i][got]).tobytes(), (name, rule)
        zc, remc, gotc = host.rand(BATCH_Z[i], 3, BATCH_SEEDS[i])
        assert remc.tolist() == rem[i].tolist() and np.array_equal(zc, z[i][gotc]), name
        for a in range(3):
            assert int(np.sum(z[i][a] < 0)) == rem[i][a]
            R.check_slots(GR.state(name), z[i][a], z[i][a] >= 0)
    want, rem_want = GR.reference(BATCH_Z[3], GR.state(names[3]), BATCH_SEEDS[3], 3)  # and one of them against the reference's greedy
    assert np.array_equal(z[3], want) and rem[3].tolist() == rem_want


def test_batch_under_take_alone_and_with_stop_at_first(db, batch_all):
    b, names = db
    z, rem, used = batch_all
    take = [True, False, True, False, False, True]
    zt, remt, usedt = b.gm_rand(BATCH_Z, BATCH_SEEDS, 3, take=take, stop_at_first=False)
    for i in range(b.B):
        if take[i]:
            assert zt[i].tobytes() == z[i].tobytes() and remt[i].tolist() == rem[i].tolist() and usedt[i] == 3
        else:
            assert zt[i] is None and remt[i].tolist() == [-1] * 3 and usedt[i] == 0
    one = _lib.BatchSolver([4], [GR.state(names[2])], 1, 0.04, device=0)
    z1, rem1, _ = one.gm_rand([BATCH_Z[2]], [BATCH_SEEDS[2]], 3, stop_at_first=False)
    one.close()
    assert z1[0].tobytes() == z[2].tobytes() and rem1[0].tolist() == rem[2].tolist()
    zs, rems, useds = b.gm_rand(BATCH_Z, BATCH_SEEDS, 3, stop_at_first=True)
    for i in range(b.B):
        full = rem[i].tolist()
        u = full.index(0) + 1 if 0 in full else 3
        assert useds[i] == u and rems[i].tolist() == full[:u] + [-1] * (3 - u), names[i]
        assert np.array_equal(zs[i][:u], z[i][:u]) and np.all(zs[i][u:] == -2)
    Zs = list(BATCH_Z)
    Zs[1] = 0  # no slot count: the instance is left out
    zo, remo, usedo = b.gm_rand(Zs, BATCH_SEEDS, 3, stop_at_first=False)
    assert zo[1] is None and usedo[1] == 0 and all(zo[i].tobytes() == z[i].tobytes() for i in range(b.B) if i != 1)


def test_batch_leaves_the_resident_factors_and_their_rounding_alone(db):
    b, _ = db
    seeds = [31, 32, 33, 34, 35, 36]
    b.factor_random(seeds)
    before = b.round(2, seeds, stop_at_first=False)
    fac = [b.read_factor(i).tobytes() for i in range(b.B)]
    b.gm_rand(BATCH_Z, BATCH_SEEDS, 2)
    after = b.round(2, seeds, stop_at_first=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0])) and before[1].tobytes() == after[1].tobytes()
    assert fac == [b.read_factor(i).tobytes() for i in range(b.B)]


def test_batch_limits_are_refused_by_name(db):
    b, _ = db
    z, rem, used = np.full(8, -7, dtype=np.int32), np.full(6, -7, dtype=np.int32), np.full(6, -7, dtype=np.int32)
    sd = _lib._u64(1, 6)
    take = _lib._i32([1, 0, 0, 0, 0, 0])
    rc = _lib.lib().mmw_batch_gm_rand(b._h, _lib._pi(take), _lib._pi(_lib._i32([1025] * 6)), 1, 0, _lib._pu(sd), _lib._pi(z), _lib._pi(rem), _lib._pi(used))
    err = _lib.lib().mmw_last_error().decode()
    assert rc == ARG and "instance 0" in err and "Z = 1025" in err and np.all(z == -7) and np.all(rem == -7) and np.all(used == -7)
    over = _lib.BatchSolver([4], [GR.state("er1025")], 1, 0.04, device=0)
    with pytest.raises(_lib.MMWError, match="instance 0: K = 1025 exceeds the limit 1024"):
        over.gm_rand([4], [1])
    over.close()


def test_batch_env_serves_the_state_of_the_last_move(pair):
    names = ["k75", "k192"]
    pos = [OC.positions(n) for n in names]
    env = _lib.BatchEnv([p[0] for p in pos], [p[1].shape[0] for p in pos], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)
    try:
        with pytest.raises(_lib.MMWError, match="no positions yet"):
            env.gm_rand([5, 5], [1, 2])
        env.move([p[1] for p in pos])
        env.move([p[2] for p in pos])
        Zs, seeds = [OC.CASES[n][3] + 2 for n in names], [41, SEED]
        z, rem, used = env.gm_rand(Zs, seeds, 3, stop_at_first=False)
        for i in range(2):
            st = env.state(i)
            h = _lib.GreedyHandle(st, device=0)
            zh, remh, got = h.rand(Zs[i], 3, seeds[i])
            h.close()
            assert remh.tolist() == rem[i].tolist() and zh.tobytes() == np.ascontiguousarray(z[i][got]).tobytes(), names[i]
            want, rem_want = GR.reference(Zs[i], st, seeds[i], 3)
            assert np.array_equal(z[i], want) and rem[i].tolist() == rem_want
            R.check_slots(st, z[i][0], z[i][0] >= 0)
        zt, _, usedt = env.gm_rand(Zs, seeds, 3, take=[False, True], stop_at_first=False)
        assert zt[0] is None and usedt.tolist() == [0, 3] and zt[1].tobytes() == z[1].tobytes()
    finally:
        env.close()


def test_mrand_in_the_sweeps():
    """`baselines_many` on a (batch, environment) pair, `compare_many` and `online.compare` with "mrand" named: the colourings are
    valid for the states they were made on, and `online.compare`'s is `GreedyHandle.rand`'s for its key."""
    geo = [(OC.positions(n)[1], OC.positions(n)[0]) for n in ("k75",)]
    out = batch.compare_many(geo, nit=20, methods=batch.METHODS + ("mrand",))
    assert set(out[0]["bler"]) == {"mmw", "rand", "mgain", "masso", "mrand"} and out[0]["bler"]["mrand"].shape == (75,)
    res = online.compare(geo[0], nit=20, methods=("mgain", "mrand"))
    env = _lib.DeviceEnv(geo[0][0], geo[0][1], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)  # `online._env`'s, for its state
    Z, st = res["Z"], env.state()
    env.close()
    key = batch.probe_seed(0, 0, 0x40000 | 4)
    want, rem_want = GR.reference(Z, st, key, 1)
    z = res["z_vec"]["mrand"]
    assert res["remainder"]["mrand"] == rem_want[0] and np.array_equal(z[want[0] >= 0], want[0][want[0] >= 0])
    R.check_slots(st, z, want[0] >= 0)
