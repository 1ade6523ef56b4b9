"""The one-call rounding on the solver handle, on the device (mmw_round_attempts, mmw_round_env_attempts, mmw_round_randv).

1. The draw: `round_randv` against `philox_ref.randv` within test_hip_sketch_rng.py's fp64 bar (1e-13 on unit rows, reasoned
   there) and bitwise against `BatchSolver.round_randv` for the same (Z, D', seed, attempt).
2. One call equals the sequential loop: every attempt's slots and count equal the single-attempt call on `round_randv(a)`, integer
   for integer, and the returned (z, pick) is what the loop with stop-at-first over those calls returns; both rules; a factor handed
   in, the resident factor (gX=None) and a spectral block; own and moved states.
3. Against the oracle: every attempt equals `round_cases.reference_attempt` on the device's own directions.
4. Nothing else moves: a twin handle, a repeated call, `round` / `round_env` before and after, the list cache.
5. The sweeps with draws="device" against their steps composed here, and draws="host" against the steps composed from `round_point`.
6. Refusals on a live handle.

The scenarios (tests/helpers/round_attempts_cases.py; test_round_attempts_host.py asserts them on the reference's draws) are
asserted here as properties of the DEVICE's counts -- its normals may differ from NumPy's in the last bits -- so that no comparison
passes vacuously: "the winner is not attempt 0", "no attempt is feasible", "the two rules differ"."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mfma_graphs as mg  # noqa: E402
import online_cases as OC  # noqa: E402
import philox_ref as pr  # noqa: E402
import round_attempts_cases as RA  # noqa: E402
import round_cases as RC  # noqa: E402

from sig_sdp_mmw_amd import _lib, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.graphs import _NOISE_FLOOR_DBM, min_sinr_dec  # noqa: E402

pytestmark = pytest.mark.gpu

ETA = 0.04
BAR64 = 1e-13  # test_hip_sketch_rng.py's fp64 bar
LOOP_FIELDS = ["F_E_THIS", "F_E_ACCU", "F_Y", "F_LVAL", "F_XVAL", "F_XAVG", "F_YAVG", "F_XHALF"]
SEEDS = (0, (1 << 32) + 1, (1 << 64) - 1)
ATTEMPTS = (0, 1, (1 << 31) - 1)
RULES = ("first", "fewest")


def new_env(name, moved=0):
    ap, p0, p1 = OC.positions(name)
    return _lib.DeviceEnv(p1 if moved else p0, ap, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)


def moved_pair(name, Z):
    """(env moved once, handle built on the unmoved state): the handle's own lists are the old state's, the environment's the new."""
    env = new_env(name)
    s = _lib.Solver.from_env(env, max(Z, 2), 2, ETA, dtype=_lib.F64)
    env.move(OC.positions(name)[2])
    return env, s


def singles(s, env, Z, gX, Dp, seed, natt):
    """What the sequential route computes: attempt a is the single-attempt call on the device's own directions of (seed, a)."""
    zs, rems, rvs = [], [], []
    for a in range(natt):
        rv = s.round_randv(Z, Dp, seed, a)
        z, r = s.round(Z, gX, rv[None]) if env is None else s.round_env(env, Z, gX, rv[None])
        zs.append(z[0]); rems.append(int(r[0])); rvs.append(rv)
    return np.stack(zs), rems, rvs


def check_call(s, env, Z, gX_call, gX_single, Dp, seed, natt, want=None):
    """One `round_attempts` / `round_env_attempts` call per rule against the single calls (`want`, or computed here).
    Returns (z_all, rems, directions)."""
    z_want, rem_want, rvs = want if want is not None else singles(s, env, Z, gX_single, Dp, seed, natt)
    for rule in RULES:
        call = (lambda *a, **k: s.round_attempts(*a, **k)) if env is None else (lambda *a, **k: s.round_env_attempts(env, *a, **k))
        z, rem, pick, z_all = call(Z, gX_call, natt, seed, pick=rule, all_attempts=True)
        assert z_all.dtype == np.int32 and z_all.shape == (natt, s.K) and rem.shape == (natt,)
        assert np.array_equal(z_all, z_want) and rem.tolist() == rem_want, (rule, rem.tolist(), rem_want)
        assert rem.tolist() == [int((z_all[a] < 0).sum()) for a in range(natt)]
        assert pick == RA.pick_of(rem_want, rule) and np.array_equal(z, z_want[pick]), (rule, pick)
        if rule == "first":  # literally the loop with stop-at-first over the single calls
            z_loop, a_loop = RA.loop_first(lambda a: (z_want[a], rem_want[a]), natt)
            assert pick == a_loop and np.array_equal(z, z_loop)
        z2, rem2, pick2 = call(Z, gX_call, natt, seed, pick=rule)  # without z_all: the same answer
        assert np.array_equal(z2, z) and np.array_equal(rem2, rem) and pick2 == pick
    return z_want, rem_want, rvs


# ---- 1. the draw ----------------------------------------------------------------------------------------------------------------------
def test_round_randv_meets_the_reference():
    """Z in {2, 3, 9, 70} x D' in {1, 2, 9, 130} (a lone column, one pair, an odd width, a lane's third pass) x every seed x every
    attempt: the full product, 144 blocks."""
    s = _lib.Solver(2, mg.band_state(70, 6, clique=3), 1, ETA, dtype=_lib.F64)
    worst = 0.0
    for Z in (2, 3, 9, 70):
        for Dp in (1, 2, 9, 130):
            for seed in SEEDS:
                for attempt in ATTEMPTS:
                    got, ref = s.round_randv(Z, Dp, seed, attempt), pr.randv(Z, Dp, seed, attempt)
                    assert got.shape == ref.shape and np.all(np.isfinite(got))
                    err = float(np.max(np.abs(got - ref)))
                    worst = max(worst, err)
                    assert err <= BAR64, (Z, Dp, seed, attempt, err)
                    assert float(np.max(np.abs(np.linalg.norm(got, axis=1) - 1.0))) <= 1e-14
    print("[round-attempts] round_randv against philox_ref.randv: worst error %.2e, bar %.0e" % (worst, BAR64))
    # what tells the draws apart really does: another attempt, another low or high word of the seed give other directions
    base = s.round_randv(9, 9, 5, 0)
    for other in (s.round_randv(9, 9, 5, 1), s.round_randv(9, 9, 6, 0), s.round_randv(9, 9, 5 + (1 << 32), 0)):
        assert float(np.max(np.abs(other - base))) > 1e-3
    s.close()


def test_round_randv_is_bitwise_the_batchs():
    """The full product of the shapes again: one batch instance per (Z, D'), its slot count Z and its factor's rank D'."""
    Zs = [Z for Z in (2, 3, 9, 70) for _ in range(4)]
    ranks = [1, 2, 9, 130] * 4
    b = _lib.BatchSolver(Zs, [mg.band_state(140, 6, clique=3)] * 16, 1, ETA, rank_radio=1)
    b.iterate(1, None, [3] * 16)
    b.factor(ranks=ranks)
    s = _lib.Solver(2, mg.band_state(70, 6, clique=3), 1, ETA, dtype=_lib.F32)  # (the draw is fp64 whatever the handle's dtype)
    for i, (Z, Dp) in enumerate(zip(Zs, ranks)):
        assert b.factor_info(i)["rank"] == Dp
        for seed in SEEDS:
            for attempt in ATTEMPTS:
                assert s.round_randv(Z, Dp, seed, attempt).tobytes() == b.round_randv(i, seed, attempt).tobytes(), (Z, Dp, seed, attempt)
    b.close()
    s.close()


# ---- 2. and 3. one call equals the sequential loop, and the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("key", list(RA.SCENARIOS), ids=RA.IDS)
def test_the_scenarios_moved_and_own(key):
    name, Z, seed = key
    gX = RA.factor(name, Z)
    Dp = gX.shape[1]
    env, s = moved_pair(name, Z)
    z_all, rem, rvs = check_call(s, env, Z, gX, gX, Dp, seed, RA.NATT)
    # the scenario's property, on the device's own counts
    if key == ("k75", 9, 0):
        assert rem[0] == 0 and any(rem[1:])  # attempt 0 wins although later attempts are not all feasible
    elif key == ("k75", 9, 3):
        first = RA.pick_of(rem, "first")
        assert first > 0 and 0 in rem[first + 1:]  # the winner is not attempt 0, and not the last feasible one
    elif key == ("k75", 8, 0):
        first = RA.pick_of(rem, "first")
        assert first >= 2 and 0 not in rem[:first]
        short = rem[:first]  # fewer attempts than the first feasible one: nothing is feasible
        assert RA.pick_of(short, "first") == first - 1
        check_call(s, env, Z, gX, gX, Dp, seed, first, want=(z_all[:first], short, rvs[:first]))
    else:
        assert 0 not in rem and RA.pick_of(rem, "first") != RA.pick_of(rem, "fewest")  # none feasible, and the two rules differ
    # round_randv of attempt a is slice a of what the call used: one attempt alone, and a longer call, agree with the six
    check_call(s, env, Z, gX, gX, Dp, seed, 1, want=(z_all[:1], rem[:1], rvs[:1]))
    z10, rem10, _, all10 = s.round_env_attempts(env, Z, gX, 10, seed, all_attempts=True)
    assert np.array_equal(all10[:RA.NATT], z_all) and rem10[:RA.NATT].tolist() == rem
    # the oracle on the device's directions and the moved state copied out
    state = env.state()
    for a in range(RA.NATT):
        want, r, _ = RC.reference_attempt(Z, gX, state, rvs[a])
        assert np.array_equal(z_all[a].astype(np.int64), want) and rem[a] == r, (key, a)
    # the handle's own (unmoved) state through round_attempts: other lists, so another answer somewhere
    own_all, own_rem, _ = check_call(s, None, Z, gX, gX, Dp, seed, RA.NATT)
    assert not np.array_equal(own_all, z_all)
    want, r, _ = RC.reference_attempt(Z, gX, OC.host_state(name, 0), rvs[0])
    assert np.array_equal(own_all[0].astype(np.int64), want) and own_rem[0] == r
    s.close()
    env.close()


def test_k1083_more_than_one_workgroup_picks():
    """K = 1083: five workgroups of k_round_pick, the last one partly filled, users beyond 1024.  Four attempts, two seeds in turn so
    that whatever a call leaves in the winner buffer differs from what the next must return."""
    name = "k1083"
    Z = OC.CASES[name][3]
    gX = OC.factor(name)
    Dp = gX.shape[1]
    env, s = moved_pair(name, Z)
    state = env.state()
    picks = set()
    for seed in (2, 7):
        z_all, rem, rvs = check_call(s, env, Z, gX, gX, Dp, seed, 4)
        picks.add((RA.pick_of(rem, "first"), RA.pick_of(rem, "fewest")))
        assert len({z_all[a][1024:].tobytes() for a in range(4)}) > 1  # the attempts differ beyond user 1024
        for a in range(4):
            want, r, _ = RC.reference_attempt(Z, gX, state, rvs[a])
            assert np.array_equal(z_all[a].astype(np.int64), want) and rem[a] == r, (seed, a)
    check_call(s, None, Z, gX, gX, Dp, 2, 2)
    s.close()
    env.close()


@pytest.mark.parametrize("name", ["k75", "k192"])
def test_the_resident_factor_and_a_spectral_block(name):
    _, _, K, Z = OC.CASES[name]
    env, s = moved_pair(name, Z)
    s.iterate(2, None, seed=3)
    rank = min(K - 1, (Z - 1) * 2)
    df = s.factor(rank, seed=3, resident=True)
    for e in (env, None):
        want = singles(s, e, Z, df, rank, 11, 5)
        assert df._host is None  # read where it lies, by the single calls too
        check_call(s, e, Z, None, None, rank, 11, 5, want=want)  # gX=None: the resident factor
        check_call(s, e, Z, df, None, rank, 11, 5, want=want)    # the DeviceFactor itself
    assert df._host is None
    host = np.array(np.asarray(df))
    check_call(s, env, Z, host, host, rank, 11, 5)  # the factor read back and handed in
    block = s.factor_spectral(Z, resident=True, index_order=True)
    for e in (env, None):
        want = singles(s, e, Z, block, Z, 4, 5)
        check_call(s, e, Z, None, None, Z, 4, 5, want=want)
        check_call(s, e, Z, block, None, Z, 4, 5, want=want)
    assert block._host is None
    s.close()
    env.close()


# ---- 4. nothing else moves ------------------------------------------------------------------------------------------------------------
def loop_fields(s):
    return {f: s.read(getattr(_lib, f)).tobytes() for f in LOOP_FIELDS}


def test_nothing_else_moves():
    name = "k192"
    _, _, K, Z = OC.CASES[name]
    gX, rv = OC.factor(name), OC.randv(name, 0)
    env, still = new_env(name), new_env(name)
    a = _lib.Solver.from_env(env, Z, 6, ETA, dtype=_lib.F64)
    twin = _lib.Solver.from_env(still, Z, 6, ETA, dtype=_lib.F64)  # never calls the new entries
    for s in (a, twin):
        s.iterate(3, None, seed=5)
    env.move(OC.positions(name)[2])
    still.move(OC.positions(name)[2])
    before = (a.round(Z, gX, rv)[0].tobytes(), a.round_env(env, Z, gX, rv)[0].tobytes())
    assert before == (twin.round(Z, gX, rv)[0].tobytes(), twin.round_env(still, Z, gX, rv)[0].tobytes()) and before[0] != before[1]
    first = a.round_env_attempts(env, Z, gX, 6, 3, all_attempts=True)
    again = a.round_env_attempts(env, Z, gX, 6, 3, all_attempts=True)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))  # a second identical call repeats the first
    own = a.round_attempts(Z, gX, 6, 3, pick="fewest")
    a.round_randv(Z, gX.shape[1], 3, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a.round_env_attempts(env, Z, gX, 6, 3, all_attempts=True), first))
    assert all(np.array_equal(x, y) for x, y in zip(a.round_attempts(Z, gX, 6, 3, pick="fewest"), own))
    assert (a.round(Z, gX, rv)[0].tobytes(), a.round_env(env, Z, gX, rv)[0].tobytes()) == before
    assert loop_fields(a) == loop_fields(twin) and a._sizes() == twin._sizes()
    for s in (a, twin):
        s.iterate(3, None, seed=5)
    assert loop_fields(a) == loop_fields(twin)
    fa, ft = a.factor(2 * (Z - 1), seed=1), twin.factor(2 * (Z - 1), seed=1)
    assert fa.tobytes() == ft.tobytes()
    for s in (a, twin):
        s.close()
    env.close()
    still.close()


def test_the_list_cache_follows_the_environment():
    """The second list set is kept per (environment, generation): calls between two moves answer for the state of the last move,
    whichever entry built the lists, and a move is seen by the very next call of either entry.  `round_list_builds` counts the
    builds: one per generation met, however many calls of either entry follow it; refused calls and `round_attempts` build none."""
    name = "k75"
    Z, seed = 9, 3
    gX = RA.factor(name, Z)
    Dp = gX.shape[1]
    ap, p0, p1 = OC.positions(name)
    env = new_env(name)
    s = _lib.Solver.from_env(env, Z, 2, ETA, dtype=_lib.F64)
    rv0 = s.round_randv(Z, Dp, seed, 0)
    s.round_attempts(Z, gX, 3, seed)
    assert s.round_list_builds() == 0  # the handle's own lists are not the second set
    at, builds = {}, 0
    for tag, pos in (("new", p1), ("old", p0), ("new", p1)):
        env.move(pos)
        state = env.state()
        z, rem, pick, z_all = s.round_env_attempts(env, Z, gX, 3, seed, all_attempts=True)  # builds the lists for this generation
        single = s.round_env(env, Z, gX, rv0[None])[0][0]                                   # ... and round_env finds them
        builds += 1
        assert s.round_list_builds() == builds
        assert np.array_equal(single, z_all[0])
        assert np.array_equal(z_all[0].astype(np.int64), RC.reference_attempt(Z, gX, state, rv0)[0])
        assert at.setdefault(tag, z_all.tobytes()) == z_all.tobytes()
        env.move(pos)  # the same positions, a new generation: round_env builds, round_env_attempts finds
        assert np.array_equal(s.round_env(env, Z, gX, rv0[None])[0][0], single)
        assert s.round_env_attempts(env, Z, gX, 3, seed, all_attempts=True)[3].tobytes() == z_all.tobytes()
        s.round_env_attempts(env, Z, gX, 10, seed + 1, pick="fewest")
        with pytest.raises(_lib.MMWError):
            s.round_env_attempts(env, Z, gX, 257, seed)
        builds += 1
        assert s.round_list_builds() == builds
    assert at["new"] != at["old"] and builds == 6
    s.close()
    env.close()


# ---- 5. the sweeps --------------------------------------------------------------------------------------------------------------------
def capture_setup(monkeypatch):
    kept = {}
    real = online._setup

    def setup(*a):
        env, alg, solver, Z, gX = real(*a)
        kept.update(Z=Z, gX=np.array(np.asarray(gX)))
        return env, alg, solver, Z, gX

    monkeypatch.setattr(online, "_setup", setup)
    return kept


def composed_point(s, env, Z, gX, natt, key, pick):
    """A point's rounding composed from single-attempt calls on the device's directions, the rule applied here."""
    z_all, rem, _ = singles(s, env, Z, gX, gX.shape[1], key, natt)
    z = z_all[RA.pick_of(rem, pick)]
    un = z < 0
    z_vec = z.astype(np.float64)
    if un.any():
        z_vec[un] = np.random.default_rng(key).integers(0, Z, int(un.sum()))
    return z_vec, int(un.sum())


@pytest.mark.parametrize("name,n_points,natt,pick", [("k75", 3, 4, "first"), ("k75", 3, 4, "fewest"), ("k1083", 2, 3, "first")])
def test_online_sweep_device_draws_is_its_documented_steps(monkeypatch, name, n_points, natt, pick):
    seed = 3
    kept = capture_setup(monkeypatch)
    np.random.seed(1)
    dtype = _lib.F64 if name == "k75" else _lib.F32
    out = online.online_sweep(OC.drop(name), n_points=n_points, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=dtype, draws="device", pick=pick)
    after = np.random.random_sample()
    Z, gX = kept["Z"], kept["gX"]
    assert out["Z"] == Z
    np.random.seed(1)
    host = online.online_sweep(OC.drop(name), n_points=n_points, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=dtype)
    assert np.random.random_sample() == after and host["Z"] == Z  # the search consumed the global stream alike, the roundings not at all
    drop = OC.drop(name)
    env = online._env(drop, 0)
    s = _lib.Solver.from_env(env, Z, 1, ETA, dtype=_lib.F64)
    for p in range(n_points):
        env.move(drop.sta_locs)
        key = probe_seed(seed, 0, 0x80000 | p)
        z_vec, rem = composed_point(s, env, Z, gX, natt, key, pick)
        _, bler = env.evaluate(z_vec, Z)
        assert np.array_equal(out["z_vec"][p], z_vec) and out["remainder"][p] == rem and out["bler"][p].tobytes() == bler.tobytes(), p
        assert np.all((0 <= z_vec) & (z_vec < Z))
        # draws="host": today's sweep, composed from round_point with the generator the same number seeds
        hz, hrem = online.round_point(s, env, Z, gX, natt, np.random.default_rng(key))
        assert np.array_equal(host["z_vec"][p], hz) and host["remainder"][p] == hrem, p
        drop.step_time(1e6, 3.0, 1e5)
    s.close()
    env.close()


@pytest.mark.parametrize("name,n_points,carry", [("k75", 3, True), ("k1083", 2, False)])
def test_online_resolve_sweep_device_is_its_documented_steps(name, n_points, carry):
    """The re-solving sweep by both routes on one seed: the same Z and iterations, other colourings (the directions differ), and at
    k75 point 0 of either route is `online_sweep`'s point 0 by that route (the same setup, factor and key), which the test above
    composes from single calls.  The later points: `test_online_resolve_sweep_device_later_points`; the host route's own steps:
    test_hip_carry_handle.py, unchanged."""
    seed, natt = 2, 3
    kw = dict(n_points=n_points, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=_lib.F64 if name == "k75" else _lib.F32, resolve_nit=10, carry=carry)
    np.random.seed(1)
    dev = online.online_resolve_sweep_device(OC.drop(name), **kw)
    np.random.seed(1)
    host = online.online_resolve_sweep(OC.drop(name), **kw)
    Z = dev["Z"]
    assert host["Z"] == Z and dev["iters"] == host["iters"] == [30] + [10] * (n_points - 1)
    assert np.all((0 <= dev["z_vec"]) & (dev["z_vec"] < Z)) and np.all(dev["z_vec"] == np.floor(dev["z_vec"])) and np.all(np.isfinite(dev["bler"]))
    assert not np.array_equal(dev["z_vec"], host["z_vec"])  # other directions: the route did change (and went back for the host call)
    if name != "k75":
        return
    # point 0 of both sweeps is online_sweep's point 0 (the same setup, the same key)
    np.random.seed(1)
    one = online.online_sweep(OC.drop(name), n_points=1, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=kw["dtype"], draws="device")
    assert np.array_equal(one["z_vec"][0], dev["z_vec"][0]) and one["bler"][0].tobytes() == dev["bler"][0].tobytes()
    np.random.seed(1)
    one = online.online_sweep(OC.drop(name), n_points=1, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=kw["dtype"])
    assert np.array_equal(one["z_vec"][0], host["z_vec"][0]) and one["bler"][0].tobytes() == host["bler"][0].tobytes()


@pytest.mark.parametrize("name,n_points,natt,dtype,carry,pick", [("k75", 3, 4, _lib.F64, True, "fewest"), ("k1083", 2, 3, _lib.F32, False, "first")])
def test_online_resolve_sweep_device_later_points(monkeypatch, name, n_points, natt, dtype, carry, pick):
    """The later points of the re-solving sweep: `round_point_device` is handed the point's new handle, its resident factor and the
    key probe_seed(seed, 0, 0x80000 | p), and what it returns is what the sweep stores -- recorded by wrapping it, then composed from
    single calls on that very handle while it is still open."""
    seed = 2
    seen = []
    real = online.round_point_device

    def wrapped(solver, env, Z, gX, nattempt, key, pick="first"):
        got = real(solver, env, Z, gX, nattempt, key, pick)
        host_factor = np.array(np.asarray(gX)) if gX is not None else None
        builds = solver.round_list_builds()  # after the one call of the point, before the single calls composed here
        seen.append((key, pick, nattempt, got, composed_point(solver, env, Z, host_factor, nattempt, key, pick), solver, builds))
        assert solver.round_list_builds() == builds  # the single calls found the lists of this generation
        return got

    monkeypatch.setattr(online, "round_point_device", wrapped)
    np.random.seed(1)
    out = online.online_resolve_sweep_device(OC.drop(name), n_points=n_points, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=dtype,
                                             resolve_nit=10, carry=carry, pick=pick)
    assert [e[0] for e in seen] == [probe_seed(seed, 0, 0x80000 | p) for p in range(n_points)] and all(e[1] == pick and e[2] == natt for e in seen)
    assert len({id(e[5]) for e in seen}) == n_points and all(e[6] == 1 for e in seen[1:])  # a new handle per point, its lists built once
    for p, (_, _, _, got, want, _, _) in enumerate(seen):
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], p
        assert np.array_equal(out["z_vec"][p], got[0]) and out["remainder"][p] == got[1]


# ---- 6. refusals on a live handle -----------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle():
    import ctypes as C
    L = _lib.lib()
    name = "k75"
    _, _, K, Z = OC.CASES[name]
    gX, rv = OC.factor(name), OC.randv(name, 0)
    env, other = new_env(name), new_env("k192")
    s = _lib.Solver.from_env(env, Z, 3, ETA, dtype=_lib.F64)
    s.iterate(3, None, seed=5)
    fields, rounded = loop_fields(s), s.round(Z, gX, rv)[0].tobytes()
    answer = s.round_env_attempts(env, Z, gX, 3, 1, all_attempts=True)

    def refused(fn, who, status, *args):
        z, rem, pick = np.full(K, 7, dtype=np.int32), np.full(4, 7, dtype=np.int32), C.c_int32(7)
        rc = fn(*args, _lib._pi(z), _lib._pi(rem), C.byref(pick), None)
        msg = L.mmw_last_error().decode()
        assert rc == status and msg.startswith(who + ":") and np.all(z == 7) and np.all(rem == 7) and pick.value == 7, (rc, msg)
        return msg

    g = _lib._pd(_lib._f64(gX))
    Dp, u64 = gX.shape[1], C.c_uint64(1)
    assert "K = 192" in refused(L.mmw_round_env_attempts, "mmw_round_env_attempts", -1, s._h, other._h, Z, Dp, g, 3, u64, 0)
    assert "null environment" in refused(L.mmw_round_env_attempts, "mmw_round_env_attempts", -1, s._h, None, Z, Dp, g, 3, u64, 0)
    assert "LDS" in refused(L.mmw_round_env_attempts, "mmw_round_env_attempts", -1, s._h, env._h, 4801, Dp, g, 3, u64, 0)
    assert "nattempt = 257" in refused(L.mmw_round_attempts, "mmw_round_attempts", -1, s._h, Z, Dp, g, 257, u64, 0)
    assert "pick_rule" in refused(L.mmw_round_attempts, "mmw_round_attempts", -1, s._h, Z, Dp, g, 3, u64, 2)
    # gX = NULL with no resident factor (none computed yet; then one of another width)
    for who, fn, head in (("mmw_round_attempts", L.mmw_round_attempts, (s._h,)), ("mmw_round_env_attempts", L.mmw_round_env_attempts, (s._h, env._h))):
        assert "holds no factor" in refused(fn, who, -3, *head, Z, Dp, None, 3, u64, 0)
    with pytest.raises(_lib.MMWError, match="holds no factor"):
        s.round_attempts(Z, None, 3, 1)
    s.factor(4, seed=1, resident=True)
    assert "holds no factor" in refused(L.mmw_round_attempts, "mmw_round_attempts", -3, s._h, Z, Dp, None, 3, u64, 0)
    if _lib.device_count() > 1:  # an environment on another device needs a second device to exist
        ap, p0, _ = OC.positions(name)
        far = _lib.DeviceEnv(p0, ap, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=1)
        assert "device 1" in refused(L.mmw_round_env_attempts, "mmw_round_env_attempts", -1, s._h, far._h, Z, Dp, g, 3, u64, 0)
        far.close()
    with pytest.raises(_lib.MMWError, match="mmw_round_env_attempts"):
        s.round_env_attempts(other, Z, gX, 3, 1)
    assert loop_fields(s) == fields and s.round(Z, gX, rv)[0].tobytes() == rounded
    assert all(np.array_equal(x, y) for x, y in zip(s.round_env_attempts(env, Z, gX, 3, 1, all_attempts=True), answer))
    s.close()
    env.close()
    other.close()
