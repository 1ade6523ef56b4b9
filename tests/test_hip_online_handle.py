"""The online sweeps on the solver handle, on the device: mmw_env_move against a fresh mmw_env_create and against the host
generator, mmw_round_env against the oracle's `rounding_one_attempt` on the moved state, mmw_gm_create_from_env against
mmw_gm_create on the state copied out, and `online.online_sweep` / `online_greedy_sweep` against the same steps composed here.
Cases (tests/helpers/online_cases.py): three `graphs.mobile_drop`s at rho = 75e-4 (K = 75, 192 and 1083 -- the last over the
batch epilogue's 1024), each moved once by `step_time(1e6, 3.0, 1e5)`.  Integers and bit patterns must be equal; only the
comparison with the host generator allows 1e-12 relative on values (device pow / log10 against NumPy's)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import online_cases as OC  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch, gm, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.graphs import _NOISE_FLOOR_DBM, min_sinr_dec  # noqa: E402

pytestmark = pytest.mark.gpu

LOOP_FIELDS = ["F_E_THIS", "F_E_ACCU", "F_Y", "F_LVAL", "F_XVAL", "F_XAVG", "F_YAVG", "F_XHALF"]
ETA = 0.04


def new_env(name, moved=0):
    ap, p0, p1 = OC.positions(name)
    return _lib.DeviceEnv(p1 if moved else p0, ap, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)


def snapshot(env, name):
    """Everything an environment answers, as bytes: sizes, the seven arrays, the bounds, the scores of one fixed colouring."""
    Z = OC.CASES[name][3]
    S, Q, h = env.state()
    z = (np.arange(env.K) % Z).astype(np.float64)
    z[::11] = Z + 1  # (some users outside every slot)
    sinr, bler = env.evaluate(z, Z)
    sz = (env.K, env.A, env.nnzS, env.nnzQ)
    assert (S.nnz, Q.nnz) == sz[2:]
    return (sz, env.bounds()) + tuple(np.ascontiguousarray(a).tobytes() for a in (S.indptr, S.indices, S.data, Q.indptr, Q.indices, Q.data, h, sinr, bler))


def same_state(a, b, rtol):
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
        np.testing.assert_allclose(x.data, y.data, rtol=rtol, atol=0)
    np.testing.assert_allclose(a[2], b[2], rtol=rtol, atol=0)


@pytest.mark.parametrize("name", OC.NAMES)
def test_move_equals_create(name):
    ap, p0, p1 = OC.positions(name)
    env = new_env(name)
    first = snapshot(env, name)
    fresh = new_env(name, 1)
    want = snapshot(fresh, name)
    fresh.close()
    assert want != first and want[0][2] != first[0][2]  # nnz(S) rises in one case and falls in the others
    env.move(p1)
    assert snapshot(env, name) == want
    env.move(p0)  # there and back again: the buffers grow and shrink in both directions over the cases
    assert snapshot(env, name) == first
    env.move(p1)
    assert snapshot(env, name) == want and env.generation == 3
    env.close()


@pytest.mark.parametrize("name", OC.NAMES)
def test_move_against_the_host_generator(name):
    # the precondition of a pattern comparison across two math libraries: no receive power within 1e-9 relative of the cut
    assert OC.cut_margin(name, 0) > 1e-9 and OC.cut_margin(name, 1) > 1e-9
    env = new_env(name)
    same_state(env.state(), OC.host_state(name, 0), 1e-12)
    env.move(OC.positions(name)[2])
    same_state(env.state(), OC.host_state(name, 1), 1e-12)
    env.close()


def to_slots(z):
    return np.asarray(z, dtype=np.int64)


@pytest.mark.parametrize("name", OC.NAMES)
def test_round_env_is_exact(name):
    _, _, K, Z = OC.CASES[name]
    gX = OC.factor(name)
    env = new_env(name)
    s = _lib.Solver.from_env(env, Z, 2, ETA, dtype=_lib.F64)
    old_state = env.state()
    # an environment that has not moved: bitwise mmw_round
    for draw in (0, 1):
        z0, r0 = s.round(Z, gX, OC.randv(name, draw))
        z1, r1 = s.round_env(env, Z, gX, OC.randv(name, draw))
        assert z0.tobytes() == z1.tobytes() and r0.tobytes() == r1.tobytes()
    env.move(OC.positions(name)[2])
    st = env.state()  # the device's own moved state, copied out
    differ = 0
    for draw in (0, 1):
        want, rem = OC.oracle_slots(orc, name, st, draw)
        differ += int(np.sum(want != OC.oracle_slots(orc, name, old_state, draw)[0]))
        z, r = s.round_env(env, Z, gX, OC.randv(name, draw))
        assert np.array_equal(to_slots(z[0]), want) and int(r[0]) == rem, (name, draw)
        zold, _ = s.round(Z, gX, OC.randv(name, draw))  # the handle's own lists still stand for the old state
        assert np.array_equal(to_slots(zold[0]), OC.oracle_slots(orc, name, old_state, draw)[0])
    assert differ >= 1  # a round_env that ignored the environment could not have passed
    # both draws in one call
    zb, rb = s.round_env(env, Z, gX, np.stack([OC.randv(name, 0), OC.randv(name, 1)]))
    assert all(np.array_equal(to_slots(zb[d]), OC.oracle_slots(orc, name, st, d)[0]) for d in (0, 1))
    # the resident factor: the same call given the factor read back
    s.iterate(2, None, seed=3)
    rank = min(K - 1, (Z - 1) * 2)
    df = s.factor(rank, seed=3, resident=True)
    rv = np.random.default_rng(5).standard_normal((Z, rank))
    rv /= np.linalg.norm(rv, axis=1, keepdims=True)
    za, ra = s.round_env(env, Z, df, rv)
    assert df._host is None  # read where it lies
    host = np.array(np.asarray(df))
    zh, rh = s.round_env(env, Z, host, rv)
    assert za.tobytes() == zh.tobytes() and ra.tobytes() == rh.tobytes()
    want, _, rem, un = orc.rounding_one_attempt(Z, host, st, rv, randint=lambda Z_, size: np.zeros(size))
    if np.unique(np.linalg.norm(host, axis=1)).size == K:  # (distinct norms: the visiting order is the oracle's)
        assert np.array_equal(to_slots(za[0]), np.where(un, -1, want).astype(np.int64)) and int(ra[0]) == rem
    s.close()
    env.close()


def loop_fields(s):
    return {f: s.read(getattr(_lib, f)).tobytes() for f in LOOP_FIELDS}


@pytest.mark.parametrize("name", OC.NAMES)
def test_nothing_else_moves(name):
    _, _, K, Z = OC.CASES[name]
    gX, rv = OC.factor(name), OC.randv(name, 0)
    env, still = new_env(name), new_env(name)
    a = _lib.Solver.from_env(env, Z, 6, ETA, dtype=_lib.F64)
    twin = _lib.Solver.from_env(still, Z, 6, ETA, dtype=_lib.F64)  # never sees a move or a round_env
    for s in (a, twin):
        s.iterate(3, None, seed=5)
    assert loop_fields(a) == loop_fields(twin)
    env.move(OC.positions(name)[2])
    assert loop_fields(a) == loop_fields(twin) and a.round(Z, gX, rv)[0].tobytes() == twin.round(Z, gX, rv)[0].tobytes()
    moved = a.round_env(env, Z, gX, rv)[0]
    assert moved.tobytes() != twin.round(Z, gX, rv)[0].tobytes()
    assert loop_fields(a) == loop_fields(twin) and a.round(Z, gX, rv)[0].tobytes() == twin.round(Z, gX, rv)[0].tobytes()
    for s in (a, twin):
        s.iterate(3, None, seed=5)
    assert loop_fields(a) == loop_fields(twin) and a._sizes() == twin._sizes()
    fa, ft = a.factor(2 * (Z - 1), seed=1), twin.factor(2 * (Z - 1), seed=1)
    assert fa.tobytes() == ft.tobytes()
    for s in (a, twin):
        s.close()
    env.close()
    still.close()


def greedy_answers(g, name, state):
    """Everything a greedy handle answers for a case: sizes, keys, runs, a pass, an assignment."""
    _, _, K, Z = OC.CASES[name]
    keys = (gm._gain_key(state), gm._asso_key(state))
    out = [g.sizes(), g.key(0).tobytes(), g.key(1).tobytes()]
    for key in keys:
        for bound, natt in ((K, 1), (Z, 1), (Z, 3)):  # Z = -1 with not_Z_bound is K slots (gm.py:22-23)
            z, zz, rem = g.run(key, bound, natt)
            out.append((z.tobytes(), zz, rem))
        out.append(g.pass_(np.argsort(-key, kind="stable"), 2).tobytes())
    rng = np.random.default_rng(K)
    pref = np.ascontiguousarray(np.argsort(-rng.standard_normal((Z, K)), axis=0).T)
    z, rem = g.assign(rng.permutation(K), pref)
    out.append((z.tobytes(), rem))
    return out, keys


@pytest.mark.parametrize("name", OC.NAMES)
def test_greedy_handle_from_env(name):
    env = new_env(name)
    answers = []
    for step in (0, 1):
        if step:
            env.move(OC.positions(name)[2])
        state = env.state()
        g, h = _lib.GreedyHandle.from_env(env), _lib.GreedyHandle(state)
        got, keys = greedy_answers(g, name, state)
        want, _ = greedy_answers(h, name, state)
        assert got == want, (name, step)
        assert got[1] == keys[0].tobytes() and got[2] == keys[1].tobytes()  # the device keys are the scipy expressions, bitwise
        assert g.groups == h.groups >= 1
        h.close()
        answers.append((g, got, state))
    assert answers[0][1] != answers[1][1]
    g0, got0, state0 = answers[0]
    assert greedy_answers(g0, name, state0)[0] == got0  # built before the move: it keeps answering for the old state
    for g, _, _ in answers:
        g.close()
    env.close()


def test_gm_classes_take_the_moved_state_without_a_host_copy(monkeypatch):
    name = "k192"
    env = new_env(name)
    env.move(OC.positions(name)[2])
    host = env.state()
    ds = env.device_state()

    def no_host(self):
        raise AssertionError("state copied to the host")

    want = []
    for cls in (gm.MAX_GAIN, gm.MAX_ASSO):
        for order in ("reference", "stable"):
            np.random.seed(2)
            want.append(cls.run(-1, host, not_Z_bound=True, order=order))
    monkeypatch.setattr(_lib.DeviceState, "host", no_host)
    monkeypatch.setattr(_lib.DeviceEnv, "state", no_host)
    got = []
    for cls in (gm.MAX_GAIN, gm.MAX_ASSO):
        for order in ("reference", "stable"):
            np.random.seed(2)
            got.append(cls.run(-1, ds, not_Z_bound=True, order=order))
    for a, b in zip(got, want):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    env.move(OC.positions(name)[1])
    with pytest.raises(_lib.MMWError, match="generation"):
        gm.MAX_GAIN.run(-1, ds, not_Z_bound=True)
    env.close()


def test_a_stale_device_state_of_a_real_environment_raises():
    from sig_sdp_mmw_amd.sdp_solver import sdp_solver
    name = "k75"
    env = new_env(name)
    old = env.device_state()
    alg = sdp_solver()
    alg._dtype_code = _lib.F64
    s = alg._device_solver(4, old)
    assert s.K == 75 and alg._same_state(old)
    env.move(OC.positions(name)[2])
    new = env.device_state()
    assert new is not old and not alg._same_state(new)
    for use in (old.host, lambda: old.env.solver(4, 1, 0.1), lambda: alg._device_solver(4, old)):
        with pytest.raises(_lib.MMWError, match="generation 0"):
            use()
    same_state(new.host(), OC.host_state(name, 1), 1e-12)
    alg.close()
    env.close()


def capture_setup(monkeypatch):
    """Let `online._setup` run as it is and keep what it found: Z and a host copy of the factor (the resident one stays resident)."""
    kept = {}
    real = online._setup

    def setup(*a):
        env, alg, solver, Z, gX = real(*a)
        kept.update(Z=Z, gX=np.array(np.asarray(gX)))
        return env, alg, solver, Z, gX

    monkeypatch.setattr(online, "_setup", setup)
    return kept


def test_online_sweep_is_its_documented_steps(monkeypatch):
    name, seed, natt, n_points = "k75", 3, 4, 3
    kept = capture_setup(monkeypatch)
    np.random.seed(1)
    timings = []
    out = online.online_sweep(OC.drop(name), n_points=n_points, mob_spd_meter_s=3.0, nit=30, seed=seed, nattempt=natt, dtype=_lib.F64, timings=timings)
    Z, gX = kept["Z"], kept["gX"]
    assert out["Z"] == Z and gX.shape == (75, min(74, (Z - 1) * 2)) and len(timings) == n_points
    # the same points composed here: move / round_env / evaluate on a handle of our own, the factor handed in
    drop = OC.drop(name)
    env = online._env(drop, 0)
    s = _lib.Solver.from_env(env, Z, 1, ETA, dtype=_lib.F64)
    moved = 0
    for p in range(n_points):
        before = env.state()[0]
        env.move(drop.sta_locs)
        moved += int(before.nnz != env.state()[0].nnz or not np.array_equal(before.data, env.state()[0].data))
        rng = np.random.default_rng(probe_seed(seed, 0, 0x80000 | p))
        for _ in range(natt):
            rv = rng.standard_normal((Z, gX.shape[1]))
            rv /= np.linalg.norm(rv, axis=1, keepdims=True)
            z, rem = s.round_env(env, Z, gX, rv[None])
            if rem[0] == 0:
                break
        z_vec = z[0].astype(np.float64)
        un = z[0] < 0
        if un.any():
            z_vec[un] = rng.integers(0, Z, int(un.sum()))
        _, bler = env.evaluate(z_vec, Z)
        assert np.array_equal(out["z_vec"][p], z_vec) and out["remainder"][p] == int(un.sum()) and out["bler"][p].tobytes() == bler.tobytes(), p
        assert np.all((0 <= z_vec) & (z_vec < Z))
        drop.step_time(1e6, 3.0, 1e5)
    assert moved == n_points - 1  # the stations did walk between the points
    s.close()
    env.close()


def test_online_greedy_sweep_is_its_documented_steps():
    name, seed, n_points = "k75", 2, 3
    out = online.online_greedy_sweep(OC.drop(name), n_points=n_points, mob_spd_meter_s=3.0, seed=seed)
    drop = OC.drop(name)
    env = online._env(drop, 0)
    state = env.state()
    g = _lib.GreedyHandle(state)
    slot, ZZ, rem = g.run(gm._gain_key(state), drop.K, 1)
    g.close()
    zv, rem = batch._fill(slot, rem, ZZ, probe_seed(seed, 0, 0x40000 | 1))
    assert out["Z"] == ZZ and np.all(out["remainder"] == rem) and out["z_vec"].shape == out["bler"].shape == (n_points, drop.K)
    for p in range(n_points):
        env.move(drop.sta_locs)
        _, bler = env.evaluate(zv, ZZ)
        assert np.array_equal(out["z_vec"][p], zv) and out["bler"][p].tobytes() == bler.tobytes(), p
        drop.step_time(1e6, 3.0, 1e4)
    env.close()
    assert not np.array_equal(out["bler"][0], out["bler"][n_points - 1])
    # what the batch computes for the same drop (K below its limit): the same colouring and scores
    many = batch.online_greedy_many([OC.drop(name)], n_points=n_points, mob_spd_meter_s=3.0, seed=seed)[0]
    assert many["Z"] == out["Z"] and np.array_equal(many["z_vec"], out["z_vec"]) and np.array_equal(many["remainder"], out["remainder"])
    np.testing.assert_allclose(many["bler"], out["bler"], rtol=1e-12, atol=0)  # (two scorers: the batch's and the environment's)


def test_the_sweeps_above_the_batch_limit():
    name = "k1083"
    assert OC.CASES[name][2] > _lib.BATCH_EPILOGUE_MAX_K
    np.random.seed(4)
    out = online.online_sweep(OC.drop(name), n_points=2, mob_spd_meter_s=3.0, nit=30, seed=1)
    Z = out["Z"]
    assert out["z_vec"].shape == out["bler"].shape == (2, 1083) and out["remainder"].shape == (2,)
    assert np.all((0 <= out["z_vec"]) & (out["z_vec"] < Z)) and np.all(out["z_vec"] == np.floor(out["z_vec"])) and np.all(np.isfinite(out["bler"]))
    assert np.all((0 <= out["bler"]) & (out["bler"] <= 1))
    gr = online.online_greedy_sweep(OC.drop(name), n_points=2, mob_spd_meter_s=3.0, seed=1)
    assert gr["z_vec"].shape == gr["bler"].shape == (2, 1083) and np.all((0 <= gr["z_vec"]) & (gr["z_vec"] < gr["Z"])) and np.all(np.isfinite(gr["bler"]))


def test_refusals_leave_the_handle_alone():
    L = _lib.lib()
    name = "k75"
    _, _, K, Z = OC.CASES[name]
    gX, rv = OC.factor(name), OC.randv(name, 0)
    env, other = new_env(name), new_env("k192")
    s = _lib.Solver.from_env(env, Z, 3, ETA, dtype=_lib.F64)
    s.iterate(3, None, seed=5)
    fields, sizes, rounded = loop_fields(s), s._sizes(), s.round(Z, gX, rv)[0].tobytes()

    def refused(env_h, Zr, randv):
        z, rem = np.full(K, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
        rc = L.mmw_round_env(s._h, env_h, Zr, gX.shape[1], _lib._pd(_lib._f64(gX)), 1, _lib._pd(randv), _lib._pi(z), _lib._pi(rem))
        msg = L.mmw_last_error().decode()
        assert rc == -1 and msg.startswith("mmw_round_env:") and np.all(z == 7) and rem[0] == 7, (rc, msg)
        return msg

    assert "K = 192" in refused(other._h, Z, _lib._f64(rv))
    assert "LDS" in refused(env._h, 4801, np.zeros((4801, gX.shape[1])))
    if _lib.device_count() > 1:  # an environment on another device needs a second device to exist
        ap, p0, _ = OC.positions(name)
        far = _lib.DeviceEnv(p0, ap, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=1)
        assert "device 1" in refused(far._h, Z, _lib._f64(rv))
        far.close()
    with pytest.raises(_lib.MMWError, match="mmw_round_env"):
        s.round_env(other, Z, gX, rv)
    bad = np.array(OC.positions(name)[1])
    bad[3, 1] = np.nan
    gen = env.generation
    with pytest.raises(_lib.MMWError, match="mmw_env_move"):
        env.move(bad)
    assert loop_fields(s) == fields and s._sizes() == sizes and s.round(Z, gX, rv)[0].tobytes() == rounded
    assert s.round_env(env, Z, gX, rv)[0].tobytes() == rounded  # (the refused move changed nothing the library holds)
    assert env.generation == gen + 1  # the wrapper counted the attempt: states handed out before are void either way
    s.close()
    env.close()
    other.close()
