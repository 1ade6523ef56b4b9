"""CPU-only checks of the online sweeps on the solver handle (mmw_env_move, mmw_round_env, mmw_gm_create_from_env,
sig_sdp_mmw_amd/online.py): the declarations and exports, the refusals that need no device, the generation rule of a
`DeviceState`, gm.py's route for a generator's state, and the per-point generator rule of `online_sweep` on stubs."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, state_from

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import online_cases as OC  # noqa: E402

from sig_sdp_mmw_amd import _lib, gm, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import sdp_solver  # noqa: E402

DECLARATIONS = [
    "int mmw_env_move(mmw_env* e, const double* sta_xy);",
    "int mmw_round_env(mmw_solver* s, mmw_env* e, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out, int32_t* rem_out);",
    "int mmw_gm_create_from_env(mmw_gm** out, mmw_env* e);",
]


def test_the_three_entries_are_declared_and_exported():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmw_hip.h")).read())
    L = _lib.lib()
    for decl in DECLARATIONS:
        assert decl in txt, decl
        name = re.search(r"(mmw_[a-z_]+)\(", decl).group(1)
        assert name in _lib.EXPORTS and hasattr(L, name)
    for name, cite in (("mmw_env_move", "env.py:74-87"), ("mmw_round_env", "sim_mmw_online.py"), ("mmw_gm_create_from_env", "sim_mmw_online_cmp_methods.py:79-88")):
        comment = txt[:txt.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert cite in comment, (name, cite)  # every entry cites the reference lines it serves


def test_the_python_methods_exist():
    assert callable(_lib.DeviceEnv.move) and callable(_lib.Solver.round_env) and callable(_lib.GreedyHandle.from_env)
    assert callable(online.online_sweep) and callable(online.online_greedy_sweep)
    import inspect
    sweep = inspect.signature(online.online_sweep).parameters
    assert list(sweep)[:13] == ["drop", "n_points", "step_us", "mob_spd_meter_s", "resolution_us", "nit", "eta", "seed", "nattempt", "rank_radio", "device", "dtype", "timings"]
    assert (sweep["n_points"].default, sweep["step_us"].default, sweep["nit"].default, sweep["eta"].default, sweep["nattempt"].default, sweep["dtype"].default) == (11, 1e6, 150, 0.04, 10, _lib.F32)


def last_error():
    return _lib.lib().mmw_last_error().decode()


def test_null_handles_answer_minus_one():
    L = _lib.lib()
    xy = np.zeros((4, 2))
    assert L.mmw_env_move(None, _lib._pd(xy)) == -1 and "mmw_env_move" in last_error()
    h = C.c_void_p()
    assert L.mmw_gm_create_from_env(C.byref(h), None) == -1 and "mmw_gm_create_from_env" in last_error() and not h.value
    assert L.mmw_gm_create_from_env(None, None) == -1
    z, rem = np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.int32)
    assert L.mmw_round_env(None, None, 2, 2, None, 1, _lib._pd(xy), _lib._pi(z), _lib._pi(rem)) == -1 and "null solver handle" in last_error()


def test_round_env_on_a_host_only_handle_answers_minus_three():
    state = state_from(load_golden("run_env75"))
    s = _lib.Solver(4, state, 3, 0.1, device=-1)
    randv = np.ones((1, 4, 8)) / np.sqrt(8.0)
    gX = np.ones((s.K, 8))
    z, rem = np.full(s.K, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    L = _lib.lib()
    assert L.mmw_round(s._h, 4, 8, _lib._pd(gX), 1, _lib._pd(randv), _lib._pi(z), _lib._pi(rem)) == -3  # the neighbouring entry
    want = last_error()
    assert L.mmw_round_env(s._h, None, 4, 8, _lib._pd(gX), 1, _lib._pd(randv), _lib._pi(z), _lib._pi(rem)) == -3 and last_error() == want
    assert np.all(z == 7) and rem[0] == 7
    s.close()


class StubEnv:
    """What a DeviceState asks of where it lives, with DeviceEnv's generation counter."""
    K = 5

    def __init__(self):
        self.generation, self.calls = 0, []

    def state(self):
        self.calls.append("state")
        return ("S%d" % self.generation, "Q", "h")

    def bounds(self):
        self.calls.append("bounds")
        return 2, 3

    def solver(self, *a, **k):
        self.calls.append("solver")
        return object()


def test_a_stale_device_state_raises():
    env = StubEnv()
    old = _lib.DeviceState(env)
    assert old.host()[0] == "S0" and old.env is env and old[1] == "Q" and len(old) == 3
    env.generation += 1  # what DeviceEnv.move does first
    new = _lib.DeviceState(env)
    assert new is not old and new.generation == 1 and new.host()[0] == "S1"
    env.calls.clear()
    for use in (old.host, lambda: old[0], lambda: list(old), lambda: old.env, old.check,
                lambda: sdp_solver()._device_solver(3, old), lambda: gm.MAX_GAIN.run(-1, old, not_Z_bound=True)):
        with pytest.raises(_lib.MMWError, match="generation 0"):
            use()
    from sig_sdp_mmw_amd.binary_search import binary_search_relaxation
    with pytest.raises(_lib.MMWError, match="generation 0"):
        binary_search_relaxation().set_bounds(old)
    assert env.calls == []  # nothing of the new arrays was read on the old state's behalf
    assert binary_search_relaxation().set_bounds(new) == (2, 3)
    # identity is content: a solver object that holds the old state does not take the new one for it
    alg = sdp_solver()
    alg._dev = (None, old, object())
    assert alg._same_state(old) and not alg._same_state(new)
    alg._dev = None


def test_device_env_counts_generations(monkeypatch):
    """DeviceEnv.move bumps the generation before the library is asked, and device_state() hands out a new object per call."""
    calls = []

    class Lib:
        def mmw_env_move(self, h, xy):
            calls.append("move")
            return 0

        def mmw_env_sizes(self, h, sz):
            sz[2], sz[3] = 11, 4
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    env = _lib.DeviceEnv.__new__(_lib.DeviceEnv)
    env.K, env.A, env.device, env.generation, env._h = 3, 2, 0, 0, C.c_void_p()
    a = env.device_state()
    env.move(np.zeros((3, 2)))
    b = env.device_state()
    assert calls == ["move"] and env.generation == 1 and (env.nnzS, env.nnzQ) == (11, 4) and a is not b and (a.generation, b.generation) == (0, 1)
    with pytest.raises(_lib.MMWError):
        a.check()
    b.check()
    with pytest.raises(_lib.MMWError, match=r"\(K, 2\)"):
        env.move(np.zeros((4, 2)))
    assert env.generation == 1


def test_gm_takes_a_generators_state_through_from_env(monkeypatch):
    """gm.py on the DeviceState of a DeviceEnv: the handle comes from GreedyHandle.from_env and the key from the handle; host() is
    never called."""
    K = 6
    env = _lib.DeviceEnv.__new__(_lib.DeviceEnv)
    env.K, env.device, env.generation, env._h = K, 0, 0, C.c_void_p()
    made = []

    class StubHandle:
        def __init__(self):
            self.K, self.asked = K, []

        def key(self, kind):
            self.asked.append(("key", kind))
            return np.arange(K, dtype=np.float64)

        def run(self, key, Z, nattempt):
            self.asked.append(("run", Z, nattempt, key.tolist()))
            return np.arange(K, dtype=np.int32) % 3, 3, 0

        def pass_(self, order, nattempt):
            self.asked.append(("pass", list(order)))
            return np.asarray(order[:2])

        def assign(self, order, pref):
            self.asked.append(("assign",))
            return np.zeros(K, dtype=np.int32), 0

        def close(self):
            self.asked.append(("close",))

    def from_env(e):
        assert e is env
        made.append(StubHandle())
        return made[-1]

    def no_host(self):
        raise AssertionError("gm.py copied a generator's state to the host")

    monkeypatch.setattr(_lib.GreedyHandle, "from_env", staticmethod(from_env))
    monkeypatch.setattr(_lib.DeviceState, "host", no_host)
    monkeypatch.setattr(_lib.DeviceEnv, "state", no_host)
    monkeypatch.setitem(gm._cache, "handle", None)
    monkeypatch.setitem(gm._cache, "key", None)
    monkeypatch.setitem(gm._cache, "held", None)
    ds = env.device_state()
    z, ZZ, rem = gm.MAX_GAIN.run(-1, ds, not_Z_bound=True, order="stable")
    assert len(made) == 1 and made[0].asked == [("key", 0), ("run", K, 1, list(range(K)))] and ZZ == 3 and rem == 0 and z.tolist() == [0, 1, 2, 0, 1, 2]
    z, ZZ, rem = gm.MAX_ASSO.run(2, ds, order="reference")  # the same state: the same handle, one pass per slot
    assert len(made) == 1 and made[0].asked[2] == ("key", 1) and [a[0] for a in made[0].asked[3:]] == ["pass", "pass"]
    np.random.seed(0)
    gm.MAX_RAND.run(2, ds)
    assert len(made) == 1 and made[0].asked[-1] == ("assign",)
    env.generation = 1  # the environment moved: a new state gets a new handle, the old one is closed
    gm.MAX_GAIN.run(-1, env.device_state(), not_Z_bound=True, order="stable")
    assert len(made) == 2 and made[0].asked[-1] == ("close",)
    with pytest.raises(_lib.MMWError):
        gm.MAX_GAIN.run(-1, ds, not_Z_bound=True, order="stable")


class SweepStubs:
    """An environment and a solver that record what `online_sweep` asks of them; round_env leaves user 1 over in every attempt
    but the one named by `feasible_at`."""

    def __init__(self, K, Z, D, feasible_at):
        self.K, self.Z, self.D, self.feasible_at = K, Z, D, feasible_at
        self.log, self.point, self.attempt = [], -1, 0
        self.gX = np.zeros((K, D))

    # the environment
    def move(self, xy):
        self.point += 1
        self.attempt = 0
        self.log.append(("move", self.point, np.array(xy)))

    def evaluate(self, z, Z):
        self.log.append(("evaluate", self.point, np.array(z), Z))
        return np.ones(self.K), np.full(self.K, 0.25 + self.point)

    def close(self):
        self.log.append(("close",))

    # the solver
    def round_env(self, env, Z, gX, randv):
        assert env is self and gX is self.gX and randv.shape == (1, Z, self.D)
        self.log.append(("round", self.point, self.attempt, randv[0].copy()))
        ok = self.feasible_at.get(self.point) == self.attempt
        self.attempt += 1
        z = np.arange(self.K, dtype=np.int32) % Z
        if not ok:
            z[1] = z[4] = -1
        return z[None], np.array([0 if ok else 2], dtype=np.int32)


def test_online_sweep_draws_every_point_from_its_own_generator(monkeypatch):
    K, Z, D, seed, natt = 7, 3, 4, 5, 3
    drop = OC.drop("k75")
    drop.sta_locs = drop.sta_locs[:K].copy()
    drop.sta_dirs = drop.sta_dirs[:K].copy()
    stubs = SweepStubs(K, Z, D, feasible_at={0: 0, 1: 2})  # point 0: first attempt; point 1: the third; point 2: none

    class Alg:
        def close(self):
            stubs.log.append(("alg.close",))

    monkeypatch.setattr(online, "_setup", lambda d, *a: (stubs, Alg(), stubs, Z, stubs.gX))
    np.random.seed(11)
    nxt = np.random.RandomState(11).random_sample()
    p0 = drop.sta_locs.copy()
    timings = []
    out = online.online_sweep(drop, n_points=3, step_us=2e5, mob_spd_meter_s=3.0, seed=seed, nattempt=natt, timings=timings)
    assert np.random.random_sample() == nxt  # the global stream is not touched
    twin = OC.drop("k75")
    twin.sta_locs, twin.sta_dirs = p0.copy(), twin.sta_dirs[:K].copy()
    want_log = []
    for p in range(3):
        rng = np.random.default_rng(probe_seed(seed, 0, 0x80000 | p))
        want_log.append(("move", p, twin.sta_locs.copy()))
        tries = {0: 1, 1: 3, 2: natt}[p]
        for a in range(tries):
            r = rng.standard_normal((Z, D))
            want_log.append(("round", p, a, r / np.linalg.norm(r, axis=1, keepdims=True)))
        z = (np.arange(K) % Z).astype(np.float64)
        if p == 2:
            z[[1, 4]] = rng.integers(0, Z, 2)
        want_log.append(("evaluate", p, z, Z))
        assert out["z_vec"][p].tolist() == z.tolist() and out["remainder"][p] == (2 if p == 2 else 0) and np.all(out["bler"][p] == 0.25 + p)
        twin.step_time(2e5, 3.0, 1e5)
    want_log += [("alg.close",), ("close",)]
    assert len(stubs.log) == len(want_log)
    for got, want in zip(stubs.log, want_log):
        assert got[0] == want[0] and len(got) == len(want)
        for g, w in zip(got[1:], want[1:]):
            assert np.array_equal(g, w), (got[0], got[1])
    assert out["Z"] == Z and out["z_vec"].shape == (3, K) and out["bler"].shape == (3, K) and out["remainder"].dtype == np.int64
    assert len(timings) == 3 and all(set(t) == {"device_s", "step_s"} for t in timings)
    assert np.array_equal(drop.sta_locs, twin.sta_locs)  # the drop walked in place, once per point
