"""CPU-only checks of the one-call rounding on the solver handle (mmw_round_attempts, mmw_round_env_attempts, mmw_round_randv;
`Solver.round_attempts`, `online.round_point_device`, `online_sweep(draws="device")`, `mmw(round_draws="device")`): the declarations
and exports, every refusal that needs no device with its text, the key rules on stubs, and the scenarios of
tests/helpers/round_attempts_cases.py on the reference's own draws -- the precondition of the GPU tests, which cannot pass
vacuously: each scenario's counts are asserted to the integer."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, state_from

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import online_cases as OC  # noqa: E402
import round_attempts_cases as RA  # noqa: E402

from sig_sdp_mmw_amd import _lib, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.mmw import mmw  # noqa: E402

DECLARATIONS = [
    "int mmw_round_attempts(mmw_solver* s, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule, "
    "int32_t* z_out, int32_t* rem_out, int32_t* pick_out, int32_t* z_all);",
    "int mmw_round_env_attempts(mmw_solver* s, mmw_env* e, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule, "
    "int32_t* z_out, int32_t* rem_out, int32_t* pick_out, int32_t* z_all);",
    "int mmw_round_randv(mmw_solver* s, int32_t Zr, int32_t Dp, uint64_t seed, int32_t attempt, double* out, int64_t n);",
]


def test_the_three_entries_are_declared_and_exported():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmw_hip.h")).read())
    L = _lib.lib()
    for decl in DECLARATIONS:
        assert decl in txt, decl
        name = re.search(r"(mmw_[a-z_]+)\(", decl).group(1)
        assert name in _lib.EXPORTS and hasattr(L, name)
    comment = txt[:txt.index("int mmw_round_attempts(")].rsplit("/*", 1)[1]
    for cite in ("sdp_solver.py:18-25", "sdp_solver.py:27-107", "sdp_solver.py:48-49", "sim_mmw_online.py:60", "0x524e4456"):
        assert cite in comment, cite


def test_the_python_surface():
    for f in (_lib.Solver.round_attempts, _lib.Solver.round_env_attempts, _lib.Solver.round_randv, online.round_point_device):
        assert callable(f)
    assert list(inspect.signature(_lib.Solver.round_attempts).parameters) == ["self", "Z", "gX", "nattempt", "seed", "pick", "all_attempts"]
    assert list(inspect.signature(_lib.Solver.round_env_attempts).parameters) == ["self", "env", "Z", "gX", "nattempt", "seed", "pick", "all_attempts"]
    assert list(inspect.signature(online.round_point_device).parameters) == ["solver", "env", "Z", "gX", "nattempt", "key", "pick"]
    p = inspect.signature(online.online_sweep).parameters
    assert p["draws"].default == "host" and p["pick"].default == "first"
    # the re-solving sweep keeps its arguments (test_carry_handle_host.py pins them): its device route is a function of its own
    r, d = inspect.signature(online.online_resolve_sweep).parameters, inspect.signature(online.online_resolve_sweep_device).parameters
    assert list(d) == list(r) + ["pick"] and d["pick"].default == "first" and all(d[k].default == r[k].default for k in r)
    for sweep in (online.online_sweep, online.online_resolve_sweep, online.online_resolve_sweep_device):
        assert "probe_seed(seed, 0, 0x80000 | p)" in sweep.__doc__ and 'draws="device"' in sweep.__doc__
    p = inspect.signature(mmw.__init__).parameters["round_draws"]
    assert p.default == "host" and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "MMW_ROUND" not in open(os.path.join(ROOT, "sig_sdp_mmw_amd", "mmw.py")).read()  # no environment switch


def last_error():
    return _lib.lib().mmw_last_error().decode()


class Outs:
    def __init__(self, K, natt):
        self.z, self.rem, self.pick = np.full(K, 7, dtype=np.int32), np.full(max(natt, 1), 7, dtype=np.int32), C.c_int32(7)

    def args(self):
        return _lib._pi(self.z), _lib._pi(self.rem), C.byref(self.pick), None

    def untouched(self):
        return bool(np.all(self.z == 7) and np.all(self.rem == 7) and self.pick.value == 7)


def test_null_handles_and_pointers_are_refused():
    L = _lib.lib()
    gX = np.ones((4, 2))
    o = Outs(4, 1)
    u64 = C.c_uint64(0)
    assert L.mmw_round_attempts(None, 2, 2, _lib._pd(gX), 1, u64, 0, *o.args()) == -1 and "null solver handle" in last_error()
    assert L.mmw_round_env_attempts(None, None, 2, 2, _lib._pd(gX), 1, u64, 0, *o.args()) == -1 and "null solver handle" in last_error()
    assert L.mmw_round_randv(None, 2, 2, u64, 0, _lib._pd(gX), 4) == -1 and "null solver handle" in last_error()
    s = _lib.Solver(4, state_from(load_golden("run_env75")), 3, 0.1, device=-1)
    g = np.ones((s.K, 8))
    o = Outs(s.K, 1)
    z, rem, pick, _ = o.args()
    for args in ((None, rem, pick, None), (z, None, pick, None), (z, rem, None, None)):
        assert L.mmw_round_attempts(s._h, 4, 8, _lib._pd(g), 1, u64, 0, *args) == -1 and "mmw_round_attempts: null pointer" in last_error()
        assert L.mmw_round_env_attempts(s._h, None, 4, 8, _lib._pd(g), 1, u64, 0, *args) == -1 and "mmw_round_env_attempts: null pointer" in last_error()
    assert L.mmw_round_randv(s._h, 4, 8, u64, 0, None, 32) == -1 and "mmw_round_randv" in last_error()
    assert o.untouched()
    s.close()


def test_a_host_only_handle_answers_minus_three():
    s = _lib.Solver(4, state_from(load_golden("run_env75")), 3, 0.1, device=-1)
    g = np.ones((s.K, 8))
    o = Outs(s.K, 3)
    L = _lib.lib()
    u64 = C.c_uint64(5)
    assert L.mmw_round(s._h, 4, 8, _lib._pd(g), 1, _lib._pd(np.ones((4, 8))), _lib._pi(o.z), _lib._pi(o.rem)) == -3  # the neighbouring entry
    want = last_error()
    assert L.mmw_round_attempts(s._h, 4, 8, _lib._pd(g), 3, u64, 0, *o.args()) == -3 and last_error() == want
    assert L.mmw_round_env_attempts(s._h, None, 4, 8, _lib._pd(g), 3, u64, 1, *o.args()) == -3 and last_error() == want
    out = np.full((4, 8), 7.0)
    assert L.mmw_round_randv(s._h, 4, 8, u64, 0, _lib._pd(out), 32) == -3 and last_error() == want
    assert o.untouched() and np.all(out == 7.0)
    assert s.round_list_builds() == 0  # the counter of list builds answers on any handle, and fetches nothing for it
    one = np.full(2, 7, dtype=np.int32)
    assert L.mmw_read_i32(s._h, _lib.I_ROUND_LIST_BUILDS, _lib._pi(one), 2) == -1 and "ROUND_LIST_BUILDS" in last_error() and np.all(one == 7)
    assert "MMW_I_ROUND_LIST_BUILDS = %d" % _lib.I_ROUND_LIST_BUILDS in open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    with pytest.raises(_lib.MMWError, match="status -3"):
        s.round_attempts(4, g, 3, 5)
    with pytest.raises(_lib.MMWError, match="pick must be"):
        s.round_attempts(4, g, 3, 5, pick="last")
    s.close()


@pytest.mark.parametrize("Z,natt,rule,text", [(4, 0, 0, "nattempt = 0 must be in [1, 256]"), (4, 257, 0, "nattempt = 257 must be in [1, 256]"),
                                               (4, -1, 1, "nattempt = -1"), (4, 3, 2, "pick_rule must be 0"), (4, 3, -1, "pick_rule must be 0"),
                                               (0, 3, 0, "Z and D' must be positive"), (4801, 3, 0, "32 Z bytes exceed the greedy kernel's LDS")])
def test_arguments_are_refused_with_their_text_before_any_device_work(Z, natt, rule, text):
    """On a device -1 handle, which cannot do any device work at all: the argument refusals (-1, each with its text, worded for the
    entry) come before the handle's -3."""
    s = _lib.Solver(4, state_from(load_golden("run_env75")), 3, 0.1, device=-1)
    g = np.ones((s.K, 8))
    L = _lib.lib()
    o = Outs(s.K, 3)
    u64 = C.c_uint64(1)
    assert L.mmw_round_attempts(s._h, Z, 8, _lib._pd(g), natt, u64, rule, *o.args()) == -1
    msg = last_error()
    assert msg.startswith("mmw_round_attempts:") and text in msg, msg
    assert L.mmw_round_env_attempts(s._h, None, Z, 8, _lib._pd(g), natt, u64, rule, *o.args()) == -1
    msg = last_error()
    assert msg.startswith("mmw_round_env_attempts:") and text in msg, msg
    assert o.untouched()
    s.close()


def test_round_randv_refuses_bad_arguments():
    s = _lib.Solver(4, state_from(load_golden("run_env75")), 3, 0.1, device=-1)
    L = _lib.lib()
    out = np.full((4, 8), 7.0)
    u64 = C.c_uint64(1)
    for args, text in (((0, 8, u64, 0, _lib._pd(out), 0), "Z and D' must be positive"), ((4, 0, u64, 0, _lib._pd(out), 0), "Z and D' must be positive"),
                       ((4, 8, u64, -1, _lib._pd(out), 32), "attempt must be >= 0"), ((4, 8, u64, 0, _lib._pd(out), 31), "Z x D'")):
        assert L.mmw_round_randv(s._h, *args) == -1 and last_error().startswith("mmw_round_randv:") and text in last_error(), last_error()
    assert np.all(out == 7.0)
    s.close()


# ---- the scenarios on the reference's own draws ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(RA.SCENARIOS), ids=RA.IDS)
def test_the_scenarios_hold_on_the_reference(key):
    slots, rem = RA.reference_attempts(*key)
    assert rem == RA.SCENARIOS[key]
    assert all(int((slots[a] < 0).sum()) == rem[a] for a in range(RA.NATT))


def test_what_the_scenarios_show():
    S = RA.SCENARIOS
    assert RA.pick_of(S[("k75", 9, 0)], "first") == 0 == RA.pick_of(S[("k75", 9, 0)], "fewest")
    assert RA.pick_of(S[("k75", 9, 3)], "first") == 2 and S[("k75", 9, 3)][3] == 0  # the first feasible, not the last feasible
    late = S[("k75", 8, 0)]
    assert RA.pick_of(late, "first") == 4 == RA.pick_of(late, "fewest")
    assert RA.pick_of(late[:4], "first") == 3 and RA.pick_of(late[:4], "fewest") == 0 and late[0] == late[3]  # the tie goes to the lower
    none = S[("k192", 9, 3)]
    assert 0 not in none and RA.pick_of(none, "first") == 5 and RA.pick_of(none, "fewest") == 4
    # the loop with stop-at-first is rule "first"
    for rem in S.values():
        for n in range(1, RA.NATT + 1):
            assert RA.loop_first(lambda a: (a, rem[a]), n) == (RA.pick_of(rem[:n], "first"),) * 2


# ---- the key rules on stubs -----------------------------------------------------------------------------------------------------------
class SweepStubs:
    """An environment and a solver that record what the sweep asks of them.  Host route: `round_env` leaves users 1 and 4 over in
    every attempt but the one named by `feasible_at`.  Device route: `round_env_attempts` leaves them over at the points not named."""

    def __init__(self, K, Z, D, feasible_at):
        self.K, self.Z, self.D, self.feasible_at = K, Z, D, feasible_at
        self.log, self.point, self.attempt = [], -1, 0
        self.gX = np.zeros((K, D))

    def move(self, xy):
        self.point += 1
        self.attempt = 0
        self.log.append(("move", self.point, np.array(xy)))

    def evaluate(self, z, Z):
        self.log.append(("evaluate", self.point, np.array(z), Z))
        return np.ones(self.K), np.full(self.K, 0.25 + self.point)

    def close(self):
        self.log.append(("close",))

    def _slots(self, ok):
        z = np.arange(self.K, dtype=np.int32) % self.Z
        if not ok:
            z[1] = z[4] = -1
        return z

    def round_env(self, env, Z, gX, randv):
        assert env is self and gX is self.gX and randv.shape == (1, Z, self.D)
        self.log.append(("round", self.point, self.attempt, randv[0].copy()))
        ok = self.feasible_at.get(self.point) == self.attempt
        self.attempt += 1
        return self._slots(ok)[None], np.array([0 if ok else 2], dtype=np.int32)

    def round_env_attempts(self, env, Z, gX, nattempt, seed, pick="first", all_attempts=False):
        assert env is self and gX is self.gX and Z == self.Z and not all_attempts
        self.log.append(("attempts", self.point, nattempt, seed, pick))
        ok = self.point in self.feasible_at
        return self._slots(ok), np.full(nattempt, 0 if ok else 2, dtype=np.int32), self.feasible_at.get(self.point, nattempt - 1)


def small_drop(K):
    drop = OC.drop("k75")
    drop.sta_locs = drop.sta_locs[:K].copy()
    drop.sta_dirs = drop.sta_dirs[:K].copy()
    return drop


def run_on_stubs(monkeypatch, stubs, Z, **kw):
    class Alg:
        def close(self):
            stubs.log.append(("alg.close",))

    monkeypatch.setattr(online, "_setup", lambda d, *a: (stubs, Alg(), stubs, Z, stubs.gX))
    np.random.seed(11)
    nxt = np.random.RandomState(11).random_sample()
    out = online.online_sweep(small_drop(stubs.K), n_points=3, step_us=2e5, mob_spd_meter_s=3.0, **kw)
    assert np.random.random_sample() == nxt  # the global stream is not touched after the search
    return out


def same_logs(got_log, want_log):
    assert len(got_log) == len(want_log), ([g[0] for g in got_log], [w[0] for w in want_log])
    for got, want in zip(got_log, want_log):
        assert got[0] == want[0] and len(got) == len(want)
        for g, w in zip(got[1:], want[1:]):
            assert np.array_equal(g, w), (got[0], got[1])


@pytest.mark.parametrize("pick", ["first", "fewest"])
def test_online_sweep_device_draws_make_one_keyed_call_per_point(monkeypatch, pick):
    K, Z, D, seed, natt = 7, 3, 4, 5, 3
    stubs = SweepStubs(K, Z, D, feasible_at={0: 0, 1: 2})  # point 2: users 1 and 4 left over
    out = run_on_stubs(monkeypatch, stubs, Z, seed=seed, nattempt=natt, draws="device", pick=pick)
    twin = small_drop(K)
    want_log = []
    for p in range(3):
        key = probe_seed(seed, 0, 0x80000 | p)
        want_log += [("move", p, twin.sta_locs.copy()), ("attempts", p, natt, key, pick)]
        z = (np.arange(K) % Z).astype(np.float64)
        if p == 2:
            z[[1, 4]] = np.random.default_rng(key).integers(0, Z, 2)
        want_log.append(("evaluate", p, z, Z))
        assert out["z_vec"][p].tolist() == z.tolist() and out["remainder"][p] == (2 if p == 2 else 0) and np.all(out["bler"][p] == 0.25 + p)
        twin.step_time(2e5, 3.0, 1e5)
    same_logs(stubs.log, want_log + [("alg.close",), ("close",)])
    assert not any(e[0] == "round" for e in stubs.log)


def test_online_sweep_host_draws_make_exactly_todays_calls(monkeypatch):
    K, Z, D, seed, natt = 7, 3, 4, 5, 3
    logs = []
    for kw in ({}, {"draws": "host", "pick": "first"}):
        stubs = SweepStubs(K, Z, D, feasible_at={0: 0, 1: 2})
        run_on_stubs(monkeypatch, stubs, Z, seed=seed, nattempt=natt, **kw)
        logs.append(stubs.log)
    twin = small_drop(K)
    want_log = []
    for p in range(3):
        rng = np.random.default_rng(probe_seed(seed, 0, 0x80000 | p))
        want_log.append(("move", p, twin.sta_locs.copy()))
        for a in range({0: 1, 1: 3, 2: natt}[p]):
            r = rng.standard_normal((Z, D))
            want_log.append(("round", p, a, r / np.linalg.norm(r, axis=1, keepdims=True)))
        z = (np.arange(K) % Z).astype(np.float64)
        if p == 2:
            z[[1, 4]] = rng.integers(0, Z, 2)
        want_log.append(("evaluate", p, z, Z))
        twin.step_time(2e5, 3.0, 1e5)
    for log in logs:
        same_logs(log, want_log + [("alg.close",), ("close",)])


def test_the_sweeps_refuse_unknown_routes_before_the_setup(monkeypatch):
    def no_setup(*a):
        raise AssertionError("the setup ran")

    monkeypatch.setattr(online, "_setup", no_setup)
    for kw, text in (({"draws": "gpu"}, "draws must be"), ({"draws": "device", "pick": "last"}, "pick must be"), ({"pick": "fewest"}, "needs draws='device'")):
        with pytest.raises(ValueError, match=text):
            online.online_sweep(small_drop(7), n_points=1, **kw)
    with pytest.raises(ValueError, match="pick must be"):
        online.online_resolve_sweep_device(small_drop(7), n_points=1, pick="last")


def test_round_point_device_fills_from_the_keys_generator():
    K, Z = 7, 3
    stubs = SweepStubs(K, Z, 4, feasible_at={})
    stubs.point = 0
    key = probe_seed(9, 0, 0x80000 | 4)
    z_vec, rem = online.round_point_device(stubs, stubs, Z, stubs.gX, 0, key, pick="fewest")
    want = (np.arange(K) % Z).astype(np.float64)
    want[[1, 4]] = np.random.default_rng(key).integers(0, Z, 2)
    assert z_vec.tolist() == want.tolist() and rem == 2 and stubs.log == [("attempts", 0, 1, key, "fewest")]  # (nattempt 0 runs one attempt, as round_point)


class StubSolver:
    def __init__(self, K, Z):
        self.K, self.Z, self.calls = K, Z, []

    def round_attempts(self, Z, gX, nattempt, seed, pick="first", all_attempts=False):
        self.calls.append((Z, gX.shape, nattempt, seed, pick))
        z = np.arange(self.K, dtype=np.int32) % Z
        if len(self.calls) % 2 == 0:  # every second call leaves three users over
            z[[0, 2, 5]] = -1
        return z, np.zeros(nattempt, dtype=np.int32), 0

    def round(self, *a):
        raise AssertionError("the host route ran")


def test_mmw_round_draws_device_follows_its_key_formula(monkeypatch):
    K, Z = 9, 4
    alg = mmw(nit=5, eta=0.1, seed=6, round_draws="device", device=0)
    stub = StubSolver(K, Z)
    monkeypatch.setattr(alg, "_device_solver", lambda Z_, state, **kw: stub)
    np.random.seed(3)
    nxt = np.random.RandomState(3).random_sample()
    gX = np.ones((K, 6))
    for call in range(4):
        key = probe_seed(6, 0, 0x20000 | call)
        assert alg.round_key(call) == key
        z_vec, Zr, rem = alg.rounding(Z, gX, "state", nattempt=7)
        want = (np.arange(K) % Z).astype(np.float64)
        if call % 2 == 1:
            want[[0, 2, 5]] = np.random.default_rng(key).integers(0, Z, 3)
        assert z_vec.tolist() == want.tolist() and Zr == Z and rem == (3 if call % 2 else 0)
        assert stub.calls[-1] == (Z, (K, 6), 7, key, "first")
    assert np.random.random_sample() == nxt  # the global stream is not touched by the rounding
    assert alg.round_key(0x20000 + 5) == alg.round_key(5)  # the counter wraps inside its field, the tag bit stays
    sib = alg.sibling()
    assert sib.round_draws == "device" and sib._round_calls == 0 and sib.round_key(0) == probe_seed(6 + 7919, 0, 0x20000)
    assert mmw(nit=5, eta=0.1).round_draws == "host"
    with pytest.raises(ValueError, match="round_draws"):
        mmw(nit=5, eta=0.1, round_draws="gpu")
    # the default route still draws from the global stream, through Solver.round
    host = mmw(nit=5, eta=0.1, seed=6, device=0)
    monkeypatch.setattr(host, "_device_solver", lambda Z_, state, **kw: stub)
    with pytest.raises(AssertionError, match="the host route ran"):
        host.rounding(Z, gX, "state", nattempt=2)
