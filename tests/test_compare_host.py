"""`online.compare` on stub handles (no GPU): the order of the calls, the key of every method, "spectral" only when named, the
unknown-method error before any device work, and everything closed on every path."""
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import online_cases as OC  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402

K, Z, RR = 7, 3, 2
ALL = batch.METHODS + batch.OPT_IN_METHODS


class Stubs:
    """The environment, the solver handle, the algorithm object and the greedy handle in one, all writing to one log.  The rounding
    leaves users 1 and 4 over; MAX_ASSO leaves user 2 over.  `fail_at`: the logged call that raises."""

    def __init__(self, fail_at=None):
        self.log, self.fail_at = [], fail_at
        self.K = K

    def say(self, *rec):
        self.log.append(rec)
        if rec[0] == self.fail_at:
            raise RuntimeError("stub: %s failed" % rec[0])

    # the environment
    def device_state(self):
        self.say("device_state")
        return "the state"

    def evaluate(self, z, Zs):
        self.say("evaluate", np.array(z), Zs)
        return np.ones(K), np.asarray(z) / 10.0 + len([r for r in self.log if r[0] == "evaluate"])

    def close(self):
        self.say("env.close")

    # the solver handle
    def factor_random(self, cols, seed, resident=False, index_order=False):
        self.say("factor_random", cols, seed, resident, index_order)
        return "rand block"

    def factor_spectral(self, Zs, seed=0, resident=False, index_order=False):
        self.say("factor_spectral", Zs, resident, index_order)
        return "spectral block"

    def round_attempts(self, Zs, gX, nattempt, seed, pick="first", all_attempts=False):
        self.say("round_attempts", Zs, gX, nattempt, seed, pick)
        z = (np.arange(K, dtype=np.int32) + (1 if gX == "rand block" else 2)) % Zs
        z[[1, 4]] = -1
        return z, np.array([2] * nattempt, dtype=np.int32), nattempt - 1


class Alg:
    def __init__(self, st):
        self.st = st

    def _device_solver(self, Zs, state):
        self.st.say("device_solver", Zs, state)
        return self.st

    def close(self):
        self.st.say("alg.close")


class Greedy:
    def __init__(self, st):
        self.st = st

    def key(self, kind):
        self.st.say("greedy.key", kind)
        return np.full(K, 10.0 + kind)

    def run(self, key, Zs, nattempt):
        self.st.say("greedy.run", key.copy(), Zs, nattempt)
        z = np.arange(K, dtype=np.int32)[::-1] % Zs
        rem = 0
        if key[0] == 11.0:
            z[2], rem = -1, 1
        return z, Zs, rem

    def close(self):
        self.st.say("greedy.close")


Z_MMW = (np.arange(K) % Z).astype(np.float64)


def install(monkeypatch, st):
    def env(drop, device):
        st.say("env", np.array(drop.sta_locs), np.array(drop.ap_locs), device)
        return st

    def search(state, nit, eta, seed, rank_radio, device, dtype):
        st.say("search", state, nit, eta, seed, rank_radio, device, dtype)
        return Alg(st), Z_MMW.copy(), Z, 0, [5, 3, 2, 3]

    def from_env(e):
        assert e is st
        st.say("greedy.from_env")
        return Greedy(st)

    monkeypatch.setattr(online, "_env", env)
    monkeypatch.setattr(online, "_search", search)
    monkeypatch.setattr(_lib.GreedyHandle, "from_env", staticmethod(from_env))


def drop7():
    d = OC.drop("k75")
    d.sta_locs = d.sta_locs[:K].copy()
    return d


def filled(z, key):
    z = np.asarray(z)
    out = z.astype(np.float64)
    un = z < 0
    if un.any():
        out[un] = np.random.default_rng(key).integers(0, Z, int(un.sum()))
    return out


def same_log(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert len(g) == len(w), g[0]
        for a, b in zip(g[1:], w[1:]):
            assert np.array_equal(a, b), (g[0], a, b)


def test_signature_and_defaults():
    sig = inspect.signature(online.compare).parameters
    assert list(sig) == ["drop_or_geometry", "nit", "eta", "seed", "nattempt", "rank_radio", "device", "dtype", "methods", "timings"]
    assert [sig[k].default for k in list(sig)[1:]] == [150, 0.04, 0, 10, 2, 0, _lib.F32, batch.METHODS, None]


@pytest.mark.parametrize("methods", [batch.METHODS, ALL, ("masso", "spectral"), ("rand",), ()], ids=["default", "all", "masso-spectral", "rand", "none"])
@pytest.mark.parametrize("geometry", ["drop", "pair"])
def test_calls_keys_and_results(monkeypatch, methods, geometry):
    st = Stubs()
    install(monkeypatch, st)
    d = drop7()
    sta, ap = d.sta_locs.copy(), d.ap_locs.copy()
    seed, natt = 5, 4
    np.random.seed(3)
    nxt = np.random.RandomState(3).random_sample()
    timings = {}
    kw = {} if methods is batch.METHODS else {"methods": methods}
    out = online.compare(d if geometry == "drop" else (sta.tolist(), ap.tolist()), nit=20, eta=0.05, seed=seed, nattempt=natt, rank_radio=RR, device=1,
                         dtype=_lib.F64, timings=timings, **kw)
    assert np.random.random_sample() == nxt  # the global stream is not touched
    key = {name: probe_seed(seed, 0, 0x40000 | ALL.index(name)) for name in ALL}
    assert [key[n] & 0xFFFFF for n in ALL] == [0x40000, 0x40001, 0x40002, 0x40003]
    want = [("env", sta, ap, 1), ("device_state",), ("search", "the state", 20, 0.05, seed, RR, 1, _lib.F64), ("device_solver", Z, "the state")]
    zs = {"mmw": Z_MMW}
    rems = {"mmw": 0}
    greedy_made = False
    for name in methods:
        if name in ("rand", "spectral"):
            block = name + " block"
            want.append(("factor_random", Z * RR, key[name], True, True) if name == "rand" else ("factor_spectral", Z, True, True))
            want.append(("round_attempts", Z, block, natt, key[name], "first"))
            z = (np.arange(K) + (1 if name == "rand" else 2)) % Z
            z[[1, 4]] = -1
            zs[name], rems[name] = filled(z, key[name]), 2
        else:
            kind = {"mgain": 0, "masso": 1}[name]
            if not greedy_made:
                want.append(("greedy.from_env",))
                greedy_made = True
            want += [("greedy.key", kind), ("greedy.run", np.full(K, 10.0 + kind), Z, 1)]
            z = np.arange(K)[::-1] % Z
            if kind == 1:
                z[2] = -1
            zs[name], rems[name] = filled(z, key[name]), kind
    order = ("mmw",) + tuple(methods)
    want += [("evaluate", zs[n], Z) for n in order]
    want += ([("greedy.close",)] if greedy_made else []) + [("alg.close",), ("env.close",)]
    same_log(st.log, want)
    assert ("factor_spectral" in [r[0] for r in st.log]) == ("spectral" in methods)
    assert out["Z"] == Z and out["probes"] == [5, 3, 2, 3]
    assert list(out["z_vec"]) == list(out["remainder"]) == list(out["bler"]) == list(order)
    for i, n in enumerate(order):
        assert out["z_vec"][n].dtype == np.float64 and np.array_equal(out["z_vec"][n], zs[n]) and out["remainder"][n] == rems[n]
        assert np.all((out["z_vec"][n] >= 0) & (out["z_vec"][n] < Z))
        assert np.array_equal(out["bler"][n], zs[n] / 10.0 + (i + 1))  # one evaluate per method, in this order
    assert set(timings) == {"search_s", "baselines_s", "evaluate_s", "arm_s"} and list(timings["arm_s"]) == list(methods)


@pytest.mark.parametrize("methods", [("rand", "bogus"), ("lrp",), ("mmw",), ("rand", "Spectral")])
def test_an_unknown_method_raises_by_name_before_any_device_work(monkeypatch, methods):
    st = Stubs()
    install(monkeypatch, st)
    bad = [m for m in methods if m not in ALL][0]
    with pytest.raises(ValueError, match="got %r" % bad):
        online.compare(drop7(), methods=methods)
    assert st.log == []


@pytest.mark.parametrize("fail_at,closed", [("device_state", ["env.close"]), ("search", ["env.close"]), ("device_solver", ["alg.close", "env.close"]),
                                            ("factor_random", ["alg.close", "env.close"]), ("round_attempts", ["alg.close", "env.close"]),
                                            ("greedy.from_env", ["alg.close", "env.close"]), ("greedy.key", ["greedy.close", "alg.close", "env.close"]),
                                            ("greedy.run", ["greedy.close", "alg.close", "env.close"]), ("factor_spectral", ["greedy.close", "alg.close", "env.close"]),
                                            ("evaluate", ["greedy.close", "alg.close", "env.close"])])
def test_everything_is_closed_when_a_step_raises(monkeypatch, fail_at, closed):
    st = Stubs(fail_at=fail_at)
    install(monkeypatch, st)
    timings = {}
    with pytest.raises(RuntimeError, match="stub: %s failed" % fail_at.replace(".", r"\.")):
        online.compare(drop7(), methods=ALL, timings=timings)
    names = [r[0] for r in st.log]
    assert names[names.index(fail_at) + 1:] == closed
    assert timings == {}
