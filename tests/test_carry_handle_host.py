"""CPU-only checks of the carry across states on the solver handle (mmw_carry, mmw_carry_map, csrc/solver_carry.h) and of the workflow
built on it (`online.online_resolve_sweep`): the declarations and exports, the refusals that need no device, the host merge of
mmw_carry_map on device -1 handles against tests/helpers/carry_oracle.py (keys in a dictionary, no merged rows), the argument checks
of the sweep and its per-point seed rule on stubs.

The state pairs are those of tests/test_hip_carry_handle.py: carry_oracle's (a), (b), (c_lose), (c_gain), (k192_moved) and the three
drops of tests/helpers/online_cases.py moved one second at 3 m/s.  The counts of what every moved pair gains and loses are asserted
here, so that a change of the generators cannot hollow the GPU tests out."""
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import carry_oracle  # noqa: E402
import online_cases as OC  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch, mmw, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402

DECLARATIONS = [
    "int mmw_carry(mmw_solver* dst, mmw_solver* src);",
    "int mmw_carry_map(mmw_solver* dst, mmw_solver* src, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc);",
]


@functools.lru_cache(maxsize=None)
def pairs():
    """name -> (old state, new state, Z old, Z new)"""
    out = {"a": carry_oracle.moved_pair(5, carry_oracle.PAIR_A_SEED) + (6, 7), "b": carry_oracle.pair_b() + (2, 3),
           "c_lose": carry_oracle.pair_c("lose") + (2, 2), "c_gain": carry_oracle.pair_c("gain") + (2, 2),
           "k192_moved": carry_oracle.moved_pair(8, 2) + (10, 9)}
    for n in OC.NAMES:
        Z = OC.CASES[n][3]
        out[n] = (OC.host_state(n, 0), OC.host_state(n, 1), Z, Z)
    return out


FIVE = ("a", "b", "c_lose", "c_gain", "k192_moved")


def last_error():
    return _lib.lib().mmw_last_error().decode()


def host_pair(name, Zs=None):
    old, new, zo, zn = pairs()[name]
    zo, zn = Zs or (zo, zn)
    return _lib.Solver(zo, old, 3, 0.05, device=-1), _lib.Solver(zn, new, 3, 0.05, device=-1), orc.Pattern(zo, old), orc.Pattern(zn, new)


def test_both_entries_are_declared_and_exported():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmw_hip.h")).read())
    L = _lib.lib()
    for decl in DECLARATIONS:
        assert decl in txt, decl
        name = re.search(r"(mmw_[a-z_]+)\(", decl).group(1)
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert callable(_lib.Solver.carry_from) and callable(_lib.Solver.carry_map)


def test_null_handles_are_refused():
    L = _lib.lib()
    src, dst, _, _ = host_pair("b")
    m = np.zeros(64, dtype=np.int32)
    for a, b in ((None, src._h), (dst._h, None), (None, None)):
        assert L.mmw_carry(a, b) == -1 and "null solver handle" in last_error()
        assert L.mmw_carry_map(a, b, _lib._pi(m), 1, _lib._pi(m), 1) == -1 and "null pointer" in last_error()
    assert L.mmw_carry_map(dst._h, src._h, None, dst.nnzL, _lib._pi(m), dst.C) == -1 and "null pointer" in last_error()
    src.close()
    dst.close()


def test_carry_on_host_only_handles_answers_minus_three():
    src, dst, _, _ = host_pair("a")
    with pytest.raises(_lib.MMWError, match=r"status -3: mmw_carry: host-only handle"):
        dst.carry_from(src)
    with pytest.raises(_lib.MMWError, match=r"status -1: mmw_carry: the handle cannot carry from itself"):
        dst.carry_from(dst)
    src.close()
    dst.close()


# what every moved pair gains and loses (the table of DESIGN.md §7b-resolve; the exact figures for the three drops, non-zero for the others)
COUNTS = {"k75": (198, 242, 37, 50), "k192": (706, 474, 53, 57), "k1083": (4942, 5516, 534, 464)}


@pytest.mark.parametrize("name", ("a", "k192_moved") + tuple(OC.NAMES))
def test_the_moved_pairs_gain_and_lose_entries_and_pairs(name):
    old, new, zo, zn = pairs()[name]
    po, pn = orc.Pattern(zo, old), orc.Pattern(zn, new)
    lmap, cmap = carry_oracle.maps(po, pn)
    back_l, back_c = carry_oracle.maps(pn, po)
    K = pn.K
    f, fb = cmap[K:K + pn.E_asso], back_c[K:K + po.E_asso]
    got = (int(np.sum(lmap < 0)), int(np.sum(back_l < 0)), int(np.sum(f < 0)), int(np.sum(fb < 0)))
    print(name, "L gained / lost, pairs gained / lost:", got, "longest new row", int(np.max(np.diff(pn.indptr))))
    assert all(g > 0 for g in got), got
    if name in COUNTS:
        assert got == COUNTS[name]
    # the trap: a gained pair whose entry the old pattern stores -- as a gain entry
    gained = np.flatnonzero(f < 0)
    stored = lmap[pn.asso_ab[gained]] >= 0
    if name in COUNTS:
        assert np.all(stored), name
    else:
        assert np.any(stored), name
    if name == "k1083":
        rows = np.bincount(pn.row, minlength=K)
        assert rows.max() == 82  # longer than one wavefront: the lanes of k_carry_rows loop


def test_pair_b_gains_pairs_whose_entry_the_old_pattern_lacks():
    old, new, zo, zn = pairs()["b"]
    po, pn = orc.Pattern(zo, old), orc.Pattern(zn, new)
    lmap, cmap = carry_oracle.maps(po, pn)
    f = cmap[pn.K:pn.K + pn.E_asso]
    assert np.all(f < 0) and np.all(lmap[pn.asso_ab] < 0)


@pytest.mark.parametrize("name", FIVE + ("k1083",))
def test_carry_map_is_the_helpers_map(name):
    src, dst, po, pn = host_pair(name)
    want_l, want_c = carry_oracle.maps(po, pn)
    lmap, cmap = dst.carry_map(src)
    assert lmap.dtype == np.int32 and cmap.dtype == np.int32 and lmap.shape == (pn.nnzL,) and cmap.shape == (pn.C,)
    assert np.array_equal(lmap, want_l) and np.array_equal(cmap, want_c)
    # and the other way round (what was lost)
    back_l, back_c = src.carry_map(dst)
    wl, wc = carry_oracle.maps(pn, po)
    assert np.array_equal(back_l, wl) and np.array_equal(back_c, wc)
    src.close()
    dst.close()


def test_carry_map_does_not_depend_on_the_slot_counts():
    src, dst, po, pn = host_pair("a", (6, 11))
    src2, dst2, _, _ = host_pair("a", (9, 4))
    want = carry_oracle.maps(po, pn)
    for s, d in ((src, dst), (src2, dst2), (src, dst2)):
        got = d.carry_map(s)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # on one state the maps are the identity, whatever the two Z
    ident = src2.carry_map(src)
    assert np.array_equal(ident[0], np.arange(src.nnzL)) and np.array_equal(ident[1], np.arange(src.C))
    for h in (src, dst, src2, dst2):
        h.close()


def test_carry_map_refuses_another_K_and_wrong_lengths():
    src, dst, _, _ = host_pair("a")
    other, _, _, _ = host_pair("b")
    L = _lib.lib()
    lmap, cmap = np.full(dst.nnzL + 1, 7, dtype=np.int32), np.full(dst.C + 1, 7, dtype=np.int32)
    with pytest.raises(_lib.MMWError, match=r"status -1: mmw_carry_map: K = 75 here, K = 4 in the source"):
        dst.carry_map(other)
    for nl, nc in ((dst.nnzL + 1, dst.C), (dst.nnzL, dst.C + 1), (dst.nnzL - 1, dst.C), (0, 0)):
        assert L.mmw_carry_map(dst._h, src._h, _lib._pi(lmap), nl, _lib._pi(cmap), nc) == -1
        assert "wrong lengths %d, %d, expected nnzL = %d and C = %d" % (nl, nc, dst.nnzL, dst.C) in last_error()
    assert np.all(lmap == 7) and np.all(cmap == 7)  # nothing was written
    for h in (src, dst, other):
        h.close()


# ---- the workflow ---------------------------------------------------------------------------------------------------------------------
def test_online_resolve_sweep_signature_and_argument_checks(monkeypatch):
    par = inspect.signature(online.online_resolve_sweep).parameters
    assert list(par) == ["drop", "n_points", "step_us", "mob_spd_meter_s", "resolution_us", "nit", "eta", "seed", "nattempt", "rank_radio", "device", "dtype",
                         "resolve_nit", "carry", "warm_fraction", "timings"]
    assert (par["n_points"].default, par["step_us"].default, par["mob_spd_meter_s"].default, par["resolution_us"].default, par["nit"].default, par["eta"].default,
            par["nattempt"].default, par["dtype"].default, par["resolve_nit"].default, par["carry"].default, par["warm_fraction"].default) == (
        11, 1e6, 0.1, 1e5, 150, 0.04, 10, _lib.F32, None, False, 1.0 / 3.0)

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(online, "_setup", no_device)
    monkeypatch.setattr(online, "_env", no_device)
    drop = OC.drop("k75")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="resolve_nit must be >= 1"):
            online.online_resolve_sweep(drop, resolve_nit=bad)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="warm_fraction must be in"):
            online.online_resolve_sweep(drop, warm_fraction=bad, carry=True)


def test_the_factor_rule_is_shared():
    """One helper states the rank and the seed of a run's factor: `mmw._run` and the sweep both call it."""
    assert mmw.factor_rank_seed(75, 6, 2, 99) == (10, 99) and mmw.factor_rank_seed(5, 6, 2, 3) == (4, 3)
    assert online.factor_rank_seed is mmw.factor_rank_seed
    assert "factor_rank_seed(" in inspect.getsource(mmw.mmw._run) and "factor_rank_seed(" in inspect.getsource(online.online_resolve_sweep)


class ResolveStubs:
    """An environment that records what `online_resolve_sweep` asks of it, and the solvers it makes."""

    def __init__(self, K, Z, D):
        self.K, self.Z, self.D = K, Z, D
        self.log, self.point = [], -1

    def move(self, xy):
        self.point += 1
        self.log.append(("move", self.point, np.array(xy)))

    def evaluate(self, z, Z):
        self.log.append(("evaluate", self.point, np.array(z), Z))
        return np.ones(self.K), np.full(self.K, 0.25 + self.point)

    def close(self):
        self.log.append(("env.close",))


class StubSolver:
    def __init__(self, env, name, nit=None):
        self.env, self.name, self.nit, self.K = env, name, nit, env.K

    def carry_from(self, src):
        self.env.log.append(("carry", self.name, src.name))

    def iterate(self, n, randv, seed=0):
        assert randv is None
        self.env.log.append(("iterate", self.name, n, seed))

    def sync(self):
        pass

    def factor(self, rank, seed=0, resident=False):
        assert resident
        self.env.log.append(("factor", self.name, rank, seed))
        return np.full((self.K, rank), float(self.name))

    def round_env(self, env, Z, gX, randv):
        assert env is self.env
        self.env.log.append(("round", self.name, float(gX[0, 0]), randv[0].copy()))
        return (np.arange(self.K, dtype=np.int32) % Z)[None], np.array([0], dtype=np.int32)

    def close(self):
        self.env.log.append(("close", self.name))


@pytest.mark.parametrize("carry,resolve_nit", [(False, None), (True, None), (True, 5)])
def test_online_resolve_sweep_follows_the_seed_rule(monkeypatch, carry, resolve_nit):
    K, Z, seed, nit, rr = 7, 3, 5, 20, 2
    rank = min(K - 1, (Z - 1) * rr)
    drop = OC.drop("k75")
    drop.sta_locs = drop.sta_locs[:K].copy()
    drop.sta_dirs = drop.sta_dirs[:K].copy()
    env = ResolveStubs(K, Z, rank)
    first = StubSolver(env, 0)
    gX0 = np.zeros((K, rank))

    class Alg:
        def close(self):
            env.log.append(("alg.close",))

    def from_env(e, Z_, n, eta, rank_radio=2, dtype=None):
        assert e is env and Z_ == Z and eta == 0.04 and rank_radio == rr and dtype == _lib.F32
        env.log.append(("create", env.point, n))
        return StubSolver(env, env.point, n)

    monkeypatch.setattr(online, "_setup", lambda d, *a: (env, Alg(), first, Z, gX0))
    monkeypatch.setattr(_lib.Solver, "from_env", staticmethod(from_env))
    np.random.seed(11)
    nxt = np.random.RandomState(11).random_sample()
    timings = []
    out = online.online_resolve_sweep(drop, n_points=3, step_us=2e5, mob_spd_meter_s=3.0, nit=nit, seed=seed, nattempt=4, resolve_nit=resolve_nit, carry=carry,
                                      timings=timings)
    assert np.random.random_sample() == nxt  # the global stream is not touched
    n_p = resolve_nit if resolve_nit is not None else batch.warm_iterations(nit, 1.0 / 3.0) if carry else nit
    assert n_p == {(False, None): 20, (True, None): 7, (True, 5): 5}[(carry, resolve_nit)]
    assert out["iters"] == [nit, n_p, n_p] and out["Z"] == Z
    want = []
    for p in range(3):
        want.append(("move", p))
        if p:
            want.append(("create", p, n_p))
            if carry:
                want.append(("carry", p, p - 1))
            key = probe_seed(seed, 0, 0xC0000 | p)
            want += [("iterate", p, n_p, key), ("factor", p, rank, key)]
            if p > 1:
                want.append(("close", p - 1))
        r = np.random.default_rng(probe_seed(seed, 0, 0x80000 | p)).standard_normal((Z, rank))
        want.append(("round", p, float(p), r / np.linalg.norm(r, axis=1, keepdims=True)))
        want.append(("evaluate", p))
    want += [("close", 2), ("alg.close",), ("env.close",)]  # the first solve's handle is the alg's to close
    assert [g[0] for g in env.log] == [w[0] for w in want], [g[0] for g in env.log]
    for got, w in zip(env.log, want):
        if w[0] in ("create", "carry", "iterate", "factor", "close"):
            assert tuple(got) == tuple(w), (got, w)
        if w[0] == "round":
            assert got[1] == w[1] and got[2] == w[2] and np.array_equal(got[3], w[3]), ("round", w[1])
    assert len(timings) == 3 and all(set(t) == {"create_s", "carry_s", "iterate_s", "epilogue_s", "evaluate_s", "step_s"} and min(t.values()) >= 0.0 for t in timings)
    assert timings[0]["create_s"] >= 0.0 and timings[0]["carry_s"] == 0.0 and timings[0]["iterate_s"] == 0.0
