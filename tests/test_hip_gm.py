"""GPU: the greedy baselines of gm.py (MAX_GAIN / MAX_ASSO / MAX_RAND) on the device against the reference's recorded outputs and the
O(deg) CPU restatement (tests/helpers/gm_restate.py): exact slot assignments, ZZ, remainders and stream positions."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import gm_restate as R  # noqa: E402

from sig_sdp_mmw_amd import _lib, gm  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph, journal_graph_device  # noqa: E402

pytestmark = pytest.mark.gpu

G = load_golden("gm_env")
CASES = [str(c) for c in G["cases"]]
SLOT_CASES = [c for c in CASES if "/rand/" not in c]
RAND_CASES = [c for c in CASES if "/rand/" in c]
KEYS = {"gain": R.gain_key, "asso": R.asso_key}
CLASSES = {"gain": gm.MAX_GAIN, "asso": gm.MAX_ASSO}


def gstate(sname):
    def csr(p):
        shape = tuple(int(x) for x in G[sname + "/" + p + "_shape"])
        return scipy.sparse.csr_matrix((G[sname + "/" + p + "_data"], G[sname + "/" + p + "_indices"], G[sname + "/" + p + "_indptr"]), shape=shape)
    return csr("S"), csr("Q"), np.array(G[sname + "/h_max"])


def recorded_orders(c):
    lens = G[c + "/order_len"]
    pos = G[c + "/order_pos"].astype(np.int64)
    return np.split(pos, np.cumsum(lens)[:-1]) if lens.size else []


def nofill(high, size):
    return np.full(size, -1)


@pytest.mark.parametrize("c", SLOT_CASES)
def test_fixture_cases_recorded_orders_match_reference(c):
    sname, alg = c.split("/")[:2]
    st = gstate(sname)
    Z, natt, nzb = int(G[c + "/Z"]), int(G[c + "/nattempt"]), bool(int(G[c + "/not_Z_bound"]))
    h = _lib.GreedyHandle(st, device=0)
    assert h.groups > 0  # the journal Q is a union of per-AP cliques: the owner path runs
    slot, ZZ, rem = R.drive_abi(h, KEYS[alg](st), Z, natt, nzb, orders=recorded_orders(c))
    ref = G[c + "/z_vec"]
    un = slot < 0
    assert ZZ == int(G[c + "/ZZ"]) and rem == int(G[c + "/rem"])
    assert np.array_equal(slot[~un], ref[~un].astype(np.int64))
    assert np.array_equal(ref[un].astype(np.int64), G[c + "/fill"].astype(np.int64))


@pytest.mark.parametrize("c", [c for c in SLOT_CASES if c.endswith(("/nb", "/infeas", "/att3"))])
def test_fixture_states_live_reference_mode_and_stream(c):
    sname, alg = c.split("/")[:2]
    st = gstate(sname)
    Z, natt, nzb = int(G[c + "/Z"]), int(G[c + "/nattempt"]), bool(int(G[c + "/not_Z_bound"]))
    seed = int(G[c + "/seed"])
    np.random.seed(seed)
    z, ZZ, rem = CLASSES[alg].run(Z, st, nattempt=natt, not_Z_bound=nzb)
    nxt = np.random.random()
    np.random.seed(seed)
    zr, ZZr, remr, _ = R.slot_major(KEYS[alg](st), Z, st, natt, nzb)
    assert np.random.random() == nxt
    assert np.array_equal(z, zr) and ZZ == ZZr and rem == remr
    assert isinstance(z, np.ndarray) and z.dtype == np.float64 and z.shape == (st[0].shape[0],)


@pytest.mark.parametrize("c", RAND_CASES)
def test_max_rand_fixture_and_stream(c):
    st = gstate(c.split("/")[0])
    Z, seed = int(G[c + "/Z"]), int(G[c + "/seed"])
    np.random.seed(seed)
    z, ZZ, rem = gm.MAX_RAND.run(Z, st)
    nxt = np.random.random()
    assert np.array_equal(z, G[c + "/z_vec"]) and ZZ == Z and rem == int(G[c + "/rem"])  # same host: same draws, same argsorts
    assert nxt == float(G[c + "/next"])
    # and against the restatement on the recorded order / preference
    zr, _, remr = R.max_rand(Z, st, G[c + "/rank"].astype(np.int64), G[c + "/pref"].astype(np.int64), randint=nofill)
    un = zr < 0
    assert remr == rem and np.array_equal(z[~un], zr[~un])


def test_max_rand_tight_slots_fill_and_stream():
    st = journal_graph(25, 75e-4, seed=1)
    for Z in (3, 12):
        np.random.seed(21)
        z, ZZ, rem = gm.MAX_RAND.run(Z, st)
        nxt = np.random.random()
        np.random.seed(21)
        K = st[0].shape[0]
        inprod = np.random.randn(Z, K)
        pref = np.argsort(-inprod, axis=0).T
        rank = np.argsort(np.random.randn(K))
        zr, _, remr = R.max_rand(Z, st, rank, pref)
        assert np.random.random() == nxt
        assert np.array_equal(z, zr) and ZZ == Z and rem == remr
        zs, _, _ = R.max_rand(Z, st, rank, pref, randint=nofill)
        R.check_slots(st, zs, zs >= 0)


_BIG = {}


def big_state(name):
    if name not in _BIG:
        _BIG[name] = journal_graph(25, 75e-4, seed=1) if name == "K1875" else journal_graph(28, 0.0319, seed=1)
    return _BIG[name]


@pytest.mark.parametrize("name", ["K1875", "K10003"])
@pytest.mark.parametrize("alg", ["gain", "asso"])
def test_large_states_exact_and_slots_valid(name, alg):
    st = big_state(name)
    K = st[0].shape[0]
    key = KEYS[alg](st)
    np.random.seed(3)
    z, ZZ, rem = CLASSES[alg].run(-1, st, not_Z_bound=True)
    zr, ZZr, remr, _ = R.slot_major(key, -1, st, 1, True, randint=nofill)
    assert ZZ == ZZr and rem == remr == 0
    assert np.array_equal(z, zr)
    R.check_slots(st, z, np.ones(K, dtype=bool))
    # bounded Z on both sides of feasibility
    for Z in (ZZ + 1, max(1, ZZ - 3)):
        z, ZZb, remb = CLASSES[alg].run(Z, st)
        zr, ZZr, remr, _ = R.slot_major(key, Z, st, 1, False, randint=nofill)
        assert ZZb == ZZr and remb == remr
        ok = zr >= 0
        assert np.array_equal(z[ok], zr[ok])
        R.check_slots(st, z, ok)
        assert (remb == 0) == (Z > ZZ - 1)


@pytest.mark.parametrize("name", ["K1875", "K10003"])
@pytest.mark.parametrize("alg", ["gain", "asso"])
def test_stable_mode_matches_stable_restatement(name, alg):
    st = big_state(name)
    key = KEYS[alg](st)
    for Z, nzb in ((-1, True), (8, False)):
        np.random.seed(5)
        z, ZZ, rem = CLASSES[alg].run(Z, st, not_Z_bound=nzb, order="stable")
        nxt = np.random.random()
        np.random.seed(5)
        zr, ZZr, remr, _ = R.slot_major(key, Z, st, 1, nzb, stable=True)
        assert np.random.random() == nxt
        assert np.array_equal(z, zr) and ZZ == ZZr and rem == remr


def test_stable_mode_env_variable(monkeypatch):
    st = journal_graph(8, 75e-4, seed=0)
    monkeypatch.setenv("MMW_GM_ORDER", "stable")
    calls = []
    orig = _lib.GreedyHandle.pass_
    monkeypatch.setattr(_lib.GreedyHandle, "pass_", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    z, ZZ, rem = gm.MAX_ASSO.run(-1, st, not_Z_bound=True)
    zr, ZZr, remr, _ = R.slot_major(R.asso_key(st), -1, st, 1, True, stable=True, randint=nofill)
    assert not calls  # one device call, no per-slot pass
    assert np.array_equal(z, zr) and ZZ == ZZr and rem == remr


def test_negative_h_max_user_ends_early(monkeypatch):
    S, Q, h = journal_graph(8, 75e-4, seed=0)
    h = h.copy()
    h[5] = -1.0
    st = (S, Q, h)
    K = S.shape[0]
    calls = []
    orig = _lib.GreedyHandle.pass_
    monkeypatch.setattr(_lib.GreedyHandle, "pass_", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    for cls, kf in ((gm.MAX_GAIN, R.gain_key), (gm.MAX_ASSO, R.asso_key)):
        for order in ("reference", "stable"):
            del calls[:]
            np.random.seed(9)
            z, ZZ, rem = cls.run(-1, st, not_Z_bound=True, order=order)
            nxt = np.random.random()
            assert ZZ == K and rem == 1
            assert len(calls) < 40  # not K passes
            np.random.seed(9)
            zr, ZZr, remr, _ = R.slot_major(kf(st), -1, st, 1, True, stable=order == "stable")
            assert np.random.random() == nxt and np.array_equal(z, zr) and ZZ == ZZr and rem == remr


def test_edge_cases_empty_q_single_user_one_slot_three_attempts():
    S, Q, h = journal_graph(8, 75e-4, seed=3)
    K = S.shape[0]
    cases = [((S, scipy.sparse.csr_matrix((K, K)), h), "empty Q"),
             ((scipy.sparse.csr_matrix(np.array([[2.0]])), scipy.sparse.csr_matrix((1, 1)), np.array([1.0])), "K = 1"),
             ((S, Q, h), "journal")]
    for st, what in cases:
        for alg in ("gain", "asso"):
            key = KEYS[alg](st)
            for Z, natt, nzb in ((-1, 1, True), (1, 1, False), (4, 3, False), (-1, 3, True)):
                for order, stable in (("reference", False), ("stable", True)):
                    np.random.seed(11)
                    z, ZZ, rem = CLASSES[alg].run(Z, st, nattempt=natt, not_Z_bound=nzb, order=order)
                    nxt = np.random.random()
                    np.random.seed(11)
                    zr, ZZr, remr, _ = R.slot_major(key, Z, st, natt, nzb, stable=stable)
                    assert np.random.random() == nxt, what
                    assert np.array_equal(z, zr) and ZZ == ZZr and rem == remr, (what, alg, Z, natt, order)


def test_general_association_check_on_device():
    S, Q, h = journal_graph(15, 75e-4, seed=2)
    Q = Q.copy()
    Q.data[::3] = 0.6
    st = (S, Q, h)
    hd = _lib.GreedyHandle(st, device=0)
    assert hd.groups == -1
    key = R.gain_key(st)
    for natt, stable in ((1, False), (3, False), (1, True), (2, True)):
        slot, ZZ, rem = R.drive_abi(hd, key, -1, natt, True, stable=stable)
        zr, ZZr, remr, _ = R.slot_major(key, -1, st, natt, True, stable=stable, randint=nofill)
        assert np.array_equal(slot, zr.astype(np.int64)) and ZZ == ZZr and rem == remr


def test_device_state_matches_host_state():
    st_dev_tuple, env = journal_graph_device(15, 75e-4, seed=4)
    ds = env.device_state()
    host = st_dev_tuple  # (the same state, copied to the host once)
    for cls in (gm.MAX_GAIN, gm.MAX_ASSO):
        for order in ("reference", "stable"):
            np.random.seed(2)
            a = cls.run(-1, ds, not_Z_bound=True, order=order)
            np.random.seed(2)
            b = cls.run(-1, host, not_Z_bound=True, order=order)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    np.random.seed(4)
    a = gm.MAX_RAND.run(6, ds)
    np.random.seed(4)
    b = gm.MAX_RAND.run(6, host)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    env.close()
