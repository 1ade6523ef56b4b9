"""The sweeps' greedy baselines through the batch ABI on its host path (mmw_batch_gm on a batch made with device = -1): MAX_GAIN /
MAX_ASSO in the stable order against the CPU restatement (tests/helpers/gm_restate.py) and the host GreedyHandle, the keys bitwise
against the reference's scipy expressions, the refusals, and independence of the batch neighbours and of `take`.

States: journal_graph at cells 5 and 7 and the hand-made 2-user one-AP state, all three in ONE batch and each alone.  The tight slot
bounds (5, 5, 1) were picked by running R.slot_major here: they leave 13 / 27 / 1 (gain) and 14 / 32 / 1 (asso) users over.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import gm_restate as R  # noqa: E402

from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import _state_at, journal_graph  # noqa: E402

RHO = 75e-4
NAMES = ["j5", "j7", "one_ap"]
BOUNDS = {"roomy": [40, 40, 40], "tight": [5, 5, 1], "unbounded": [0, -1, 0]}
KEYS = [R.gain_key, R.asso_key]


def nofill(high, size):
    return np.full(size, -1)


def make_states():
    one_ap = _state_at(np.array([[3.0, 4.0], [15.5, 12.25]]), np.array([[10.0, 10.0]]))[0]
    return [journal_graph(5, RHO, seed=3), journal_graph(7, RHO, seed=1), one_ap]


@pytest.fixture(scope="module")
def states():
    return make_states()


@pytest.fixture(scope="module")
def hb(states):
    b = _lib.BatchSolver([4] * len(states), states, 1, 0.04, device=-1)
    yield b
    b.close()


def expected(st, kind, Z, natt):
    key = KEYS[kind](st)
    z, ZZ, rem, _ = R.slot_major(key, Z, st, natt, Z <= 0, stable=True, randint=nofill)
    return key, z.astype(np.int32), ZZ, rem


def test_one_ap_state_is_what_it_claims(states):
    S, Q, h = states[2]
    assert Q.toarray().tolist() == [[0, 1], [1, 0]] and S.shape == (2, 2)


@pytest.mark.parametrize("natt", [1, 3])
@pytest.mark.parametrize("bound", list(BOUNDS))
@pytest.mark.parametrize("kind", [0, 1])
def test_batch_gm_is_the_restatement_and_the_host_handle(states, hb, kind, bound, natt):
    Zs = BOUNDS[bound]
    z, ZZ, rem, keys = hb.gm(kind, Zs, natt, keys=True)
    for i, st in enumerate(states):
        key, ze, ZZe, reme = expected(st, kind, Zs[i], natt)
        assert np.array_equal(keys[i], key), (NAMES[i], "key")  # bitwise: scipy's summation order
        assert np.array_equal(z[i], ze) and ZZ[i] == ZZe and rem[i] == reme, (NAMES[i], ZZ[i], ZZe, rem[i], reme)
        assert int(np.sum(z[i] < 0)) == rem[i]
        K = st[0].shape[0]
        g = _lib.GreedyHandle(st, device=-1)
        zh, ZZh, remh = g.run(key, Zs[i] if Zs[i] > 0 else K, natt)
        g.close()
        assert np.array_equal(z[i], zh) and ZZ[i] == ZZh and rem[i] == remh, NAMES[i]
        R.check_slots(st, z[i], z[i] >= 0)
        if bound == "tight":
            assert rem[i] > 0, NAMES[i]
        else:
            assert rem[i] == 0 and ZZ[i] == z[i].max() + 1, NAMES[i]


def test_results_are_independent_of_the_neighbours_and_of_take(states, hb):
    for kind in (0, 1):
        Zs = BOUNDS["tight"]
        z, ZZ, rem, keys = hb.gm(kind, Zs, 3, keys=True)
        for i, st in enumerate(states):
            one = _lib.BatchSolver([4], [st], 1, 0.04, device=-1)
            z1, ZZ1, rem1, k1 = one.gm(kind, [Zs[i]], 3, keys=True)
            one.close()
            assert np.array_equal(z1[0], z[i]) and ZZ1[0] == ZZ[i] and rem1[0] == rem[i] and np.array_equal(k1[0], keys[i]), NAMES[i]
        zt, ZZt, remt, kt = hb.gm(kind, Zs, 3, take=[True, False, True], keys=True)
        assert zt[1] is None and kt[1] is None and ZZt[1] == -1 and remt[1] == -1
        for i in (0, 2):
            assert np.array_equal(zt[i], z[i]) and ZZt[i] == ZZ[i] and remt[i] == rem[i] and np.array_equal(kt[i], keys[i])


def raw_gm(b, kind, take, Zs, natt, n):
    """mmw_batch_gm with outputs the test owns: (rc, z, zz, rem, key), every output pre-filled with a sentinel."""
    z = np.full(n, -7, dtype=np.int32)
    zz = np.full(b.B, -7, dtype=np.int32)
    rem = np.full(b.B, -7, dtype=np.int32)
    key = np.full(n, -7.0)
    t = None if take is None else _lib._i32(take)
    rc = _lib.lib().mmw_batch_gm(b._h, kind, None if t is None else _lib._pi(t), _lib._pi(_lib._i32(Zs)), natt, _lib._pi(z), _lib._pi(zz),
                                 _lib._pi(rem), _lib._pd(key))
    return rc, z, zz, rem, key


def untouched(r):
    return all(np.all(a == -7) for a in r[1:])


def small_state(q_pairs, weight, K=3):
    S = scipy.sparse.csr_matrix(np.full((K, K), 0.25) + np.eye(K))
    Q = scipy.sparse.lil_matrix((K, K))
    for a, c in q_pairs:
        Q[a, c] = Q[c, a] = weight
    return S, Q.tocsr(), np.full(K, 2.0)


def test_refusals_name_the_instance_and_leave_the_outputs_untouched(states):
    ARG = -1  # MMW_ERR_ARG
    good = states[2]
    err = lambda: _lib.lib().mmw_last_error().decode()  # noqa: E731
    for bad, what in ((small_state([(0, 1), (1, 2)], 1.0), "not a clique"), (small_state([(0, 1)], 0.5), "weight 0.5")):
        b = _lib.BatchSolver([2, 2], [good, bad], 1, 0.04, device=-1)
        r = raw_gm(b, 0, None, [4, 4], 1, 5)
        assert r[0] == ARG and untouched(r), what
        assert "instance 1" in err() and "union of cliques" in err() and "GreedyHandle" in err(), err()
        # the instance is only refused when it takes part
        r = raw_gm(b, 0, [1, 0], [4, 4], 1, 5)
        assert r[0] == 0 and r[2][1] == -1 and r[3][1] == -1 and np.all(r[1][:2] >= 0) and np.all(r[1][2:] == -7), what
        with pytest.raises(_lib.MMWError, match="instance 1"):
            b.gm(1, [4, 4])
        b.close()
    b = _lib.BatchSolver([2], [good], 1, 0.04, device=-1)
    for args, msg in (((2, None, [4], 1, 2), "kind"), ((-1, None, [4], 1, 2), "kind"), ((0, None, [4], 0, 2), "nattempt"),
                      ((0, [0], [4], 1, 2), "no instance takes part")):
        r = raw_gm(b, *args)
        assert r[0] == ARG and untouched(r) and msg in err(), (args, err())
    # the clique with weight 1 right beside: accepted, and a 3-clique is one group
    ok = _lib.BatchSolver([2], [small_state([(0, 1), (1, 2), (0, 2)], 1.0)], 1, 0.04, device=-1)
    z, ZZ, rem = ok.gm(1, [0])
    assert sorted(z[0].tolist()) == [0, 1, 2] and ZZ[0] == 3 and rem[0] == 0
    ok.close()
    b.close()


def test_factor_random_and_env_gm_have_no_host_form(hb):
    with pytest.raises(_lib.MMWError, match="host patterns only"):
        hb.factor_random([1, 2, 3])
