"""GPU checks of the batch's slot change on the device (csrc/kernels_batch_relayout.h) and of the warm-started probes built on it
(mmw_batch_set_slots_warm, `search_many(..., warm_start=True)`).

One batch of four instances of different sizes -- the golden states run_env75, run_er120, run_dense60 and journal_graph(8, 75e-4,
seed=2) (K = 192) -- so that a new D of one instance moves the offsets of every later one.  Bars: bitwise wherever two runs of the
batch are compared; 1e-9 relative against the CPU restatement (tests/helpers/warm_oracle.py) and against the fp64 handle, the bar
the batch's golden runs meet at set_expm(16, 1e-13); |Z_warm - Z_cold| <= 2 for the search, the spread DESIGN
section 12 records between the batch's two epilogues on identical probes."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden, relerr, state_from
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import warm_oracle  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph  # noqa: E402

pytestmark = pytest.mark.gpu

ETA = 0.05
Z1 = [int(load_golden("run_" + n)["Z"]) for n in ("env75", "er120", "dense60")] + [10]
Z2 = [Z1[0] + 1, Z1[1] - 1, Z1[2] + 1, Z1[3] - 1]  # D grows for some and shrinks for others
SEEDS = np.array([31, 32, 33, 34], dtype=np.uint64)
FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_EXPM_INFO,
          _lib.F_S_SUM, _lib.F_NORM_H, _lib.F_ST_DATA)
IFIELDS = (_lib.I_L_INDPTR, _lib.I_L_INDICES, _lib.I_ST_INDPTR, _lib.I_ST_INDICES, _lib.I_GAIN_X, _lib.I_GAIN_Y, _lib.I_ASSO_X, _lib.I_ASSO_Y,
           _lib.I_DIAG_POS, _lib.I_ASSO_POS)
KEPT = (_lib.F_E_ACCU, _lib.F_LVAL, _lib.F_XVAL, _lib.F_Y)


@functools.lru_cache(maxsize=None)
def four_states():
    return tuple(state_from(load_golden("run_" + n)) for n in ("env75", "er120", "dense60")) + (journal_graph(8, 75e-4, seed=2),)


def fields(b, i):
    out = [b.read(i, f) for f in FIELDS] + [b.read_i32(i, f) for f in IFIELDS]
    if b.iterations_done(i) > 0:
        out.append(b.read(i, _lib.F_SKETCH))
    return out


def same(b, i, ref, what):
    got = fields(b, i)
    assert len(got) == len(ref), what
    for n, (a, r) in enumerate(zip(got, ref)):
        assert a.shape == r.shape and np.array_equal(a, r), (what, "field %d" % n)


def sizes(b, i):
    return {k: b.sizes[i][k] for k in ("K", "Z", "D", "nnzL", "C")}


# ---- 1. the cold slot change is what it was: a fresh batch at those slot counts ---------------------------------------------------
@pytest.mark.parametrize("case", ["alone", "four", "one_out"])
def test_cold_set_slots_is_a_fresh_batch(case):
    pick = [3] if case == "alone" else [0, 1, 2, 3]
    states = [four_states()[i] for i in pick]
    za, zb, seeds = [Z1[i] for i in pick], [Z2[i] for i in pick], SEEDS[pick]
    out = 1 if case == "one_out" else None
    b = _lib.BatchSolver(za, states, 9, ETA)
    b.iterate(2, None, seeds)  # something to be thrown away
    give = list(zb)
    if out is not None:
        give[out] = 0
        zb[out] = za[out]  # it sits out at the slot count it had
    b.set_slots(give, 5)
    fresh = _lib.BatchSolver(zb, states, 5, ETA)
    for i in range(len(pick)):
        assert sizes(b, i) == sizes(fresh, i) and b.iterations_done(i) == 0, (case, i)
        same(b, i, fields(fresh, i), (case, i, "before"))
    before_out = fields(b, out) if out is not None else None
    b.iterate(3, None, seeds)
    fresh.iterate(3, None, seeds)
    for i in range(len(pick)):
        if i == out:
            assert b.iterations_done(i) == 0
            same(b, i, before_out, (case, i, "sitting out"))
        else:
            assert b.iterations_done(i) == 3
            same(b, i, fields(fresh, i), (case, i, "after"))
    b.close()
    fresh.close()


# ---- 2. the warm slot change keeps (e_accu, L, X, Y) and restarts the sums -----------------------------------------------------------
def test_warm_keeps_the_iterate_and_restarts_the_sums():
    states = list(four_states())
    b = _lib.BatchSolver(Z1, states, 6, ETA)
    b.iterate(6, None, SEEDS)
    kept = [[b.read(i, f) for f in KEPT] for i in range(4)]
    b.set_slots(Z2, 4, warm=True)
    for i in range(4):
        for f, r in zip(KEPT, kept[i]):
            assert np.array_equal(b.read(i, f), r), (i, f)
        for f in (_lib.F_XAVG, _lib.F_YAVG, _lib.F_E_THIS, _lib.F_XHALF, _lib.F_EXPM_INFO):
            assert not np.any(b.read(i, f)), (i, f)
        assert b.iterations_done(i) == 0
        assert (b.sizes[i]["Z"], b.sizes[i]["D"]) == (Z2[i], 2 * Z2[i])
        p = orc.Pattern(Z2[i], states[i])
        assert relerr(b.read(i, _lib.F_NORM_H), p.norm_H) < 1e-12
    b.iterate(4, None, SEEDS)
    for i in range(4):
        s = float(b.read(i, _lib.F_YAVG).sum())
        print("instance %d: sum of yavg after 4 warm iterations = %.15g" % (i, s))
        assert abs(s - 4.0) < 1e-9, (i, s)
        assert b.iterations_done(i) == 4
    with pytest.raises(_lib.MMWError):
        b.iterate(1, None, SEEDS)  # every instance has run the 4 it announced
    b.close()


# ---- 3. against the CPU restatement and the fp64 handle -------------------------------------------------------------------------------
def test_warm_follows_the_oracle_and_the_handle():
    states = list(four_states())
    n1, n2 = 5, 4
    rng = np.random.default_rng(7)
    Ks = [st[0].shape[0] for st in states]
    sk1 = [np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * z))) for _ in range(n1)]) for K, z in zip(Ks, Z1)]
    sk2 = [np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * z))) for _ in range(n2)]) for K, z in zip(Ks, Z2)]
    b = _lib.BatchSolver(Z1, states, n1, ETA)
    b.set_expm(16, 1e-13)
    b.iterate(n1, sk1)
    b.set_slots(Z2, n2, warm=True)
    b.iterate(n2, sk2)
    for i, st in enumerate(states):
        w = warm_oracle.run(Z1[i], n1, Z2[i], n2, st, ETA, lambda it, K, D: sk1[i][it], lambda it, K, D: sk2[i][it])
        got = {"lval": b.read(i, _lib.F_LVAL), "xval": b.read(i, _lib.F_XVAL), "Y": b.read(i, _lib.F_Y), "e_accu": b.read(i, _lib.F_E_ACCU),
               "xsum": b.read(i, _lib.F_XAVG), "ysum": b.read(i, _lib.F_YAVG)}
        errs = {k: relerr(got[k], w[k]) for k in got}
        print("instance %d vs warm oracle: %s" % (i, {k: "%.2e" % v for k, v in errs.items()}))
        h = _lib.Solver(Z1[i], st, n1, ETA, dtype=_lib.F64, device=0)
        h.set_expm(_lib.EXPM_TAYLOR, 16, 1e-13)
        h.iterate(n1, sk1[i])
        h.set_slots(Z2[i], n2, warm=True)
        h.iterate(n2, sk2[i])
        h.sync()
        herr = {"lval": relerr(got["lval"], h.read(_lib.F_LVAL)), "xval": relerr(got["xval"], h.read(_lib.F_XVAL)),
                "Y": relerr(got["Y"], h.read(_lib.F_Y)), "e_accu": relerr(got["e_accu"], h.read(_lib.F_E_ACCU)),
                "xsum/n": relerr(got["xsum"] / n2, h.read(_lib.F_XAVG) / n2), "ysum/n": relerr(got["ysum"] / n2, h.read(_lib.F_YAVG) / n2)}
        print("instance %d vs fp64 handle: %s" % (i, {k: "%.2e" % v for k, v in herr.items()}))
        h.close()
        for k, v in list(errs.items()) + list(herr.items()):
            assert v <= 1e-9, (i, k, v)
    b.close()


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------
def _alone(i, plan):
    """Instance i in a batch of one through `plan`: [(Z or None for the first leg, n), ...], every later leg warm."""
    a = _lib.BatchSolver([plan[0][0]], [four_states()[i]], plan[0][1], ETA)
    for leg, (z, n) in enumerate(plan):
        if leg:
            a.set_slots([z], n, warm=True)
        a.iterate(n, None, SEEDS[i:i + 1])
    out = fields(a, 0)
    a.close()
    return out


def test_a_warm_instance_is_the_same_alone_and_in_the_batch():
    b = _lib.BatchSolver(Z1, list(four_states()), 6, ETA)
    b.iterate(6, None, SEEDS)
    b.set_slots(Z2, 4, warm=True)
    b.iterate(4, None, SEEDS)
    for i in range(4):
        same(b, i, _alone(i, [(Z1[i], 6), (Z2[i], 4)]), i)
    b.close()


def test_a_neighbour_sitting_out_is_picked_up_warm_two_rounds_later():
    b = _lib.BatchSolver(Z1, list(four_states()), 3, ETA)
    b.iterate(3, None, SEEDS)
    Z3 = [Z2[0] + 2, 0, Z2[2] - 2, Z2[3] + 1]
    b.set_slots([Z2[0], 0, Z2[2], Z2[3]], 2, warm=True)  # instance 1 sits out; instance 0 grows, so 1's arrays move
    assert b.iterations_done(1) == 3
    b.iterate(2, None, SEEDS)
    b.set_slots(Z3, 2, warm=True)
    b.iterate(2, None, SEEDS)
    assert b.iterations_done(1) == 3
    same(b, 1, _alone(1, [(Z1[1], 3)]), "still the iterate it stopped at")
    Z4 = [Z3[0] - 1, Z2[1], Z3[2], Z3[3]]
    b.set_slots(Z4, 2, warm=True)
    b.iterate(2, None, SEEDS)
    same(b, 1, _alone(1, [(Z1[1], 3), (Z2[1], 2)]), "picked up")
    same(b, 0, _alone(0, [(Z1[0], 3), (Z2[0], 2), (Z3[0], 2), (Z4[0], 2)]), "the neighbour in front")
    same(b, 3, _alone(3, [(Z1[3], 3), (Z2[3], 2), (Z3[3], 2), (Z4[3], 2)]), "the neighbour behind")
    b.close()


# ---- 5. warm with nothing to continue from is cold --------------------------------------------------------------------------------------
def test_first_warm_call_is_a_cold_one():
    states = list(four_states())
    w = _lib.BatchSolver(Z1, states, 3, ETA)
    c = _lib.BatchSolver(Z1, states, 3, ETA)
    w.set_slots(Z2, 3, warm=True)
    c.set_slots(Z2, 3)
    for i in range(4):
        same(w, i, fields(c, i), (i, "before"))
    w.iterate(3, None, SEEDS)
    c.iterate(3, None, SEEDS)
    for i in range(4):
        same(w, i, fields(c, i), (i, "after"))
    w.close()
    c.close()


# ---- 6. with the splits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["split", "row_split", "both"])
def test_warm_run_is_bitwise_the_same_under_the_splits(which):
    ref = _alone(3, [(Z1[3], 4), (Z2[3], 3)])
    b = _lib.BatchSolver(Z1, list(four_states()), 4, ETA)
    if which in ("split", "both"):
        b.set_split([1, 1, 1, 2])
    if which in ("row_split", "both"):
        b.set_row_split([1, 1, 1, 2])
    b.iterate(4, None, SEEDS)
    b.set_slots(Z2, 3, warm=True)
    b.iterate(3, None, SEEDS)
    same(b, 3, ref, which)
    b.close()


# ---- 7. the search -------------------------------------------------------------------------------------------------------------------------
def feasible(state, z_vec, Z):
    """The check of tests/test_hip_handles.py: no slot overloads a member, no slot holds two users of one AP."""
    S, Q, h = state
    Sd = S.toarray()
    np.fill_diagonal(Sd, 0)
    for zz in range(Z):
        mem = np.where(z_vec == zz)[0]
        if mem.size and (np.any(Sd[np.ix_(mem, mem)].sum(axis=0) > h[mem] + 1e-12) or Q[np.ix_(mem, mem)].nnz):
            return False
    return True


@functools.lru_cache(maxsize=None)
def search_states():
    return tuple(journal_graph(c, 75e-4, seed=s) for c in (5, 6) for s in (0, 1))


@functools.lru_cache(maxsize=None)
def cold_search():
    return batch.search_many(list(search_states()), nit=60, epilogue="batch")


def test_cold_search_returns_what_the_parent_commit_returned():
    """Z, z_vec, probes and remainder of search_many(search_states(), nit=60, epilogue="batch") captured before the slot change moved
    to the device (tests/golden/batch_search_cold.npz)."""
    g = np.load(os.path.join(GOLDEN, "batch_search_cold.npz"), allow_pickle=False)
    for i, r in enumerate(cold_search()):
        assert int(r["Z"]) == int(g["Z"][i]) and int(r["remainder"]) == int(g["remainder"][i]), i
        assert [int(z) for z in r["probes"]] == [int(z) for z in g["probes_%d" % i]], i
        assert np.array_equal(np.asarray(r["z_vec"], dtype=np.int64), g["z_vec_%d" % i]), i
        assert r["iters"] == [60] * len(r["probes"]), i


def test_warm_search_ends_feasible_and_near_the_cold_one():
    states = list(search_states())
    tm = []
    warm = batch.search_many(states, nit=60, epilogue="batch", warm_start=True, timings=tm)
    cold = cold_search()
    for i, (w, c) in enumerate(zip(warm, cold)):
        print("instance %d: Z warm %d cold %d, probes warm %s cold %s" % (i, w["Z"], c["Z"], w["probes"], c["probes"]))
    for i, (w, c) in enumerate(zip(warm, cold)):
        assert w["remainder"] == 0 and feasible(states[i], w["z_vec"], int(w["Z"])), i
        assert w["iters"] == [60] + [20] * (len(w["probes"]) - 1), (i, w["iters"])
        assert abs(int(w["Z"]) - int(c["Z"])) <= 2, (i, w["Z"], c["Z"])
    assert all(t["set_slots_s"] >= 0.0 for t in tm) and len(tm) == max(len(w["probes"]) for w in warm)
