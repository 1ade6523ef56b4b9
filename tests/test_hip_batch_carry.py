"""GPU checks of the carry across states (mmw_batch_carry, csrc/kernels_batch_carry.h) and of the re-solve workflow built on it
(`batch.online_resolve_many`).

The state pairs are those of tests/test_batch_carry_host.py (tests/helpers/carry_oracle.py): (a) mobile_drop(5, 75e-4, 3) before and
after one second at 3 m/s, (b) the hand-made K = 4 pair whose L patterns share only the diagonal, (c) K = 2 losing / gaining its one
association pair, and the K = 192 instance journal_graph(8, 75e-4, seed=2) -- against itself at another Z, and moved like (a).
Bars: bitwise wherever two runs of the batch, or the batch and a gather, are compared; 1e-9 relative against the CPU restatement
(carry_oracle.run) at set_expm(16, 1e-13), the bar of tests/test_hip_batch_warm.py for the batch's golden and warm runs."""
import copy
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import carry_oracle  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import _NOISE_FLOOR_DBM, journal_graph, min_sinr_dec, mobile_drop  # noqa: E402

pytestmark = pytest.mark.gpu

ETA = 0.05
# the FIELDS / IFIELDS of tests/test_hip_batch_warm.py
FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_EXPM_INFO,
          _lib.F_S_SUM, _lib.F_NORM_H, _lib.F_ST_DATA)
IFIELDS = (_lib.I_L_INDPTR, _lib.I_L_INDICES, _lib.I_ST_INDPTR, _lib.I_ST_INDICES, _lib.I_GAIN_X, _lib.I_GAIN_Y, _lib.I_ASSO_X, _lib.I_ASSO_Y,
           _lib.I_DIAG_POS, _lib.I_ASSO_POS)
CARRIED = (_lib.F_LVAL, _lib.F_XVAL, _lib.F_E_ACCU, _lib.F_Y)
ZEROED = (_lib.F_XAVG, _lib.F_YAVG, _lib.F_E_THIS, _lib.F_XHALF, _lib.F_EXPM_INFO)


@functools.lru_cache(maxsize=None)
def pairs():
    """name -> (old state, new state, Z old, Z new)"""
    k192 = journal_graph(8, 75e-4, seed=2)
    return {"a": carry_oracle.moved_pair(5, carry_oracle.PAIR_A_SEED) + (6, 7), "b": carry_oracle.pair_b() + (2, 3),
            "c_lose": carry_oracle.pair_c("lose") + (2, 2), "c_gain": carry_oracle.pair_c("gain") + (2, 2), "k192_other_Z": (k192, k192, 10, 9),
            "k192_moved": carry_oracle.moved_pair(8, 2) + (10, 9)}


ALL = ("a", "b", "c_lose", "c_gain", "k192_other_Z", "k192_moved")


def make(names, side, nit, **kw):
    """A batch on the old (side 0) or the new (side 1) states of the named pairs."""
    return _lib.BatchSolver([pairs()[n][2 + side] for n in names], [pairs()[n][side] for n in names], nit, ETA, **kw)


def seeds_of(names):
    return np.array([41 + ALL.index(n) for n in names], dtype=np.uint64)


def fields(b, i):
    out = [b.read(i, f) for f in FIELDS] + [b.read_i32(i, f) for f in IFIELDS]
    if b.iterations_done(i) > 0:
        out.append(b.read(i, _lib.F_SKETCH))
    return out


def same(got, ref, what):
    assert len(got) == len(ref), what
    for n, (a, r) in enumerate(zip(got, ref)):
        assert a.shape == r.shape and np.array_equal(a, r), (what, "field %d" % n)


# ---- 1. what is written, and what is not ------------------------------------------------------------------------------------------------
def test_carried_fields_are_the_mapped_source_and_the_rest_is_untouched():
    names = ALL
    src = make(names, 0, 3)
    src.iterate(3, None, seeds_of(names))
    dst = make(names, 1, 4)
    dst.carry_from(src)
    for i, n in enumerate(names):
        old, new, zo, zn = pairs()[n]
        rl, rc = carry_oracle.maps(orc.Pattern(zo, old), orc.Pattern(zn, new))
        ml, mc = dst.carry_map(src, i)
        for f in CARRIED:
            got, have = dst.read(i, f), src.read(i, f)
            assert np.array_equal(got, carry_oracle.gather(have, rl if f in (_lib.F_LVAL, _lib.F_XVAL) else rc)), (n, f, "helper")
            assert np.array_equal(got, carry_oracle.gather(have, (ml if f in (_lib.F_LVAL, _lib.F_XVAL) else mc).astype(np.int64))), (n, f, "carry_map")
        assert np.any(dst.read(i, _lib.F_LVAL)) and np.any(dst.read(i, _lib.F_E_ACCU)), n  # (something was there to carry)
        for f in ZEROED:
            assert not np.any(dst.read(i, f)), (n, f)
        assert dst.iterations_done(i) == 0 and dst.nits[i] == 4
        diag = dst.read_i32(i, _lib.I_DIAG_POS)
        assert np.array_equal(dst.read(i, _lib.F_XVAL)[diag], src.read(i, _lib.F_XVAL)[src.read_i32(i, _lib.I_DIAG_POS)]), n
    dst.iterate(4, None, seeds_of(names))  # and it runs the iterations it announced, no more
    assert all(dst.iterations_done(i) == 4 for i in range(len(names)))
    with pytest.raises(_lib.MMWError):
        dst.iterate(1, None, seeds_of(names))
    src.close()
    dst.close()


# ---- 2. on identical states the carry is the warm slot change ------------------------------------------------------------------------
def test_carry_onto_the_same_states_is_the_warm_slot_change():
    names = ("a", "k192_other_Z", "b")
    st = [pairs()[n][0] for n in names]
    Z1, Z2 = [6, 10, 2], [7, 9, 3]
    a = _lib.BatchSolver(Z1, st, 4, ETA)
    a.iterate(4, None, seeds_of(names))
    c = _lib.BatchSolver(Z2, st, 3, ETA)
    c.carry_from(a)
    a.set_slots(Z2, 3, warm=True)
    for i in range(len(names)):
        same(fields(c, i), fields(a, i), (names[i], "before"))
    a.iterate(3, None, seeds_of(names))
    c.iterate(3, None, seeds_of(names))
    for i in range(len(names)):
        same(fields(c, i), fields(a, i), (names[i], "after"))
    a.close()
    c.close()


# ---- 3. across states against the CPU restatement ---------------------------------------------------------------------------------------
def test_carry_across_states_follows_the_oracle():
    names = ("a", "k192_moved")
    n1, n2 = 5, 4
    rng = np.random.default_rng(11)
    Ks = [pairs()[n][0][0].shape[0] for n in names]
    sk1 = [np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * pairs()[n][2]))) for _ in range(n1)]) for K, n in zip(Ks, names)]
    sk2 = [np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * pairs()[n][3]))) for _ in range(n2)]) for K, n in zip(Ks, names)]
    src = make(names, 0, n1)
    src.set_expm(16, 1e-13)
    src.iterate(n1, sk1)
    dst = make(names, 1, n2)
    dst.set_expm(16, 1e-13)
    dst.carry_from(src)
    dst.iterate(n2, sk2)
    worst = {}
    for i, n in enumerate(names):
        old, new, zo, zn = pairs()[n]
        w = carry_oracle.run(zo, n1, old, zn, n2, new, ETA, lambda it, K, D: sk1[i][it], lambda it, K, D: sk2[i][it])
        got = {"lval": dst.read(i, _lib.F_LVAL), "xval": dst.read(i, _lib.F_XVAL), "Y": dst.read(i, _lib.F_Y), "e_accu": dst.read(i, _lib.F_E_ACCU),
               "xsum": dst.read(i, _lib.F_XAVG), "ysum": dst.read(i, _lib.F_YAVG)}
        errs = {k: relerr(got[k], w[k]) for k in got}
        print("%s vs carry oracle: %s" % (n, {k: "%.2e" % v for k, v in errs.items()}))
        worst.update({(n, k): v for k, v in errs.items()})
    for key, v in worst.items():
        assert v <= 1e-9, (key, v)
    src.close()
    dst.close()


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------
def test_an_instance_carries_the_same_alone_among_neighbours_and_under_take():
    def carried(names, take=None, sit_out=None, n_src=3, n_dst=2):
        src = make(names, 0, n_src)
        if sit_out is not None:  # that instance of the source never iterates
            z = [pairs()[n][2] for n in names]
            z[sit_out] = 0
            src.set_slots(z, n_src)
        src.iterate(n_src, None, seeds_of(names))
        dst = make(names, 1, n_dst)
        dst.carry_from(src, take)
        before = [fields(dst, i) for i in range(len(names))]
        dst.iterate(n_dst, None, seeds_of(names))
        after = [fields(dst, i) for i in range(len(names))]
        src.close()
        dst.close()
        return before, after

    group = ("b", "a", "k192_moved", "c_gain")
    alone = carried(("a",))
    among = carried(group)
    taken = carried(group, take=[0, 1, 0, 0])
    for leg in (0, 1):
        same(among[leg][1], alone[leg][0], ("among neighbours", leg))
        same(taken[leg][1], alone[leg][0], ("under take", leg))
    # a skipped instance, and one whose source never iterated, are a fresh batch
    fresh = make(group, 1, 2)
    f0 = [fields(fresh, i) for i in range(len(group))]
    fresh.iterate(2, None, seeds_of(group))
    f1 = [fields(fresh, i) for i in range(len(group))]
    fresh.close()
    never = carried(group, sit_out=2)
    for leg, ref in ((0, f0), (1, f1)):
        for i in (0, 2, 3):
            same(taken[leg][i], ref[i], ("skipped", group[i], leg))
        same(never[leg][2], ref[2], ("source never iterated", leg))
        same(never[leg][1], among[leg][1], ("beside it", leg))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(status, text, call):
    with pytest.raises(_lib.MMWError, match=text) as e:
        call()
    assert ("status %d:" % status) in str(e.value), str(e.value)


def test_refusals_leave_both_batches_unchanged():
    names = ("a", "b")
    src = make(names, 0, 3)
    src.iterate(2, None, seeds_of(names))
    dst = make(names, 1, 3)
    other_k = make(("a", "c_gain"), 1, 3)  # instance 1 has K = 2, the source's K = 4
    three = make(("a", "b", "b"), 1, 3)
    host = make(names, 0, 3, device=-1)
    ran = make(names, 1, 3)
    ran.iterate(1, None, seeds_of(names))
    view = lambda b: [fields(b, i) for i in range(b.B)]  # noqa: E731
    vs, vd, vo, vt, vr = view(src), view(dst), view(other_k), view(three), view(ran)
    refused(-1, "cannot carry from itself", lambda: dst.carry_from(dst))
    refused(-3, "host-only", lambda: dst.carry_from(host))
    refused(-3, "host-only", lambda: host.carry_from(src))
    refused(-1, "holds 2 instances, this batch 3", lambda: three.carry_from(src))
    refused(-1, "instance 1: K = 2 here, K = 4 in the source", lambda: other_k.carry_from(src))
    refused(-1, "instance 1: K = 2 here, K = 4 in the source", lambda: other_k.carry_from(src, take=[1, 1]))
    refused(-3, "instance 0 has run 1 iterations", lambda: ran.carry_from(src))
    refused(-3, "instance 1 has run 1 iterations", lambda: ran.carry_from(src, take=[0, 1]))
    for b, v, done in ((src, vs, 2), (dst, vd, 0), (other_k, vo, 0), (three, vt, 0), (ran, vr, 1)):
        for i in range(b.B):
            same(fields(b, i), v[i], "after the refusals")
            assert b.iterations_done(i) == done
    other_k.carry_from(src, take=[1, 0])  # the mismatch is the skipped instance's: served
    same(fields(other_k, 1), vo[1], "the skipped instance")
    dst.carry_from(src)
    for f in CARRIED:
        assert np.array_equal(other_k.read(0, f), dst.read(0, f)), f
    for b in (src, dst, other_k, three, host, ran):
        b.close()


# ---- 6. the workflow ---------------------------------------------------------------------------------------------------------------------
KW = dict(nit=20, eta=ETA, seed=5, nattempt=10)
NPTS, STEP, SPD = 3, 1e6, 3.0


def two_drops():
    return [mobile_drop(5, 75e-4, s) for s in (3, 4)]


@functools.lru_cache(maxsize=None)
def resolved(carry):
    tm = []
    drops = two_drops()
    return batch.online_resolve_many(drops, n_points=NPTS, step_us=STEP, mob_spd_meter_s=SPD, carry=carry, timings=tm, **KW), tm, drops


@pytest.mark.parametrize("carry", [True, False])
def test_online_resolve_many_is_the_same_steps_done_by_hand(carry):
    res, tm, walked = resolved(carry)
    n_p = 7 if carry else 20  # warm_iterations(20, 1 / 3) = 7
    hand = two_drops()
    B = len(hand)
    states = [d.state() for d in hand]
    found = batch.search_many(states, epilogue="batch", **KW)
    Zs = [r["Z"] for r in found]
    prev = _lib.BatchSolver(Zs, states, KW["nit"], ETA)
    prev.iterate(KW["nit"], None, np.array([batch.probe_seed(5, i, len(found[i]["probes"])) for i in range(B)], dtype=np.uint64))
    prev.factor()
    env = _lib.BatchEnv([d.ap_locs for d in hand], [d.K for d in hand], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)
    for p in range(NPTS):
        env.move([d.sta_locs for d in hand])
        seeds = np.array([batch.probe_seed(5, i, 0x80000 | p) for i in range(B)], dtype=np.uint64)
        if p == 0:
            z, rem, used = prev.round_env(env, 10, seeds)
        else:
            b = _lib.BatchSolver(Zs, [env.state(i) for i in range(B)], n_p, ETA)
            if carry:
                b.carry_from(prev)
            b.iterate(n_p, None, np.array([batch.probe_seed(5, i, 0xC0000 | p) for i in range(B)], dtype=np.uint64))
            b.factor()
            z, rem, used = b.round(10, seeds)
            prev.close()
            prev = b
        fin = [batch._finish(z, rem, used, i, Zs[i], int(seeds[i])) for i in range(B)]
        _, bler = env.evaluate([f[0] for f in fin], Zs)
        for i in range(B):
            assert np.array_equal(res[i]["z_vec"][p], fin[i][0]) and res[i]["remainder"][p] == fin[i][2], (p, i)
            assert np.array_equal(res[i]["bler"][p], bler[i]), (p, i)
        for d in hand:
            d.step_time(STEP, SPD)
    env.close()
    prev.close()
    for i in range(B):
        assert res[i]["Z"] == Zs[i] and res[i]["probes"] == found[i]["probes"] and res[i]["iters"] == [20] + [n_p] * (NPTS - 1), i
    assert all(np.array_equal(d.sta_locs, h.sta_locs) for d, h in zip(walked, hand))
    assert len(tm) == NPTS and all(set(t) == {"create_s", "carry_s", "iterate_s", "epilogue_s", "evaluate_s", "step_s"} for t in tm)
    assert all(v >= 0.0 for t in tm for v in t.values())


def test_point_zero_is_online_manys():
    res = resolved(True)[0]
    ref = batch.online_many(two_drops(), n_points=1, step_us=STEP, mob_spd_meter_s=SPD, **KW)
    for i in range(2):
        assert res[i]["Z"] == ref[i]["Z"] and res[i]["probes"] == ref[i]["probes"]
        assert np.array_equal(res[i]["z_vec"][0], ref[i]["z_vec"][0]) and res[i]["remainder"][0] == ref[i]["remainder"][0]
        assert np.array_equal(res[i]["bler"][0], ref[i]["bler"][0])


def test_a_drop_gives_the_same_alone_and_in_a_batch_of_two():
    """The seeds are keyed by the instance's index, so each drop is compared at index 0: alone, and in front of the other one."""
    run = lambda drops: batch.online_resolve_many(drops, n_points=NPTS, step_us=STEP, mob_spd_meter_s=SPD, carry=True, **KW)  # noqa: E731
    d = two_drops()
    for first, pair in ((0, resolved(True)[0]), (1, run([copy.deepcopy(d[1]), copy.deepcopy(d[0])]))):
        alone = run([copy.deepcopy(d[first])])[0]
        for key in ("z_vec", "remainder", "bler"):
            assert np.array_equal(alone[key], pair[0][key]), (first, key)
        assert alone["Z"] == pair[0]["Z"] and alone["probes"] == pair[0]["probes"] and alone["iters"] == pair[0]["iters"]


def test_over_the_epilogue_limit_is_refused_by_name():
    class Big:
        K = _lib.BATCH_EPILOGUE_MAX_K + 1
    with pytest.raises(ValueError, match="instance 1 has K = 1025"):
        batch.online_resolve_many([two_drops()[0], Big()], n_points=1)
