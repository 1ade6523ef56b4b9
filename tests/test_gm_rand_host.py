"""Host side of MAX_RAND with its draws on the device (mmw_gm_rand, mmw_gm_rand_draw, mmw_batch_gm_rand; no GPU): everything a
device = -1 handle and a host-only batch can reach, which is the whole procedure as plain C++ with the draw through the host form of
the same functions.

The comparator is never the code under test: the draw is `gm_rand_cases.draw` (a NumPy restatement of the rule in include/mmw_hip.h
on `philox_ref`'s Philox), the greedy is the reference's own (`gm_restate.max_rand`, gm.py:152-199) fed the order and preference that
NumPy forms from that draw.  Draws are compared bit for bit, slots and counts as integers.  The restatement's ln / cos / sin are held
to `math`'s (ln within 2 ulp, the sine and cosine within 1e-15: their reference angle 2 pi u is itself rounded), so it evaluates
Box-Muller and not something else.
"""
import ctypes as C
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import gm_rand_cases as GR  # noqa: E402
import gm_restate as R  # noqa: E402
import philox_ref as pr  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch, gm, online  # noqa: E402

ARG, STATE = -1, -3  # MMW_ERR_ARG, MMW_ERR_STATE
DECLARATIONS = (
    "int mmw_gm_rand(mmw_gm* g, int32_t Z, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out, int32_t* rem_out, int32_t* pick_out);",
    "int mmw_gm_rand_draw(mmw_gm* g, int32_t Z, uint64_t seed, int32_t attempt, double* pref_val_out, double* order_key_out);",
    "int mmw_batch_gm_rand(mmw_batch* b, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds, "
    "int32_t* z_out, int32_t* rem_out, int32_t* used_out);",
    "int mmw_batch_env_gm_rand(mmw_batch_env* e, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, "
    "const uint64_t* seeds, int32_t* z_out, int32_t* rem_out, int32_t* used_out);",
)


def last_error():
    return _lib.lib().mmw_last_error().decode()


@pytest.fixture(scope="module")
def handles():
    hs = {}

    def get(name):
        if name not in hs:
            hs[name] = _lib.GreedyHandle(GR.state(name), device=-1)
        return hs[name]
    yield get
    for h in hs.values():
        h.close()


# ---- 1. the draw ---------------------------------------------------------------------------------------------------------------------
def test_the_restatement_evaluates_box_muller():
    """ln, cos and sin by the header's fixed sequences against `math`'s, on the uniforms of 20 000 draws: the normals differ from the
    library evaluation by a few ulp of their scale, and Box-Muller's pair has the moments of a normal."""
    w = pr.philox4x32_10(np.arange(200)[:, None], np.arange(100)[None, :], 1, GR.TAG_PREF, 7, 9)
    u1, u2 = GR.uniforms(w)
    ln = GR.ln_fixed(u1)
    ref = np.array([math.log(x) for x in u1.ravel()]).reshape(u1.shape)
    ulp = np.max(np.abs(ln - ref) / np.spacing(np.abs(ref)))
    c, s = GR.cos_sin_fixed(u2)
    # the reference angle 2 pi u2 is itself rounded (an error up to 2 pi 2^-53 in the angle), so the bar is absolute
    ec = max(abs(a - math.cos(2.0 * math.pi * x)) for a, x in zip(c.ravel(), u2.ravel()))
    es = max(abs(a - math.sin(2.0 * math.pi * x)) for a, x in zip(s.ravel(), u2.ravel()))
    n = GR.normals(w)
    print("[gm-rand] ln: %.2f ulp; cos %.2e, sin %.2e absolute; mean %.4f, variance %.4f" % (ulp, ec, es, n.mean(), n.var()))
    assert ulp <= 2.0 and ec <= 1e-15 and es <= 1e-15
    assert abs(n.mean()) < 0.02 and abs(n.var() - 1.0) < 0.03 and np.max(np.abs(n - pr.normals_f64(w))) < 1e-14


@pytest.mark.parametrize("K,Z", GR.DRAW_SHAPES)
def test_draw_is_the_restatement_bit_for_bit(handles, K, Z):
    g = handles(GR.STATE_OF_K[K])
    assert g.K == K
    for seed in GR.DRAW_SEEDS:
        for a in GR.DRAW_ATTEMPTS:
            pv, key = g.rand_draw(Z, seed, a)
            rv, rk = GR.draw(K, Z, seed, a)
            assert pv.shape == (K, Z) and pv.tobytes() == rv.tobytes() and key.tobytes() == rk.tobytes(), (seed, a)
    if Z % 2:  # the discarded half pair: an odd Z is the even one without its last column
        wide = g.rand_draw(Z + 1, GR.DRAW_SEEDS[0], 0)[0]
        assert g.rand_draw(Z, GR.DRAW_SEEDS[0], 0)[0].tobytes() == np.ascontiguousarray(wide[:, :Z]).tobytes()
    lo = g.rand_draw(Z, GR.DRAW_SEEDS[1] & 0xFFFFFFFF, 0)[0]  # the key's upper word counts
    assert lo.tobytes() != g.rand_draw(Z, GR.DRAW_SEEDS[1], 0)[0].tobytes()


def test_draw_pieces_may_be_left_out(handles):
    g = handles("er65")
    pv, key = g.rand_draw(7, 3, 2)
    only_pv, only_key = np.empty_like(pv), np.empty_like(key)
    L = _lib.lib()
    assert L.mmw_gm_rand_draw(g._h, 7, 3, 2, _lib._pd(only_pv), None) == 0 and only_pv.tobytes() == pv.tobytes()
    assert L.mmw_gm_rand_draw(g._h, 7, 3, 2, None, _lib._pd(only_key)) == 0 and only_key.tobytes() == key.tobytes()


# ---- 2. the slots --------------------------------------------------------------------------------------------------------------------
SLOT_CASES = [("one_ap", 1), ("one_ap", 2), ("one_ap", 3), ("env75", 3), ("env75", 12), ("er64", 2), ("er65", 9), ("j8", 7), ("j8", 14)]


@pytest.mark.parametrize("name,Z", SLOT_CASES)
def test_slots_are_the_reference_greedy_on_the_restated_draw(handles, name, Z):
    g, st = handles(name), GR.state(name)
    natt, seed = 3, GR.DRAW_SEEDS[1]
    want, rem_want = GR.reference(Z, st, seed, natt)
    for rule, pick in ((0, "first"), (1, "fewest")):
        z, rem, got = g.rand(Z, natt, seed, pick)
        assert rem.tolist() == rem_want and got == GR.pick_of(rem_want, rule), (rule, rem.tolist(), rem_want)
        assert np.array_equal(z, want[got]) and int(np.sum(z < 0)) == rem[got]
        R.check_slots(st, z, z >= 0)
    one = g.rand(Z, 1, seed)  # attempt 0 does not depend on how many follow
    assert np.array_equal(one[0], want[0]) and one[1].tolist() == rem_want[:1] and one[2] == 0


def test_feasible_and_infeasible_slot_counts_are_both_covered(handles):
    rems = {c: GR.reference(c[1], GR.state(c[0]), GR.DRAW_SEEDS[1], 3)[1] for c in SLOT_CASES}
    assert rems[("one_ap", 1)] == [1, 1, 1] and rems[("one_ap", 2)] == [0, 0, 0]  # two users behind one access point
    assert any(min(r) > 0 for r in rems.values()) and any(max(r) == 0 for r in rems.values())


def test_both_pick_rules_where_an_attempt_fails_and_a_later_one_succeeds(handles):
    """The (Z, seed) is found by the restatement alone: the reference's greedy leaves somebody over in attempt 0 and nobody in a later
    one.  Rule 0 then returns that later attempt, rule 1 the same (0 users over is the fewest); one slot fewer, where every attempt
    fails, separates the rules."""
    st, g, natt = GR.state("env75"), handles("env75"), 4
    found = None
    for Z in range(8, 14):
        for seed in range(1, 9):
            rem = GR.reference(Z, st, seed, natt)[1]
            if rem[0] > 0 and 0 in rem[1:]:
                found = (Z, seed, rem)
                break
        if found:
            break
    assert found, "no slot count shows the pattern"
    Z, seed, rem_want = found
    want = GR.reference(Z, st, seed, natt)[0]
    first = rem_want.index(0)
    for pick in ("first", "fewest"):
        z, rem, got = g.rand(Z, natt, seed, pick)
        assert rem.tolist() == rem_want and got == first and np.array_equal(z, want[first]) and np.all(z >= 0)
    tight = next(z for z in range(Z - 1, 1, -1) if min(GR.reference(z, st, seed, natt)[1]) > 0)
    want, rem_want = GR.reference(tight, st, seed, natt)
    z0, rem0, p0 = g.rand(tight, natt, seed, "first")
    z1, rem1, p1 = g.rand(tight, natt, seed, "fewest")
    assert rem0.tolist() == rem1.tolist() == rem_want and p0 == natt - 1 and p1 == int(np.argmin(rem_want))
    assert np.array_equal(z0, want[p0]) and np.array_equal(z1, want[p1])


def test_the_widest_slot_count_is_accepted(handles):
    g = handles("one_ap")
    z, rem, got = g.rand(4800, 1, 1)
    assert rem.tolist() == [0] and got == 0 and np.array_equal(z, GR.reference(4800, GR.state("one_ap"), 1, 1)[0][0])


# ---- 3. the host-only batch ----------------------------------------------------------------------------------------------------------
BATCH_NAMES = ["one_ap", "er64", "er65", "j8", "env75", "j5", "er120"]
BATCH_Z = [2, 4, 9, 7, 10, 6, 5]
BATCH_SEEDS = [11, 12, GR.DRAW_SEEDS[1], 14, 15, 16, 17]


@pytest.fixture(scope="module")
def hb():
    b = _lib.BatchSolver([4] * len(BATCH_NAMES), [GR.state(n) for n in BATCH_NAMES], 1, 0.04, device=-1)
    yield b
    b.close()


def test_batch_instance_alone_among_neighbours_under_take_and_on_the_handle(handles, hb):
    natt = 3
    z, rem, used = hb.gm_rand(BATCH_Z, BATCH_SEEDS, natt, stop_at_first=False)
    assert used.tolist() == [natt] * hb.B
    for i, name in enumerate(BATCH_NAMES):
        want, rem_want = GR.reference(BATCH_Z[i], GR.state(name), BATCH_SEEDS[i], natt)
        assert np.array_equal(z[i], want) and rem[i].tolist() == rem_want, name
        zh, remh, ph = handles(name).rand(BATCH_Z[i], natt, BATCH_SEEDS[i])
        assert remh.tolist() == rem_want and np.array_equal(zh, z[i][ph]), name
    i = 4  # one instance alone, and under a partial take
    one = _lib.BatchSolver([4], [GR.state(BATCH_NAMES[i])], 1, 0.04, device=-1)
    z1, rem1, used1 = one.gm_rand([BATCH_Z[i]], [BATCH_SEEDS[i]], natt, stop_at_first=False)
    one.close()
    assert z1[0].tobytes() == z[i].tobytes() and rem1[0].tolist() == rem[i].tolist() and used1[0] == natt
    take = [False, True, False, False, True, False, True]
    zt, remt, usedt = hb.gm_rand(BATCH_Z, BATCH_SEEDS, natt, take=take, stop_at_first=False)
    for j in range(hb.B):
        if take[j]:
            assert zt[j].tobytes() == z[j].tobytes() and remt[j].tolist() == rem[j].tolist() and usedt[j] == natt
        else:
            assert zt[j] is None and remt[j].tolist() == [-1] * natt and usedt[j] == 0


def test_batch_stops_at_the_first_attempt_that_leaves_nobody_over(hb):
    natt = 4
    z, rem, used = hb.gm_rand(BATCH_Z, BATCH_SEEDS, natt, stop_at_first=False)
    zs, rems, useds = hb.gm_rand(BATCH_Z, BATCH_SEEDS, natt, stop_at_first=True)
    assert any(u < natt for u in useds) and any(u == natt for u in useds)  # both happen in this batch
    for i in range(hb.B):
        full = rem[i].tolist()
        u = full.index(0) + 1 if 0 in full else natt
        assert useds[i] == u and rems[i].tolist() == full[:u] + [-1] * (natt - u)
        assert np.array_equal(zs[i][:u], z[i][:u]) and np.all(zs[i][u:] == -2)


def test_batch_leaves_out_an_instance_without_a_slot_count(hb):
    Zs = list(BATCH_Z)
    Zs[1], Zs[3] = 0, -1
    z, rem, used = hb.gm_rand(Zs, BATCH_SEEDS, 2, stop_at_first=False)
    ref = hb.gm_rand(BATCH_Z, BATCH_SEEDS, 2, stop_at_first=False)
    for i in range(hb.B):
        if i in (1, 3):
            assert z[i] is None and rem[i].tolist() == [-1, -1] and used[i] == 0
        else:
            assert z[i].tobytes() == ref[0][i].tobytes() and rem[i].tolist() == ref[1][i].tolist()


def raw_batch(b, take, Zs, natt, seeds, n, nulls=()):
    z = np.full(n, -7, dtype=np.int32)
    rem = np.full(b.B * max(natt, 1), -7, dtype=np.int32)
    used = np.full(b.B, -7, dtype=np.int32)
    t = None if take is None else _lib._i32(take)
    sd = _lib._u64(seeds, b.B)
    args = {"take": _lib._opt_pi(t), "Z": _lib._pi(_lib._i32(Zs)), "seeds": _lib._pu(sd), "z": _lib._pi(z), "rem": _lib._pi(rem), "used": _lib._pi(used)}
    for k in nulls:
        args[k] = None
    rc = _lib.lib().mmw_batch_gm_rand(b._h, args["take"], args["Z"], natt, 0, args["seeds"], args["z"], args["rem"], args["used"])
    return rc, z, rem, used


def untouched(r):
    return all(np.all(a == -7) for a in r[1:])


def test_batch_limits_and_refusals():
    big = _lib.BatchSolver([4], [GR.state("k1024")], 1, 0.04, device=-1)
    assert big.sizes[0]["K"] == 1024
    z, rem, used = big.gm_rand([6], [3], 1)
    want, rem_want = GR.reference(6, GR.state("k1024"), 3, 1)
    assert np.array_equal(z[0], want) and rem[0].tolist() == rem_want
    for Zs, word in (([1025], "Z = 1025"),):
        r = raw_batch(big, None, Zs, 1, 3, 1024)
        assert r[0] == ARG and untouched(r) and "instance 0" in last_error() and word in last_error(), last_error()
    big.close()
    over = _lib.BatchSolver([4, 4], [GR.state("one_ap"), GR.state("er1025")], 1, 0.04, device=-1)
    r = raw_batch(over, None, [2, 4], 1, 3, 1027)
    assert r[0] == ARG and untouched(r) and "instance 1" in last_error() and "K = 1025" in last_error() and "1024" in last_error(), last_error()
    r = raw_batch(over, [1, 0], [2, 4], 1, 3, 2)  # only an instance that takes part is refused
    assert r[0] == 0 and sorted(r[1].tolist()) == [0, 1] and r[3].tolist() == [1, 0]
    r = raw_batch(over, None, [2, 0], 1, 3, 2)  # and one without a slot count does not take part
    assert r[0] == 0 and r[3].tolist() == [1, 0]
    for kw, word in ((dict(natt=0), "nattempt = 0"), (dict(natt=4097), "nattempt = 4097"), (dict(take=[0, 0]), "no instance takes part"),
                     (dict(Zs=[0, 0]), "no instance takes part"), (dict(nulls=("Z",)), "null"), (dict(nulls=("seeds",)), "null"),
                     (dict(nulls=("z",)), "null"), (dict(nulls=("rem",)), "null"), (dict(nulls=("used",)), "null")):
        a = dict(take=[1, 0], Zs=[2, 4], natt=1, nulls=())
        a.update(kw)
        r = raw_batch(over, a["take"], a["Zs"], a["natt"], 3, 8, a["nulls"])
        assert r[0] == ARG and untouched(r) and word in last_error() and "mmw_batch_gm_rand" in last_error(), (kw, last_error())
    over.close()


# ---- 4. the handle's refusals --------------------------------------------------------------------------------------------------------
def test_handle_refusals_name_the_value_and_leave_the_outputs_untouched(handles):
    g = handles("one_ap")
    L = _lib.lib()

    def raw(Z, natt, rule, nulls=()):
        z, rem, got = np.full(2, -7, dtype=np.int32), np.full(300, -7, dtype=np.int32), C.c_int32(-7)
        p = {"z": _lib._pi(z), "rem": _lib._pi(rem), "pick": C.byref(got)}
        for k in nulls:
            p[k] = None
        rc = L.mmw_gm_rand(g._h, Z, natt, 5, rule, p["z"], p["rem"], p["pick"])
        return rc, np.all(z == -7) and np.all(rem == -7) and got.value == -7

    for args, word in (((0, 1, 0), "Z = 0"), ((-3, 1, 0), "Z = -3"), ((2, 0, 0), "nattempt = 0"), ((2, 257, 0), "nattempt = 257"),
                       ((2, 1, 2), "pick_rule = 2"), ((2, 1, -1), "pick_rule = -1"), ((4801, 1, 0), "Z = 4801")):
        rc, clean = raw(*args)
        assert rc == ARG and clean and word in last_error() and "mmw_gm_rand" in last_error(), (args, last_error())
    for nulls in (("z",), ("rem",), ("pick",)):
        rc, clean = raw(2, 1, 0, nulls)
        assert rc == ARG and clean and "null" in last_error(), nulls
    assert L.mmw_gm_rand(None, 2, 1, 5, 0, None, None, None) == ARG and "null" in last_error()
    pv = np.full(4, -7.0)
    for Z, a, word in ((0, 0, "Z = 0"), (2, -1, "attempt = -1"), (4801, 0, "Z = 4801")):
        assert L.mmw_gm_rand_draw(g._h, Z, 5, a, _lib._pd(pv), None) == ARG and word in last_error() and np.all(pv == -7.0), last_error()
    assert raw(2, 256, 1)[0] == 0  # the bounds themselves are accepted
    with pytest.raises(ValueError, match="'best'"):
        g.rand(2, 1, 5, pick="best")


# ---- 5. gm.MAX_RAND.run ---------------------------------------------------------------------------------------------------------------
def same_stream(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_max_rand_device_draws_are_reproducible_and_take_one_integer():
    st = GR.state("env75")
    K = st[0].shape[0]
    np.random.seed(42)
    a = gm.MAX_RAND.run(20, st, device=-1, draws="device")
    after = np.random.get_state()
    np.random.seed(42)
    b = gm.MAX_RAND.run(20, st, device=-1, draws="device")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert a[0].dtype == np.float64 and a[0].shape == (K,) and a[1] == 20 and int(a[2]) == 0  # the reference's triple
    np.random.seed(42)
    key = int(np.random.randint(0, 1 << 64, dtype=np.uint64))
    assert same_stream(np.random.get_state(), after)  # nobody left over: that one integer is all it took
    want = GR.reference(20, st, key, 1)[0][0]
    assert np.array_equal(a[0], want)
    # users left over: the fill is the host's randint, right after that integer
    np.random.seed(7)
    z, Z, rem = gm.MAX_RAND.run(3, st, device=-1, draws="device")
    after = np.random.get_state()
    np.random.seed(7)
    key = int(np.random.randint(0, 1 << 64, dtype=np.uint64))
    want, rem_want = GR.reference(3, st, key, 1)
    fill = np.random.randint(3, size=rem_want[0])
    assert same_stream(np.random.get_state(), after) and rem == rem_want[0] > 0 and Z == 3
    assert np.array_equal(z[want[0] >= 0], want[0][want[0] >= 0]) and np.array_equal(z[want[0] < 0], fill)
    # an explicit seed takes nothing from the stream
    np.random.seed(1)
    before = np.random.get_state()
    z2 = gm.MAX_RAND.run(20, st, device=-1, draws="device", seed=key, nattempt=2)
    assert same_stream(np.random.get_state(), before) and np.all(z2[0] >= 0)


def test_max_rand_host_draws_are_the_reference_expressions():
    st = GR.state("env75")
    K = st[0].shape[0]
    for Z in (3, 12):
        np.random.seed(99)
        got = gm.MAX_RAND.run(Z, st, device=-1)
        np.random.seed(99)
        inprod = np.random.randn(Z, K)  # gm.py:148-150
        sorted_indices = np.argsort(-inprod, axis=0)
        rank = np.argsort(np.random.randn(K))
        want = R.max_rand(Z, st, rank, sorted_indices.T)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and int(got[2]) == want[2]
    sig = inspect.signature(gm.MAX_RAND.run).parameters
    assert list(sig) == ["Z", "state", "nattempt", "device", "draws", "seed"] and sig["draws"].default == "host" and sig["seed"].default is None


def test_max_rand_refuses_an_unknown_draws_value():
    with pytest.raises(ValueError, match="'gpu'"):
        gm.MAX_RAND.run(3, GR.state("one_ap"), device=-1, draws="gpu")


# ---- 6. "mrand" in the sweeps ---------------------------------------------------------------------------------------------------------
class Reached(Exception):
    pass


def test_mrand_is_accepted_where_documented_and_the_defaults_stand(hb, monkeypatch):
    assert batch.METHODS == ("rand", "mgain", "masso") and batch.OPT_IN_METHODS == ("spectral",) and online.METHODS == batch.METHODS
    assert batch.ALL_METHODS == ("rand", "mgain", "masso", "spectral", "mrand")
    for fn in (batch.baselines_many, batch.compare_many, online.compare):
        assert inspect.signature(fn).parameters["methods"].default == batch.METHODS, fn.__name__
    assert inspect.signature(batch.online_greedy_many).parameters["methods"].default == ("mgain",)
    # baselines_many runs it on a host-only batch: the key scheme's index is 4, the first feasible attempt counts
    out = batch.baselines_many(hb, BATCH_Z, methods=("mrand",), seed=5, nattempt_gm=3)
    for i, name in enumerate(BATCH_NAMES):
        key = batch.probe_seed(5, i, 0x40000 | 4)
        want, rem_want = GR.reference(BATCH_Z[i], GR.state(name), key, 3)
        a = GR.pick_of(rem_want, 0)
        z_vec, Z, rem = out[i]["mrand"]
        assert list(out[i]) == ["mrand"] and Z == BATCH_Z[i] and rem == rem_want[a]
        assert np.array_equal(z_vec[want[a] >= 0], want[a][want[a] >= 0]) and np.all((z_vec >= 0) & (z_vec < Z))

    # the entries that need a device: the name passes their checks (the first device object is reached), another name does not
    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(batch._lib, "BatchEnv", reached)
    monkeypatch.setattr(online, "_env", reached)
    geo = (np.array([[3.0, 4.0], [15.5, 12.25]]), np.array([[10.0, 10.0]]))
    with pytest.raises(Reached):
        batch.compare_many([geo], methods=("mrand",))
    with pytest.raises(Reached):
        online.compare(geo, methods=("mgain", "mrand"))
    for call in (lambda: batch.compare_many([geo], methods=("mrand", "lrp")), lambda: online.compare(geo, methods=("lrp",)),
                 lambda: batch.baselines_many(hb, BATCH_Z, methods=("lrp",)), lambda: batch.online_greedy_many([], methods=("mgain", "lrp"))):
        with pytest.raises(ValueError, match="got 'lrp'"):
            call()
    with pytest.raises(ValueError, match="must name 'mgain'"):
        batch.online_greedy_many([], methods=("mrand",))


# ---- 7. the symbols -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_documented_exported_and_bound():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmw_hip.h")).read())
    for d in DECLARATIONS:
        assert d in txt, d
    assert txt.index("int mmw_gm_assign(") < txt.index("int mmw_gm_rand(") < txt.index("int mmw_gm_rand_draw(") < txt.index("int mmw_batch_create(")
    assert txt.index("int mmw_batch_gm(") < txt.index("int mmw_batch_gm_rand(") < txt.index("int mmw_batch_env_gm(") < txt.index("int mmw_batch_env_gm_rand(")
    comment = txt[:txt.index("int mmw_gm_rand(")].rsplit("/*", 1)[1]
    for cite in ("gm.py:131-200", "0x47525046", "0x47524b59", "seed >> 32", "ascending order_key", "descending pref_val", "lower slot", "4800",
                 "mmw_gm_create_from_env", "device == -1"):
        assert cite in comment, cite
    comment = txt[:txt.index("int mmw_batch_gm_rand(")].rsplit("/*", 1)[1]
    for cite in ("mmw_gm_rand", "MMW_BATCH_EPILOGUE_MAX_K", "clique condition is NOT needed", "stop_at_first", "host-only batch"):
        assert cite in comment, cite
    L = _lib.lib()
    p_i32, p_f64, p_u64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    for name in ("mmw_gm_rand", "mmw_gm_rand_draw", "mmw_batch_gm_rand", "mmw_batch_env_gm_rand"):
        assert name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).restype is C.c_int, name
    assert L.mmw_gm_rand.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int, p_i32, p_i32, p_i32]
    assert L.mmw_gm_rand_draw.argtypes == [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, p_f64, p_f64]
    assert L.mmw_batch_gm_rand.argtypes == L.mmw_batch_env_gm_rand.argtypes == [C.c_void_p, p_i32, p_i32, C.c_int32, C.c_int, p_u64, p_i32, p_i32, p_i32]
    sig = inspect.signature(_lib.GreedyHandle.rand).parameters
    assert list(sig) == ["self", "Z", "nattempt", "seed", "pick"] and (sig["nattempt"].default, sig["seed"].default, sig["pick"].default) == (1, 0, "first")
    assert list(inspect.signature(_lib.GreedyHandle.rand_draw).parameters) == ["self", "Z", "seed", "attempt"]
    for cls in (_lib.BatchSolver, _lib.BatchEnv):
        assert list(inspect.signature(cls.gm_rand).parameters) == ["self", "Zs", "seeds", "nattempt", "take", "stop_at_first"], cls.__name__
