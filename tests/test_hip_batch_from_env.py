"""A batch built on the device from a BatchEnv (mmw_batch_create_from_env, csrc/kernels_batch_pattern.h, csrc/batch_from_env.h)
against the batch mmw_batch_create makes from the arrays `BatchEnv.state` hands out: every list equal, every fp64 field equal on its
raw bits, the sizes equal; the batch outlives the environment's next move and completes its host lists from its own copy of the
state; everything downstream (iterations, factor, rounding, carry, export, the greedy baseline) is bitwise the same; an instance is
the same alone and among neighbours; the refusals; and `batch.online_resolve_many(handover="device")` against `handover="host"`.

The shapes: the seven of test_hip_batch_online.py (one BatchEnv holds them all) and four hand-placed ones:
  wave63, wave64, wave65   K 63 / 64 / 65, A 4: the last trip of the 64-wide ballot scan is one short of full, full, and one lane
  sparse                   K 6, A 3: AP 0 hears nobody of another AP (three empty S_T' rows whose L rows are not empty), and user 2
                           sits alone on a far AP (an L row with the diagonal only)
"""
import functools

import numpy as np
import pytest

from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.graphs import _state_at, min_sinr_dec, mobile_drop
from test_hip_batch_online import SHAPES, ZS, geometry, moved_positions
from test_hip_batch_shapes import FIELDS

pytestmark = pytest.mark.gpu

ETA = 0.04
NIT = 3
MSINR = min_sinr_dec()
EXTRA = ["wave63", "wave64", "wave65", "sparse"]
ALL = SHAPES + EXTRA
ZALL = ZS + [4, 4, 4, 2]
I_LISTS = (_lib.I_L_INDPTR, _lib.I_L_INDICES, _lib.I_ST_INDPTR, _lib.I_ST_INDICES, _lib.I_GAIN_X, _lib.I_GAIN_Y, _lib.I_ASSO_X, _lib.I_ASSO_Y,
           _lib.I_DIAG_POS, _lib.I_ASSO_POS)
I_LAZY = tuple(f for f in I_LISTS if f != _lib.I_L_INDPTR)  # what a device-built batch fetches on demand
F_EAGER = (_lib.F_S_SUM, _lib.F_NORM_H, _lib.BATCH_F_PATTERN) + FIELDS  # what never needs a host list


@functools.lru_cache(maxsize=None)
def geo(name):
    """(sta_locs, ap_locs) of a shape, the hand-placed ones included; shared and left unchanged."""
    if name.startswith("wave"):
        K = int(name[4:])
        k = np.arange(K)
        sta = np.stack([(k * 37 % 61) * (40.0 / 61.0), (k * 17 % 53) * (40.0 / 53.0)], axis=1)
        return sta, np.array([[10.0, 10.0], [30.0, 10.0], [10.0, 30.0], [30.0, 30.0]])
    if name == "sparse":
        return (np.array([[3.0, 4.0], [5.0, 1.0], [5003.0, 2.0], [38.0, 3.0], [43.0, -2.0], [20.0, 1.0]]),
                np.array([[0.0, 0.0], [5000.0, 0.0], [40.0, 0.0]]))
    return geometry(name)


def moved(name):
    return moved_positions(name) if name in SHAPES else geo(name)[0][::-1] + 1.5


def new_env(names):
    return _lib.BatchEnv([geo(n)[1] for n in names], [geo(n)[0].shape[0] for n in names], min_sinr=MSINR)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)


def same_f64(x, y, inst_x, inst_y, fields, what):
    for f in fields:
        a, b = x.read(inst_x, f), y.read(inst_y, f)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, "f64 field", f)


def same_i32(x, y, inst_x, inst_y, fields, what):
    for f in fields:
        assert np.array_equal(x.read_i32(inst_x, f), y.read_i32(inst_y, f)), (what, "i32 field", f)


def build_info(b, inst):
    return [int(v) for v in b.read(inst, _lib.BATCH_F_BUILD_INFO)]


def snapshot(b, inst):
    """Everything of an instance that needs no host list, as raw bits."""
    return ([bits(b.read(inst, f)).copy() for f in F_EAGER], b.read_i32(inst, _lib.I_PATTERN).copy(), b.read_i32(inst, _lib.I_L_INDPTR).copy(),
            dict(b.sizes[inst]))


def same_snapshot(s, t):
    return all(np.array_equal(a, b) for a, b in zip(s[0], t[0])) and np.array_equal(s[1], t[1]) and np.array_equal(s[2], t[2]) and s[3] == t[3]


class Pair:
    """Every shape in one BatchEnv at its first positions, the batch built on the device from it and the batch built on the host from
    its states; shared by the tests below, which read and do not iterate."""

    def __init__(self):
        self.env = new_env(ALL)
        self.env.move([geo(n)[0] for n in ALL])
        self.dev = _lib.BatchSolver.from_env(self.env, ZALL, NIT, ETA)
        self.states = [self.env.state(i) for i in range(len(ALL))]
        self.host = _lib.BatchSolver(ZALL, self.states, NIT, ETA)


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.dev.close()
    p.host.close()
    p.env.close()


def test_hand_placed_shapes_are_what_they_claim():
    for n in ("wave63", "wave64", "wave65"):
        sta, ap = geo(n)
        P = orc.Pattern(4, _state_at(sta, ap)[0])
        rows = np.diff(P.indptr)
        assert P.K == int(n[4:]) and P.E_gain > 0 and P.E_asso > 0 and rows.min() < P.K and rows.max() > 1
        assert P.col[P.indptr[0]:P.indptr[1]].max() >= 63 - (n == "wave63")  # row 0 reaches into the scan's last trip
    sta, ap = geo("sparse")
    P = orc.Pattern(2, _state_at(sta, ap)[0])
    st_rows, l_rows = np.diff(P.ST.tocsr().indptr), np.diff(P.indptr)
    assert st_rows.tolist() == [0, 0, 0, 1, 1, 0] and l_rows[2] == 1 and all(l_rows[k] > 1 for k in (0, 1, 5))
    assert P.E_gain == 2 and P.E_asso == 4


def test_every_field_of_every_shape_is_the_host_builds(pair):
    dev, host = pair.dev, pair.host
    assert (dev.B, dev.nits, dev.active, dev.device) == (host.B, host.nits, host.active, host.device)
    assert dev.sizes == host.sizes
    for i, n in enumerate(ALL):
        assert build_info(host, i) == [0, 1]
        fresh = build_info(dev, i)
        assert fresh[0] == 1
        same_f64(dev, host, i, i, F_EAGER, n)
        same_i32(dev, host, i, i, (_lib.I_PATTERN, _lib.I_L_INDPTR), n)
        assert build_info(dev, i) == fresh, "a field that needs no host list completed them"
        same_i32(dev, host, i, i, I_LISTS, n)
        same_f64(dev, host, i, i, (_lib.F_ST_DATA,), n)
        assert build_info(dev, i) == [1, 1]
        same_f64(dev, host, i, i, F_EAGER, n)  # completing the lists changed no value


def test_the_batch_outlives_the_environments_next_move():
    env = new_env(ALL)
    env.move([geo(n)[0] for n in ALL])
    first = _lib.BatchSolver.from_env(env, ZALL, NIT, ETA)
    host_first = _lib.BatchSolver(ZALL, [env.state(i) for i in range(len(ALL))], NIT, ETA)
    before = [snapshot(first, i) for i in range(len(ALL))]
    env.move([moved(n) for n in ALL])
    second = _lib.BatchSolver.from_env(env, ZALL, NIT, ETA)
    host_second = _lib.BatchSolver(ZALL, [env.state(i) for i in range(len(ALL))], NIT, ETA)
    changed = 0
    for i, n in enumerate(ALL):
        assert same_snapshot(snapshot(first, i), before[i]), n
        assert second.sizes[i] == host_second.sizes[i]
        same_f64(second, host_second, i, i, F_EAGER + (_lib.F_ST_DATA,), n)
        same_i32(second, host_second, i, i, I_LISTS + (_lib.I_PATTERN,), n)
        changed += first.sizes[i] != second.sizes[i]
    assert changed >= 4, "the move must change the patterns for this test to say anything"
    # only now the first batch's host lists, for the first time: they are still those of the first state
    for i, n in enumerate(ALL):
        assert build_info(first, i) == [1, 0], n
        same_i32(first, host_first, i, i, I_LAZY, n)
        same_f64(first, host_first, i, i, (_lib.F_ST_DATA,), n)
        assert build_info(first, i) == [1, 1], n
    env.close()  # and the batch needs nothing of the environment afterwards
    same_i32(first, host_first, 2, 2, (_lib.I_PATTERN,), "after the environment is gone")
    for b in (first, host_first, second, host_second):
        b.close()


DOWN = ["j5", "j7", "one_ap"]
ZDOWN = [ZS[SHAPES.index(n)] for n in DOWN]
SEEDS = np.array([11, 12, 13], dtype=np.uint64)


def test_downstream_is_bitwise_the_host_built_batchs():
    B = len(DOWN)
    env = new_env(DOWN)
    env.move([geo(n)[0] for n in DOWN])
    states = [env.state(i) for i in range(B)]
    dev = _lib.BatchSolver.from_env(env, ZDOWN, NIT, ETA)
    host = _lib.BatchSolver(ZDOWN, states, NIT, ETA)
    for b in (dev, host):
        b.iterate(NIT, None, SEEDS)
        b.factor()
    assert dev.sizes == host.sizes
    rd, rh = dev.round(4, SEEDS), host.round(4, SEEDS)
    for i, n in enumerate(DOWN):
        same_f64(dev, host, i, i, FIELDS + (_lib.F_SKETCH,), n)
        assert np.array_equal(bits(dev.read_factor(i)), bits(host.read_factor(i))), n
        assert build_info(dev, i) == [1, 0], "iterating, factoring and rounding need no host list"
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for x, y in zip(rd, rh) for a, b in zip(x, y))
    # the greedy baseline: the clique decision comes from the batch's own copy of Q and completes no host list
    gd, gh = dev.gm(0, ZDOWN, keys=True), host.gm(0, ZDOWN, keys=True)
    for i in range(B):
        assert np.array_equal(gd[0][i], gh[0][i]) and np.array_equal(bits(gd[3][i]), bits(gh[3][i]))
        assert build_info(dev, i) == [1, 0]
    assert np.array_equal(gd[1], gh[1]) and np.array_equal(gd[2], gh[2])
    # export into a handle
    for i, n in enumerate(DOWN):
        s1, s2 = (_lib.Solver(ZDOWN[i], states[i], NIT, ETA) for _ in range(2))
        dev.export(i, s1)
        host.export(i, s2)
        for f in (_lib.F_Y, _lib.F_E_ACCU, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG):
            assert np.array_equal(bits(s1.read(f)), bits(s2.read(f))), (n, f)
        assert s1.iterations_done == s2.iterations_done == NIT
        s1.close()
        s2.close()
    # a carry across the move: from the host-built batch (and from the device-built one) into a device-built batch on the moved
    # state, against the same carry into a host-built one
    env.move([moved(n) for n in DOWN])
    into_dev, from_dev = (_lib.BatchSolver.from_env(env, ZDOWN, NIT, ETA) for _ in range(2))
    into_host = _lib.BatchSolver(ZDOWN, [env.state(i) for i in range(B)], NIT, ETA)
    into_dev.carry_from(host)
    from_dev.carry_from(dev)
    into_host.carry_from(host)
    for i, n in enumerate(DOWN):
        same_f64(into_dev, into_host, i, i, FIELDS, n)
        same_f64(from_dev, into_host, i, i, FIELDS, n)
        lm, cm = into_dev.carry_map(host, i)
        lm0, cm0 = into_host.carry_map(host, i)
        assert np.array_equal(lm, lm0) and np.array_equal(cm, cm0)
    for b in (into_dev, into_host):
        b.iterate(NIT, None, SEEDS)
    for i, n in enumerate(DOWN):
        same_f64(into_dev, into_host, i, i, FIELDS, n)
    # a reset writes the initial point again (one launch for a device-built batch), and the run repeats bit for bit
    for b in (dev, host):
        b.reset(NIT)
    for i, n in enumerate(DOWN):
        same_f64(dev, host, i, i, F_EAGER, n)
    for b in (dev, host):
        b.iterate(NIT, None, SEEDS)
    for i, n in enumerate(DOWN):
        same_f64(dev, host, i, i, FIELDS, n)
    for b in (dev, host, into_dev, from_dev, into_host):
        b.close()
    env.close()


def same_gm(got, want, who):
    for i in who:
        assert np.array_equal(got[0][i], want[0][i]) and np.array_equal(bits(got[3][i]), bits(want[3][i])), i
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_gm_with_other_takers_in_every_call_answers_as_the_host_built_batch():
    """The decisions of all instances go up once, at the first call: a FIRST call that takes instance 0 only, then instance 1 only, then
    instance 2 only, then all, and an instance that sat out of a slot change and came back, each against the host-built batch."""
    B = len(DOWN)
    env = new_env(DOWN)
    env.move([geo(n)[0] for n in DOWN])
    dev = _lib.BatchSolver.from_env(env, ZDOWN, NIT, ETA)
    host = _lib.BatchSolver(ZDOWN, [env.state(i) for i in range(B)], NIT, ETA)
    env.close()
    for kind in (0, 1):
        for who in ([0], [1], [2], [0, 1, 2], [1]):
            take = [i in who for i in range(B)]
            same_gm(dev.gm(kind, ZDOWN, take=take, keys=True), host.gm(kind, ZDOWN, take=take, keys=True), who)
    dev.close()
    # the search's pattern: instances sit out of a slot change before the first baseline and come back afterwards
    env = new_env(DOWN)
    env.move([geo(n)[0] for n in DOWN])
    dev = _lib.BatchSolver.from_env(env, ZDOWN, NIT, ETA)
    env.close()
    for Zs, who in (([0, ZDOWN[1], 0], [1]), (ZDOWN, [0, 1, 2])):
        for b in (dev, host):
            b.set_slots(Zs, NIT)
        same_gm(dev.gm(0, ZDOWN, keys=True), host.gm(0, ZDOWN, keys=True), who)
    for i in range(B):
        assert build_info(dev, i) == [1, 0]
    out = np.empty(1, dtype=np.int32)
    assert _lib.lib().mmw_batch_read_i32(dev._h, 0, 99, _lib._pi(out), 1) == -1 and b"unknown field" in _lib.lib().mmw_last_error()
    assert build_info(dev, 0) == [1, 0], "an unknown field id completed the host lists"
    dev.close()
    host.close()


@pytest.mark.parametrize("k", range(len(ALL)), ids=ALL)
def test_alone_and_among_neighbours(pair, k):
    env = new_env([ALL[k]])
    env.move([geo(ALL[k])[0]])
    one = _lib.BatchSolver.from_env(env, [ZALL[k]], NIT, ETA)
    env.close()
    assert one.sizes[0] == pair.dev.sizes[k]
    same_f64(one, pair.dev, 0, k, F_EAGER + (_lib.F_ST_DATA,), ALL[k])
    same_i32(one, pair.dev, 0, k, I_LISTS + (_lib.I_PATTERN,), ALL[k])
    one.close()


def test_refusals_name_the_instance_and_leave_the_environment_usable():
    names = ["one_ap", "j5"]
    env = new_env(names)
    with pytest.raises(_lib.MMWError, match=r"status -3: mmw_batch_create_from_env: instance 0: .*no positions yet"):
        _lib.BatchSolver.from_env(env, [2, 6], NIT, ETA)
    env.move([geo(n)[0] for n in names])
    with pytest.raises(_lib.MMWError, match=r"status -1: mmw_batch_create_from_env: instance 1: Z must be >= 2"):
        _lib.BatchSolver.from_env(env, [2, 1], NIT, ETA)
    with pytest.raises(_lib.MMWError, match=r"status -1: mmw_batch: instance 1: D = 600 exceeds the batch limit 512 \(run it on a handle\)"):
        _lib.BatchSolver.from_env(env, [2, 300], NIT, ETA)
    with pytest.raises(_lib.MMWError, match="3 slot counts for the environment's 2 instances"):
        _lib.BatchSolver.from_env(env, [2, 6, 6], NIT, ETA)
    env.move([moved(n) for n in names])
    dev = _lib.BatchSolver.from_env(env, [2, 6], NIT, ETA)
    host = _lib.BatchSolver([2, 6], [env.state(i) for i in range(2)], NIT, ETA)
    for i, n in enumerate(names):
        same_f64(dev, host, i, i, F_EAGER, n)
        assert build_info(dev, i) == [1, 0]
    # a slot change needs no host list either: cold, then warm after two iterations
    for warm, Zs in ((False, [2, 7]), (True, [2, 5])):
        for b in (dev, host):
            b.set_slots(Zs, NIT, warm=warm)
            b.iterate(2, None, SEEDS[:2])
        assert dev.sizes == host.sizes
        for i, n in enumerate(names):
            same_f64(dev, host, i, i, F_EAGER, n)
            assert build_info(dev, i) == [1, 0]
    with pytest.raises(_lib.MMWError, match=r"instance 1: Z must be >= 2"):
        dev.set_slots([2, 1], NIT)
    for i, n in enumerate(names):
        same_i32(dev, host, i, i, I_LISTS + (_lib.I_PATTERN,), n)
        same_f64(dev, host, i, i, F_EAGER, n)
    dev.close()
    host.close()
    env.close()


@pytest.mark.parametrize("carry", [False, True], ids=["cold", "carried"])
def test_online_resolve_many_is_the_same_with_either_handover(carry):
    def run(handover):
        drops = [mobile_drop(c, 75e-4, s) for c in (5, 6) for s in (0, 1)]
        return batch.online_resolve_many(drops, n_points=3, nit=20, mob_spd_meter_s=3.0, factor_split="auto", carry=carry, handover=handover)
    dev, host = run("device"), run("host")
    assert len(dev) == len(host) == 4
    for d, h in zip(dev, host):
        assert d["Z"] == h["Z"]
        for key in ("z_vec", "remainder", "bler", "iters"):
            assert np.array_equal(np.asarray(d[key]), np.asarray(h[key])), key
