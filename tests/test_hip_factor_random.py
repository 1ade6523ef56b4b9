"""The random embedding as a solver handle's resident factor, on the device (mmw_factor_random, csrc/kernels_factor_random.h).

1. Every width at one seed, every seed at two widths, against `philox_ref.sketch(K, cols, seed, 0, "f64")`: the bars are
   test_hip_sketch_rng.py's for the fp64 sketch, for its reasons (|entry - reference| <= 1e-13 on unit rows, |norm - 1| <= 1e-14),
   on fp64 and fp32 handles, whose blocks are bitwise equal.
2. Row edges: a partial workgroup, rows past the grid stride.
3. Bitwise ties: the fp64 handle's `sketch(seed, 0)` where cols is its D, `BatchSolver.factor_random` + `read_factor`,
   `rand_sdp_solver.index_ordered` of the plain block.
4. Nothing else moves: between two `iterate` calls with a chunk pending, against a twin nobody asked.
5. Rounding the resident block: every attempt equals the oracle's on the block read back and the device's own directions.
6. Refusals on a live handle.

The margin condition of 5, checked on the CPU when the seeds were fixed (the key is probe_seed(5, 0, 0x40000) = 0x50000040000 for
the block and for the directions): with `philox_ref.sketch` / `philox_ref.randv` through `round_cases.reference_attempt`'s inner
products, every user's smallest difference between two consecutive sorted inner products, attempts 0 and 1, is
    k75   (K 75,   Z 6,  cols 12)   1.31e-04, 7.98e-05
    k192  (K 192,  Z 9,  cols 18)   7.50e-06, 5.63e-05
    k1083 (K 1083, Z 14, cols 28)   2.49e-06, 1.73e-06
against the condition's 1e-9 and the block's bar of 1e-13: no preference order hangs on the last bits of a normal.  (On those
draws the reference leaves 12, 8 / 4, 2 / 1, 1 users over on the own states and 10, 9 / 5, 2 / 0, 1 on the moved ones: both
outcomes of an attempt occur.)
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mfma_graphs as mg  # noqa: E402
import online_cases as OC  # noqa: E402
import philox_ref as pr  # noqa: E402

from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.graphs import _NOISE_FLOOR_DBM, min_sinr_dec  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver  # noqa: E402

pytestmark = pytest.mark.gpu

BAR64 = 1e-13
ETA = 0.04
DTYPES = [_lib.F64, _lib.F32]
IDS = ["f64", "f32"]
SEEDS = [0, 1 << 32, (1 << 32) + 1, (1 << 64) - 1]  # test_hip_sketch_rng.py's
WIDTHS = [1, 2, 3, 127, 128, 129, 511, 512, 513, 1030]
KEY = probe_seed(5, 0, 0x40000)
MAX_COLS = 2 ** 31 - 1 - 64
FIELDS = ("F_Y", "F_E_ACCU", "F_LVAL", "F_XVAL", "F_XAVG", "F_YAVG", "F_E_THIS", "F_XHALF", "F_EXPM_INFO")


@functools.lru_cache(maxsize=None)
def band(K):
    return mg.band_state(K, min(6, K - 1), clique=min(3, K))


@functools.lru_cache(maxsize=64)
def reference(K, cols, seed):
    ref = pr.sketch(K, cols, seed, 0, "f64")
    ref.setflags(write=False)
    return ref


def hold(got, K, cols, seed, what):
    ref = reference(K, cols, seed)
    assert got.shape == ref.shape == (K, cols) and got.dtype == np.float64 and np.all(np.isfinite(got)), what
    err = float(np.max(np.abs(got - ref)))
    nrm = float(np.max(np.abs(np.linalg.norm(got, axis=1) - 1.0)))
    print("[factor-random] %-44s K %5d cols %4d seed %#x: err %.2e (bar %.0e) |norm - 1| %.1e" % (what, K, cols, seed, err, BAR64, nrm))
    assert err <= BAR64, (what, err)
    assert nrm <= 1e-14, (what, nrm)


def pair(K, Z=2):
    return [_lib.Solver(Z, band(K), 4, ETA, rank_radio=1, dtype=dt) for dt in DTYPES]


def read(s):
    return {f: s.read(getattr(_lib, f)) for f in FIELDS}


def same(got, ref, what):
    for f in ref:
        assert got[f].shape == ref[f].shape and got[f].tobytes() == ref[f].tobytes(), (what, f)


# ---- 1. every width at one seed ------------------------------------------------------------------------------------------------------
def test_every_width_and_seed_on_both_dtypes():
    """K = 70: 17 full workgroups of 4 rows and a half one.  A lane's second pass starts at column 128, its fifth -- the first the
    sketch does not have -- at 512; 1030 ends in the ninth."""
    s64, s32 = pair(70)
    for cols in WIDTHS:
        for seed in (SEEDS if cols in (3, 257) else [(1 << 32) + 1]):
            a, b = s64.factor_random(cols, seed), s32.factor_random(cols, seed)
            hold(a, 70, cols, seed, "width")
            assert a.tobytes() == b.tobytes(), (cols, seed)
    for seed in SEEDS:
        a, b = s64.factor_random(257, seed), s32.factor_random(257, seed)
        hold(a, 70, 257, seed, "seed at cols 257")
        assert a.tobytes() == b.tobytes(), seed
    # what tells the draws apart does: the low and the high word of the seed
    base = s64.factor_random(9, 5)
    for other in (s64.factor_random(9, 6), s64.factor_random(9, 5 + (1 << 32))):
        assert float(np.max(np.abs(other - base))) > 1e-3
    s64.close()
    s32.close()


# ---- 2. row edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
def test_a_partial_workgroup(K):
    s64, s32 = pair(K)
    for cols in (2, 5, 130):
        for seed in (0, (1 << 64) - 1):
            a = s64.factor_random(cols, seed)
            hold(a, K, cols, seed, "partial workgroup")
            assert a.tobytes() == s32.factor_random(cols, seed).tobytes()
    s64.close()
    s32.close()


@functools.lru_cache(maxsize=None)
def big_blocks():
    """K = 16 387 at cols 4: the grid is capped at 4096 workgroups of 4 rows, so rows 16 384 ... 16 386 are a second trip.  The plain
    and the index-ordered block of an fp32 handle, and the plain one of an fp64 handle (shared by the tests below)."""
    seed = (1 << 32) + 1
    s = _lib.Solver(2, band(16387), 4, ETA, rank_radio=2, dtype=_lib.F32)
    plain, ordered = s.factor_random(4, seed), s.factor_random(4, seed, index_order=True)
    s.close()
    s = _lib.Solver(2, band(16387), 4, ETA, rank_radio=2, dtype=_lib.F64)
    plain64 = s.factor_random(4, seed)
    same_as_sketch = plain64.tobytes() == s.sketch(seed, 0).tobytes()
    s.close()
    return seed, plain, ordered, plain64, same_as_sketch


def test_rows_past_the_grid_stride():
    seed, plain, ordered, plain64, same_as_sketch = big_blocks()
    hold(plain, 16387, 4, seed, "grid stride")
    assert plain.tobytes() == plain64.tobytes() and same_as_sketch
    assert float(np.max(np.abs(plain[16384:] - reference(16387, 4, seed)[16384:]))) <= BAR64 and np.all(np.linalg.norm(plain[16384:], axis=1) > 0.5)


# ---- 3. bitwise ties -------------------------------------------------------------------------------------------------------------------
def test_the_block_is_the_fp64_handles_sketch_of_iteration_0():
    """cols = the handle's D <= 512: `sketch(seed, 0)` of an fp64 handle, bit for bit -- from that handle and from an fp32 one."""
    s64 = _lib.Solver(2, band(70), 4, ETA, rank_radio=1, dtype=_lib.F64)
    s32 = _lib.Solver(2, band(70), 4, ETA, rank_radio=1, dtype=_lib.F32)
    for D in (2, 3, 129, 257, 511, 512):
        if D != s64.D:
            s64.set_slots(D, 4)
        for seed in ((1 << 32) + 1, (1 << 64) - 1):
            want = s64.sketch(seed, 0)
            assert s64.factor_random(D, seed).tobytes() == want.tobytes(), (D, seed)
            assert s32.factor_random(D, seed).tobytes() == want.tobytes(), (D, seed)
    s64.close()
    s32.close()


@pytest.mark.parametrize("name", ["k75", "k192"])
def test_the_block_is_the_batchs_factor_random(name):
    _, _, K, Z = OC.CASES[name]
    state = OC.host_state(name, 0)
    b = _lib.BatchSolver([Z], [state], 1, ETA)
    for dt in DTYPES:
        s = _lib.Solver(Z, state, 1, ETA, dtype=dt)
        for seed in (KEY, (1 << 64) - 1):
            b.factor_random([seed])
            want = b.read_factor(0)
            assert want.shape == (K, 2 * Z)
            assert s.factor_random(2 * Z, seed).tobytes() == want.tobytes(), (name, dt, seed)
        s.close()
    b.close()


def test_index_order_is_index_ordered_of_the_plain_block():
    s64, s32 = pair(70)
    for cols in (1, 3, 130, 513):
        for s in (s64, s32):
            plain = s.factor_random(cols, KEY)
            got = s.factor_random(cols, KEY, index_order=True)
            assert got.tobytes() == rand_sdp_solver.index_ordered(plain).tobytes(), cols
            df = s.factor_random(cols, KEY, resident=True, index_order=True)
            assert isinstance(df, _lib.DeviceFactor) and df.index_ordered and df._host is None and df.shape == (70, cols)
            assert rand_sdp_solver.index_ordered(df) is df and df._host is None
            assert np.asarray(df).tobytes() == got.tobytes()
            assert not s.factor_random(cols, KEY, resident=True).index_ordered
    s64.close()
    s32.close()
    seed, plain, ordered, _, _ = big_blocks()
    assert ordered.tobytes() == rand_sdp_solver.index_ordered(plain).tobytes()
    assert np.all(np.diff(np.linalg.norm(ordered, axis=1)[[0, 4096, 16384, 16386]]) < 0)  # the norms fall with the index


# ---- 4. nothing else moves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nothing_else_moves(dtype):
    """k192 on device sketches, n = 24 announced: 10 iterations, the call -- no read in between, so the chunk is still pending --, then
    the other 14.  A twin runs 10 + 14 and is never asked.  Every field is bitwise the twin's straight after the call and after the
    remaining iterations."""
    _, _, K, Z = OC.CASES["k192"]
    state = OC.host_state("k192", 0)
    s, twin = (_lib.Solver(Z, state, 24, ETA, dtype=dtype) for _ in range(2))
    for h in (s, twin):
        h.iterate(10, None, seed=7)
    df = s.factor_random(2 * Z, KEY, resident=True, index_order=True)  # (resident: nothing is copied out, nothing waits)
    for h in (s, twin):
        h.iterate(14, None, seed=7)
    same(read(s), read(twin), "after the remaining iterations")
    assert s.iterations_done == twin.iterations_done == 24
    assert np.array_equal(s.read(_lib.F_BLOCKING), twin.read(_lib.F_BLOCKING))
    block = np.asarray(df)
    assert block.tobytes() == rand_sdp_solver.index_ordered(s.factor_random(2 * Z, KEY)).tobytes()
    # ... and with a read straight after the call
    s2, twin2 = (_lib.Solver(Z, state, 24, ETA, dtype=dtype) for _ in range(2))
    for h in (s2, twin2):
        h.iterate(10, None, seed=7)
    s2.factor_random(2 * Z, KEY)
    same(read(s2), read(twin2), "straight after the call")
    for h in (s2, twin2):
        h.iterate(14, None, seed=7)
    same(read(s2), read(twin2), "after the remaining iterations, read in between")
    # factor() and factor_random replace each other; FACTOR_ROWNORM belongs to a spectral block
    rank = min(K - 1, (Z - 1) * 2)
    f1 = s.factor(rank, seed=3, resident=True)
    held = s.factor_random(2 * Z, KEY, resident=True)  # f1 is copied out before the block overwrites it
    assert f1._host is not None and f1.shape == (K, rank) and held.shape == (K, 2 * Z)
    f1_again = s.factor(rank, seed=3)
    assert held._host is not None  # ... and so was the block
    assert np.asarray(f1).tobytes() == f1_again.tobytes() == twin.factor(rank, seed=3).tobytes()
    assert np.asarray(held).tobytes() == s.factor_random(2 * Z, KEY).tobytes() == twin2.factor_random(2 * Z, KEY).tobytes()
    assert s.read(_lib.F_FACTOR, K * 2 * Z).tobytes() == np.asarray(held).tobytes()
    s.factor_spectral(Z)
    assert s.factor_row_norms().shape == (K,)
    s.factor_random(2 * Z, KEY)
    with pytest.raises(_lib.MMWError, match="status -3"):
        s.factor_row_norms()
    same(read(s), read(twin), "after the factors")
    for h in (s, twin, s2, twin2):
        h.close()


def test_no_iteration_needs_to_have_run():
    s = _lib.Solver(5, band(70), 4, ETA, dtype=_lib.F32)
    hold(s.factor_random(10, KEY), 70, 10, KEY, "fresh handle")
    assert s.iterations_done == 0
    s.iterate(4, None, seed=1)
    s.sync()
    assert s.iterations_done == 4
    s.close()


# ---- 5. rounding the resident block ----------------------------------------------------------------------------------------------------
def new_env(name, moved=0):
    ap, p0, p1 = OC.positions(name)
    return _lib.DeviceEnv(p1 if moved else p0, ap, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", OC.NAMES)
def test_rounding_the_resident_block_is_the_oracles(name, dtype):
    """Own state (`round_attempts`) and moved state (`round_env_attempts`), 2 attempts, gX = None and the DeviceFactor: every
    attempt's slots and count equal `oracle.rounding_one_attempt` on index_ordered(the block read back) and the device's own
    directions -- what test_hip_batch_gm.py asserts for the batch.  The margins are in the head of this file."""
    _, _, K, Z = OC.CASES[name]
    cols, natt = 2 * Z, 2
    env = new_env(name)
    s = _lib.Solver.from_env(env, Z, 2, ETA, dtype=dtype)
    env.move(OC.positions(name)[2])
    plain = s.factor_random(cols, KEY)
    df = s.factor_random(cols, KEY, resident=True, index_order=True)
    reads = []
    real_read = s.read
    s.read = lambda which, n=None: reads.append(which) or real_read(which, n)
    rvs = [s.round_randv(Z, cols, KEY, a) for a in range(natt)]
    for a in range(natt):
        assert float(np.max(np.abs(rvs[a] - pr.randv(Z, cols, KEY, a)))) <= BAR64
    results = {}
    for gX in (None, df):
        results[("own", gX is None)] = s.round_attempts(Z, gX, natt, KEY, all_attempts=True)
        results[("moved", gX is None)] = s.round_env_attempts(env, Z, gX, natt, KEY, all_attempts=True)
    assert reads == [] and df._host is None  # the block never crossed to the host for the roundings
    s.read = real_read
    block = np.asarray(df)
    assert block.tobytes() == rand_sdp_solver.index_ordered(plain).tobytes()
    for where, state in (("own", OC.host_state(name, 0)), ("moved", OC.host_state(name, 1))):
        want = []
        for a in range(natt):
            zo, _, remo, un = orc.rounding_one_attempt(Z, block, state, rvs[a])
            want.append((np.where(un, -1, zo).astype(np.int32), int(remo)))
        for by_none in (True, False):
            z, rem, pick, z_all = results[(where, by_none)]
            for a in range(natt):
                print("[factor-random] %s %s attempt %d: left over %d (oracle %d), %d slots differ" % (
                    name, where, a, rem[a], want[a][1], int(np.sum(z_all[a] != want[a][0]))))
                assert int(rem[a]) == want[a][1] and np.array_equal(z_all[a], want[a][0]), (name, where, a)
            first = [r for _, r in want]
            assert pick == (first.index(0) if 0 in first else natt - 1) and np.array_equal(z, want[pick][0])
            assert np.all((z_all >= -1) & (z_all < Z))
    s.close()
    env.close()


# ---- 6. refusals on a live handle ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_last_factor_standing():
    s = _lib.Solver(5, band(70), 4, ETA, dtype=_lib.F64)
    before = s.factor_random(10, KEY)
    L = _lib.lib()
    for args, status, msg in (((0, 0), -1, "cols = 0 must be >= 1"), ((10, 2), -1, "index_order = 2 must be 0 or 1"),
                              ((MAX_COLS + 1, 0), -1, "cols = %d exceeds" % (MAX_COLS + 1)),
                              ((MAX_COLS, 0), -2, "70 x %d doubles" % MAX_COLS)):  # 1.2 TB: refused on the free-memory figure, nothing is allocated
        assert L.mmw_factor_random(s._h, args[0], args[1], None, 1) == status, args
        assert msg in L.mmw_last_error().decode(), (args, L.mmw_last_error().decode())
        assert s.read(_lib.F_FACTOR, 700).reshape(70, 10).tobytes() == before.tobytes()
    z, rem, pick = s.round_attempts(5, None, 2, KEY)  # and the rounding still finds it
    assert z.shape == (70,) and rem.shape == (2,)
    s.close()
