"""The device Gaussian generator against tests/helpers/philox_ref.py, the NumPy restatement of its contract.

Every other test that follows a device-RNG run asks the device for its block and hands that block to the oracle, so a wrong
generator sits on both sides of the comparison.  Here the blocks come from the contract: the stand-alone draws (mmw_sketch,
mmw_batch_sketch, mmw_batch_round_randv) at the seams of their lane layout, and the draws the loops really multiplied -- with
eta = 0 the matrix stays 0, exp(L/2)R = R, and MMW_F_XHALF after n iterations is the block of iteration n - 1 -- on every launch
the sketch can ride in.

Bars.
  fp64   |entry - reference| <= 1e-13 on unit rows.  A normal is at most 8.6 before normalisation; log, sqrt and sincospi on the
         device and libm on the host are each within a few ulp, the argument 2 pi u2 of the NumPy side adds 7e-16 r: a few 1e-15
         in all, and the bar leaves about 30 times that.
  fp32   the hardware log2 / sqrt / sin / cos are not correctly rounded, so the yardstick is the reference's own fp32 error on the
         same words, e_ref = max |sketch evaluated in float32 - sketch evaluated in float64| (about 1.5e-6 / sqrt(D)), and the
         device gets 16 e_ref: a few ulp per hardware function and the fp32 inverse norm, three to four orders below the
         O(1 / sqrt(D)) a wrong word, a swapped sin / cos or an aliased group gives.  Every case prints its device / e_ref ratio
         (DESIGN.md records them).
  XHALF  the bar of the sketch of its dtype: the Lanczos step of a zero matrix scales a column by its norm and back (a few ulp of
         the entry), the batch's Taylor sum adds zeros.  The fp32 block the API hands out is the combination's fp32 result, also
         where the matrix-core kernels ran (their bf16 halves are a copy beside it), so nothing is added for the halves.
  norms  |norm - 1| <= 1e-14 (fp64) and 1e-6 (fp32: a lane sums its 16 squares in fp32, (16 + 1) 2^-24 of the sum at worst, half
         of that on the norm, plus the fp32 roundings of the inverse norm and of the entry).

Through the public entries a width is D = Z rank_radio with Z >= 2 and a state has K >= 2, so D = 1 and K = 1 exist in the
reference (test_sketch_rng_host.py) but not on the device: test_the_smallest_shapes_are_k2_and_d2 pins that, and the device
cases start at K = 2 and D = 2.  mmw_batch_round_randv does reach D' = 1 (a factor of rank 1).

Mutations of the kernels, tried once in scratch builds; each turned tests of this file red while the older device-RNG parity tests
(test_hip_timed_path.py's small cases, test_hip_batch.py's two) stayed green, except the last:
  * the key's second word taken as 0: every case whose seed has a high word, 34 of 37;
  * group index p & 63: mmw_sketch at the widths past one pass (both dtypes; the two- and three-row handles at D = 130 in fp64), the
    refusal test's widest width, round_randv at D' = 130;
  * sin and cos swapped in box_muller: every fp64 case (handles, loop, batch, round_randv), 19;
  * the >= D zeroing removed: 33 here -- and the older tests too wherever Dpad > D, since the padding then reaches the products.
The library before this file's fix of mmw_set_slots fails test_a_width_past_the_four_passes_is_refused_and_the_handle_lives_on
(both dtypes) and nothing else.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mfma_graphs as mg  # noqa: E402
import philox_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR64 = 1e-13
F32_FACTOR = 16.0
SEEDS = [0, 1 << 32, (1 << 32) + 1, (1 << 64) - 1]
ITERATIONS = [0, 1, (1 << 31) - 1]
D64 = [2, 3, 127, 128, 129, 255, 257, 511, 512]          # a lane's second pass starts at column 128
D32 = [2, 3, 4, 5, 255, 256, 257, 1023, 1024]            # ... at column 256
FORM = {_lib.F64: "f64", _lib.F32: "f32"}


@functools.lru_cache(maxsize=None)
def band(K):
    return mg.band_state(K, min(6, K - 1), clique=min(3, K))  # (K = 2: one association pair, so no list of the state is empty)


@functools.lru_cache(maxsize=64)
def reference(K, D, seed, index, form):
    """(reference block, its bar): 1e-13, or 16 e_ref of this very case."""
    ref = pr.sketch(K, D, seed, index, form)
    bar = BAR64 if form == "f64" else F32_FACTOR * float(np.max(np.abs(pr.sketch(K, D, seed, index, "f32-in-f32") - ref)))
    ref.setflags(write=False)
    return ref, bar


def hold(got, ref, bar, form, what, unit_rows=True):
    """Prints the figures, then asserts: finite, within the bar, unit rows.  Returns error / bar."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what
    err = float(np.max(np.abs(got - ref)))
    nrm = float(np.max(np.abs(np.linalg.norm(got, axis=1) - 1.0)))
    ratio = err / bar
    print("[sketch-rng] %-58s err %.2e bar %.2e (%s) |norm - 1| %.1e" % (
        what, err, bar, "%.2f of it" % ratio if form == "f64" else "%.2f e_ref" % (ratio * F32_FACTOR), nrm))
    assert err <= bar, (what, err, bar)
    if unit_rows:
        assert nrm <= (1e-14 if form == "f64" else 1e-6), (what, nrm)
    return ratio


def hold_sketch(s, seed, it, what):
    form = FORM[s.dtype]
    ref, bar = reference(s.K, s.D, seed, it, form)
    return hold(s.sketch(seed, it), ref, bar, form, "%s %s K %d D %d seed %#x it %d" % (what, form, s.K, s.D, seed, it))


# ---- mmw_sketch against sketch() ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [_lib.F64, _lib.F32], ids=["f64", "f32"])
def test_mmw_sketch_at_every_width_seed_and_iteration(dtype):
    """K = 70 (17 full workgroups of 4 rows and a half one); one handle, its width changed through set_slots (rank_radio 1, D = Z).
    Every width at one (seed, iteration); every seed x iteration at an odd width in the second pass and at a narrow one."""
    widths = D64 if dtype == _lib.F64 else D32
    s = _lib.Solver(widths[0], band(70), 4, 0.0, rank_radio=1, dtype=dtype)
    for D in widths:
        if D != s.D:
            s.set_slots(D, 4)
        assert s.D == D and s.K == 70
        hold_sketch(s, (1 << 32) + 1, 1, "width")
        if D in (3, 257):
            for seed in SEEDS:
                for it in ITERATIONS:
                    hold_sketch(s, seed, it, "seed x iteration")
    s.close()


@pytest.mark.parametrize("dtype", [_lib.F64, _lib.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", [2, 3])
def test_mmw_sketch_on_a_partial_workgroup(K, dtype):
    """Fewer rows than one workgroup's four waves; widths with a partly zeroed last group."""
    s = _lib.Solver(2, band(K), 4, 0.0, rank_radio=1, dtype=dtype)
    for D in (2, 3, 5, 130):
        if D != s.D:
            s.set_slots(D, 4)
        for seed, it in ((0, 0), ((1 << 64) - 1, (1 << 31) - 1)):
            hold_sketch(s, seed, it, "partial workgroup")
    s.close()


@pytest.mark.parametrize("dtype", [_lib.F64, _lib.F32], ids=["f64", "f32"])
def test_mmw_sketch_past_the_grid_stride(dtype):
    """K = 16 387: the grid is capped at ROW_GRID_MAX = 4096 workgroups of 4 rows, so rows 16 384 ... 16 386 are a second trip."""
    s = _lib.Solver(2, band(16387), 4, 0.0, rank_radio=2, dtype=dtype)
    assert s.K == 16387 and s.D == 4
    hold_sketch(s, (1 << 32) + 1, 1, "grid stride")
    s.close()


def test_the_smallest_shapes_are_k2_and_d2():
    """D = 1 and K = 1 cannot be asked for: the slot count is at least 2 (the constraints divide by Z - 1), and so is K."""
    with pytest.raises(_lib.MMWError, match="status -1: .*Z must be >= 2"):
        _lib.Solver(1, band(3), 4, 0.0, rank_radio=1, dtype=_lib.F64)
    one = (band(3)[0][:1, :1], band(3)[1][:1, :1], np.ones(1))
    with pytest.raises(_lib.MMWError, match="status -1: .*K must be >= 2"):
        _lib.Solver(2, one, 4, 0.0, rank_radio=1, dtype=_lib.F64)
    with pytest.raises(_lib.MMWError, match="status -1: .*Z must be >= 2"):
        _lib.BatchSolver([1], [band(3)], 1, 0.0, rank_radio=1)


@pytest.mark.parametrize("dtype,D", [(_lib.F64, 513), (_lib.F32, 1025)], ids=["f64-513", "f32-1025"])
def test_a_width_past_the_four_passes_is_refused_and_the_handle_lives_on(dtype, D):
    """A lane draws at most four groups (NS = 4): 512 fp64 / 1024 fp32 columns.  One more is refused with MMW_ERR_ARG at creation and at
    set_slots, and after the refusal the handle is still the one it was: same sizes, same blocks, and it iterates."""
    with pytest.raises(_lib.MMWError, match="status -1: .*too large"):
        _lib.Solver(D, band(70), 4, 0.0, rank_radio=1, dtype=dtype)
    s = _lib.Solver(7, band(70), 4, 0.0, rank_radio=1, dtype=dtype)
    before = s.sketch(5, 1)
    with pytest.raises(_lib.MMWError, match="status -1: mmw_set_slots: .*too large"):
        s.set_slots(D, 4)
    assert s._sizes()[:4] == [70, 7, 7, s.Dpad]
    s._load_sizes()
    assert (s.K, s.Z, s.D) == (70, 7, 7)
    assert np.array_equal(s.sketch(5, 1), before)
    hold_sketch(s, 5, 1, "after the refusal")
    s.iterate(2, None, seed=5)
    form = FORM[dtype]
    ref, bar = reference(70, 7, 5, 1, form)
    hold(s.read(_lib.F_XHALF), ref, bar, form, "XHALF after the refusal %s" % form, unit_rows=False)
    s.set_slots(D - 1, 4)  # the widest width still goes
    hold_sketch(s, 5, 1, "widest")
    s.close()


# ---- the draws the loop multiplies: eta = 0, XHALF after n iterations is the block of iteration n - 1 --------------------------------
# path: (dtype, graph, D, switches, SpMM kind the handle must report)
LOOP_PATHS = {
    "rides-in-loss-f32": (_lib.F32, "band70", 7, {}, None),
    "own-launch-f32": (_lib.F32, "band70", 7, {"MMW_NO_LOSS_SKETCH": "1"}, None),
    "rides-in-sddmm-f32": (_lib.F32, "j9", 29, {"MMW_FUSED_SKETCH": "1", "MMW_NO_MFMA": "1"}, 2.0),
    "rides-in-sddmm-f64": (_lib.F64, "j9", 29, {"MMW_FUSED_SKETCH": "1"}, 2.0),
    "matrix-core-f32": (_lib.F32, "j9", 29, {}, 3.0),
    "rides-in-loss-f64": (_lib.F64, "band70", 7, {}, None),
}


@pytest.mark.parametrize("n", [1, 2, 9])
@pytest.mark.parametrize("path", list(LOOP_PATHS))
def test_the_block_the_loop_multiplied(path, n, monkeypatch):
    """A fresh handle per case, created under the path's switches (a handle reads them once).  n = 1 runs synchronously, n = 2 is one
    chunk, n = 9 two chunks (4 + 5): the sketch of a chunk's later iterations is the one that rides."""
    dtype, graph, D, switches, kind = LOOP_PATHS[path]
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    state = band(70) if graph == "band70" else mg.state(graph)
    seed = (1 << 32) + 1
    s = _lib.Solver(D, state, 16, 0.0, rank_radio=1, dtype=dtype)
    s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6 if dtype == _lib.F32 else 1e-12)
    if kind is not None:  # the case must be on the kernels it is named after, or it tests nothing
        assert s.read(_lib.F_SPMM_KIND)[0] == kind, s.read(_lib.F_SPMM_KIND)
    s.iterate(n, None, seed=seed)
    got = s.read(_lib.F_XHALF)
    spmm, info = s.read(_lib.F_SPMM_KIND), s.read(_lib.F_DUAL_INFO)
    assert np.max(np.abs(s.read(_lib.F_LVAL))) == 0.0  # eta = 0: the matrix is still zero
    assert s.iterations_done == n
    form = FORM[dtype]
    ref, bar = reference(s.K, D, seed, n - 1, form)
    print("[sketch-rng] %s n %d: SPMM_KIND %s DUAL_INFO %s" % (path, n, spmm, info))
    if path == "matrix-core-f32":
        # the Lanczos product on the matrix cores, allowed to the end, and no iteration in the first-order form (whose fp16 plane of
        # the sketch would be another bar's business)
        assert spmm[0] == 3.0 and spmm[1] == 1.0 and info[2] == 0.0, (spmm, info)
        if n > 1:
            assert info[0] > 0, info  # later iterations took X's row sums from the matrix-core SDDMM before them: it ran too
    hold(got, ref, bar, form, "XHALF %s n %d K %d D %d" % (path, n, s.K, D), unit_rows=False)
    s.close()


# ---- the batch ---------------------------------------------------------------------------------------------------------------------
BATCH_D = [2, 7, 8, 24]   # (D = 1 does not exist: see the head of the file; 24 is wide enough for three column slices)
BATCH_SEEDS = [0, (1 << 32) + 1, (1 << 64) - 1, 12345]


def new_batch(nit, eta=0.0):
    return _lib.BatchSolver(BATCH_D, [band(70)] * len(BATCH_D), nit, eta, rank_radio=1)


def test_batch_sketch_is_bitwise_the_handles_and_meets_the_reference():
    b = new_batch(1)
    s = _lib.Solver(BATCH_D[0], band(70), 1, 0.0, rank_radio=1, dtype=_lib.F64)
    for i, D in enumerate(BATCH_D):
        if D != s.D:
            s.set_slots(D, 1)
        for seed, it in zip(SEEDS, [0, 1, (1 << 31) - 1, 1]):
            got = b.sketch(i, seed, it)
            assert np.array_equal(got, s.sketch(seed, it)), (D, seed, it)
            ref, bar = reference(70, D, seed, it, "f64")
            hold(got, ref, bar, "f64", "batch sketch D %d seed %#x it %d" % (D, seed, it))
    s.close()
    b.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("split", ["one-workgroup", "row-split", "column-split"])
def test_the_block_the_batch_multiplied(split, n):
    """eta = 0 in the batch: the Taylor sum of a zero matrix is its first term, so XHALF is the block itself -- drawn by
    batch_sketch_rows in the single launch, by its row-range copy under set_row_split and by the column slice under set_split."""
    b = new_batch(4)
    if split == "row-split":
        b.set_row_split(2)
    elif split == "column-split":
        b.set_split([1, 1, 1, 3])
    b.iterate(n, None, BATCH_SEEDS)
    assert b.split_call()["path"] == {"one-workgroup": 0, "row-split": 2, "column-split": 1}[split]
    for i, D in enumerate(BATCH_D):
        assert b.iterations_done(i) == n
        ref, bar = reference(70, D, BATCH_SEEDS[i], n - 1, "f64")
        hold(b.read(i, _lib.F_XHALF), ref, bar, "f64", "batch XHALF %s n %d D %d" % (split, n, D))
    b.close()


def test_batch_round_randv_meets_the_reference():
    """The rounding's directions: Z rows (2, 3, 9 and 70: more rows than the workgroup has waves) of D' = the factor's rank
    columns (1, 2, 9, 130: a lone column, one pair, an odd width, a lane's third pass), attempts 0, 1 and 2^31 - 1."""
    Zs, ranks = [2, 3, 9, 70], [1, 2, 9, 130]
    b = _lib.BatchSolver(Zs, [band(140)] * 4, 1, 0.04, rank_radio=1)
    b.iterate(1, None, [3] * 4)
    b.factor(ranks=ranks)
    for i, (Z, Dp) in enumerate(zip(Zs, ranks)):
        assert b.factor_info(i)["rank"] == Dp
        for seed in (0, (1 << 32) + 1, (1 << 64) - 1):
            for attempt in (0, 1, (1 << 31) - 1):
                got = b.round_randv(i, seed, attempt)
                hold(got, pr.randv(Z, Dp, seed, attempt), BAR64, "f64", "round_randv Z %d D' %d seed %#x attempt %d" % (Z, Dp, seed, attempt))
    b.close()
