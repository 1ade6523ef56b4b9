"""Shapes of the matrix-core SpMM and SDDMM (csrc/kernels_mfma.h: k_spmm_mfma, k_sddmm_mfma) inside the MMW loop, against the fp64
CPU oracle (oracle/mmw_oracle.py: the reference loop restated, exp(L/2)R by SciPy's expm_multiply).

Which instantiation a product runs on follows from three things (csrc/expm_engine.h, spmm_mfma_launch):
  * row tiles MT: 2 when a block of the matrix-core blocking has more than 32 rows (MMW_MF_ROWS, default 64), else 1;
  * column tiles per workgroup `gt`: MMW_MF_GT = 4 | 8 | 12, or by the grid's size -- which gives 4 at every size a test can run,
    so the wider groups are reached through the switch only; then gt = 4 for ntiles <= 4 and gt <= 8 for ntiles <= 8;
  * the padded width Dpad (fp32: 4 pow2ceil(ceil(D / 4)) for D <= 128, else 32 ceil(D / 32)) and ntiles = Dpad / 32 in
    {1, 2, 4, 5, 6, ...}.  Every handle here has rank_radio = 1, so D = Z; the widths are ragged (D = Dpad - 3) with a few exact ones.
The launch forms <MT, NT, NW, MS, KC, NB> (row tiles, column tiles per wave, waves, row-tile groups of waves, k-steps per chunk,
chunks resident):
    MT 1:  gt 4 <1,1,4,1,2,2>    gt 8 <1,2,4,1,2,2>    gt 12 <1,3,4,1,1,3>
    MT 2:  gt 4 <2,1,8,2,2,2>    gt 8 <2,2,8,2,2,2>    gt 12 <2,3,4,1,1,3>    gt 4, first-order epilogue: <2,1,8,2,4,2>
A workgroup of column group y takes ng = min(gt, ntiles - gt y) tiles: full groups and, behind them, one remainder group.  ng sets
the staged row's pitch, the float-reciprocal decode of the LDS-DMA pieces, the hand-counted s_waitcnt vmcnt, and the bank rotation:
ng & 3 == 0 rotates a row's 64-byte groups by (row & 3), ng & 3 == 2 by (row & 3) >> 1, odd ng not at all.

The graphs are the designed ones of tests/helpers/mfma_graphs.py (their blocks are pinned by test_mfma_shapes_host.py); a block is
written rows:k-steps.  Bars: exp(L/2)R <= 1e-5 relative Frobenius, every other quantity of the loop <= 1e-4 (compare() of
test_hip_timed_path.py: e_this, e_accu, Y, L, X on the pattern, the running sums).  Uploaded sketches run the synchronous path at
set_expm(LANCZOS, 16, 1e-7); device-RNG runs the shipped path at bench.py's (LANCZOS, 12, 1e-6).  Every fp32 handle asserts
MMW_F_SPMM_KIND[0] == 3, and where nothing is meant to rule the kernel out also [1] == 1 at the end (the two-half split needs
2.3e-5 max_i sum_j |a_ij| <= tol, which at tol = 1e-7 bounds the step size of the synchronous legs: ETA_SYNC, per graph).

  Leg A  column groups of the Lanczos product (k_spmm_mfma<SPMM_LANCZOS>, planes from k_lz_update) and of the SDDMM.  3 iterations,
         every one compared.  `hub` (MT 2: 64:8 x5, 64:24, 11:4, 2:4, 1:4 x3) and `hubr32` (MT 1: 18 blocks, 32:24 beside 1:4).
           MMW_MF_GT=4    ntiles 1 2 4 5 6 7 8         ng: 1 | 2 | 4 | 4+1 | 4+2 | 4+3 | 4+4       <1,1,4,1,2,2> / <2,1,8,2,2,2>
           MMW_MF_GT=8    ntiles 5 6 7 8 9 11 13       ng: 5 | 6 | 7 | 8 | 8+1 | 8+3 | 8+5         <1,2,4,1,2,2> / <2,2,8,2,2,2>
           MMW_MF_GT=12   ntiles 9 10 11 12 13         ng: 9 | 10 | 11 | 12 | 12+1                 <1,3,4,1,1,3> / <2,3,4,1,1,3>
           exact widths   D = 256 (gt 4: 4+4), 160 (gt 8: 5), 384 (gt 12: 12)
           no switch      D = 16 (Dpad 16: the kind reads 3 but the products run on the LDS kernel) and D = 17 (Dpad 32, ng 1)
         All three rotation modes occur in a full group and in a remainder group (ng 4 / 8 / 12, 2 / 6 / 10, odd; remainders 4, 2, 1 3 5).
  Leg B  block shapes at the default gt (4): every graph at D = 29, 125, 221 (ng 1 | 4 | 4+3), 61 instead of 221 where K < 221:
           j5 64:8 11:4 | j9 64:8 x3 51:12 | j9r20 20-row blocks, MT 1 | j9cap48 47 blocks of 1..30 rows, all 4 k-steps, MT 1 |
           b97r33 33:4 33:8 31:4 (one row in the second row tile) | one64 64:4 | hub | hubr32 | cap (21 blocks of 16..40 k-steps, two at the
           640-column cap; D = 29, 125) | k2048r64 (K = 2048, 35 blocks, two of one row; D = 221).
         `j9` and `hub` also at two larger step sizes (STEP2) at which the run takes >= 2 Lanczos steps while the matrix-core kernel
         stays allowed: planes written by k_lz_update, the shifted epilogue.
  Leg C  the first-order forms on the shipped path (device RNG, follow(): two calls of 24, the oracle on mmw_sketch's blocks):
           j9 <2,1,8,2,4,2> | j9r20 <1,1,4,1,2,2> under the first-order epilogue | j9cap48 KS = 4: one chunk per block | hub 1:4 beside 64:24
         at D = 29, 61, 125, 221 with MMW_MF_GT=4 and D = 221 with MMW_MF_GT=8 (ng 7: <2,2,8,2,2,2> / <1,2,4,1,2,2>), each once with the
         matrix as fp16 hi + lo (MMW_NO_FIRST_A16; F_DUAL_INFO[2] >= nit / 3, [3] == 0, no replay) and once in one fp16 half at a
         smaller step ([3] >= nit / 3).  The counters are the guard: a case that stopped taking its form fails.
  Leg D  the SDDMM's bookkeeping: on the last iterate of every Leg B case every entry of X on the pattern is within
         1e-3 sqrt(X_ii X_jj) of the oracle's (the two-half product's own bound is 3 * 2^-17 = 2.3e-5 of that scale and the iterate's
         error sits at the bars, while an entry that is missing, written twice or put into another slot is off by the entry itself);
         `hub` and `cap` also run 12 iterations of the shipped path with the row sums of X taken from the SDDMM's slabs
         (F_DUAL_INFO[0] > 0) and with MMW_NO_SDDMM_ROWSUMS ([0] == 0).  `cap`'s blocks span five union-tile groups and their
         straddling first tile (desc[6]) decides which block owns an edge.
  Leg E  the LDS-staged kernels on the new shapes: hub, j9 and cap at D = 29 and 125 on fp64 (half-tile), fp64 MMW_FULL_TILE and
         fp32 MMW_NO_MFMA handles; bars as test_blocking_on_mid_size_graphs (1e-9 at tol 1e-12, 1e-5 at tol 1e-7).

The step sizes are not derivable from the shapes: they were found on the device (the rule is written beside each) and DESIGN.md
records the counters each gave.  Every graph reached both first-order forms, so none had to be replaced.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from test_hip_timed_path import FIELDS, compare, compare_calls, follow, oracle_for, run_calls, snapshot

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mfma_graphs as mg  # noqa: E402

pytestmark = pytest.mark.gpu

NIT = 3
# Step sizes.  Synchronous legs (A, B; tol = 1e-7): the largest of 0.2, 0.05, 0.02 at which the last plan of the three iterations still
# allows the matrix-core kernel on every width of the graph (rho = 1.3e-3 ... 3e-3 then, two Lanczos steps from the second iteration on).
ETA_SYNC = {"j5": 0.02, "j9": 0.05, "b97": 0.02, "one64": 0.02, "hub": 0.02, "cap": 0.2, "k2048": 0.2}
STEP2 = {"j9": (0.08, 0.1), "hub": (0.025, 0.03)}  # leg B: larger still, F_EXPM_INFO[1] = 2 and the kernel allowed to the end
ETA_FIRST = {"j9": 0.005, "hub": 0.0025}   # leg C, fp16 hi + lo of the matrix: 0.01 halved until F_DUAL_INFO[2] >= nit / 3
ETA_FIRST16 = {"j9": 0.002, "hub": 0.001}  # leg C, the matrix in one fp16 half: 0.004 halved until F_DUAL_INFO[3] >= nit / 3
ETA_ROWSUMS = 0.04                         # leg D, shipped path (hub: Lanczos steps; cap: 8 of 12 iterations first-order)
ETA_LDS = 0.05                              # leg E (test_blocking_on_mid_size_graphs')


def ragged(ntiles):
    return 32 * ntiles - 3


@functools.lru_cache(maxsize=None)
def uploaded(key, Z, eta, nit, seed):
    """(sketches, oracle) of a synchronous case; the launch-form variants of one (graph, width) share both."""
    state = mg._state(key)
    K = state[0].shape[0]
    rng = np.random.default_rng(seed)
    sk = np.stack([orc.sketch_rows(rng.standard_normal((K, Z))) for _ in range(nit)])
    sk.setflags(write=False)
    o = orc.MMWOracle(nit=nit, eta=eta)
    o.run(Z, state, lambda i, K_, D_: sk[i], keep_trace=True, factor=False)
    return sk, o


_DEVICE_ORACLES = {}


def device_oracle(key):
    """oracle_for behind a cache on (graph, Z, eta, nit, seed, calls): the generator is counter-based, so every handle regenerates the same blocks."""
    def get(sketch, state, Z, nit, eta, seed, calls):
        k = (key, Z, eta, nit, seed, tuple(calls))
        if k not in _DEVICE_ORACLES:
            _DEVICE_ORACLES[k] = oracle_for(sketch, state, Z, nit, eta, seed, calls)
        return _DEVICE_ORACLES[k]
    return get


def figures(got, o, idx):
    """(error of exp(L/2)R, largest error of the other per-iteration fields): printed before compare() asserts."""
    errs = {name: relerr(got[name], o.trace[name][idx]) for name, _ in FIELDS}
    return errs["X_half"], max(v for k, v in errs.items() if k != "X_half")


def sync_run(name, D, eta, monkeypatch, extra=None, leg="", want_ok=True):
    """A fp32 handle on the case under its switches, NIT iterations on uploaded sketches, every one under compare(); returns the last
    snapshot, the oracle and the handle (open)."""
    mg.apply_switches(monkeypatch, name, extra)
    key = mg.state_key(name)
    sk, o = uploaded(key, D, eta, NIT, 1)
    s = _lib.Solver(D, mg.state(name), NIT, eta, rank_radio=1, dtype=_lib.F32)
    s.set_expm(_lib.EXPM_LANCZOS, 16, 1e-7)
    assert s.read(_lib.F_SPMM_KIND)[0] == 3.0, "this case is expected on the matrix-core kernels"
    worst = [0.0, 0.0]
    got = None
    for i in range(NIT):
        s.iterate(1, sk[i])
        got = snapshot(s)
        e = figures(got, o, i)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        print("mfshape leg %s %s D %d eta %g it %d: X_half %.3e others %.3e" % (leg, name, D, eta, i, e[0], e[1]))
        compare(got, o, i, i == NIT - 1, NIT)
    if want_ok:
        assert s.read(_lib.F_SPMM_KIND)[1] == 1.0, "the last plan is expected to allow the matrix-core kernel"
    return got, o, s


# ---- leg A ------------------------------------------------------------------------------------------------------------------
A_WIDTHS = ([("4", ragged(n)) for n in (1, 2, 4, 5, 6, 7, 8)] + [("8", ragged(n)) for n in (5, 6, 7, 8, 9, 11, 13)]
            + [("12", ragged(n)) for n in (9, 10, 11, 12, 13)] + [("4", 256), ("8", 160), ("12", 384), (None, 16), (None, 17)])


@pytest.mark.parametrize("gt,D", A_WIDTHS, ids=["gt%s-D%d" % (g or "default", d) for g, d in A_WIDTHS])
@pytest.mark.parametrize("name", ["hub", "hubr32"])
def test_column_groups_of_the_lanczos_product_and_the_sddmm(name, gt, D, monkeypatch):
    got, o, s = sync_run(name, D, ETA_SYNC["hub"], monkeypatch, {"MMW_MF_GT": gt} if gt else None, leg="A")
    assert s.Dpad == (16 if D == 16 else 32 * ((D + 31) // 32))
    s.close()


# ---- legs B and D -------------------------------------------------------------------------------------------------------------
SMALL_K = ("j5", "b97r33", "one64")
B_CASES = ([(n, d, ETA_SYNC[mg.state_key(n)]) for n in ("j5", "j9", "j9r20", "j9cap48", "b97r33", "one64", "hub", "hubr32") for d in (29, 125, 61 if n in SMALL_K else 221)]
           + [("cap", 29, ETA_SYNC["cap"]), ("cap", 125, ETA_SYNC["cap"]), ("k2048r64", 221, ETA_SYNC["k2048"])]
           + [(n, 125, e) for n in ("j9", "hub") for e in STEP2[n]])


def entrywise_ratio(s, xval, o):
    """max over the pattern of |x_ij - oracle| / sqrt(X_ii X_jj), the diagonal taken from the oracle."""
    ip, ix, dp = s.read_i32(_lib.I_L_INDPTR), s.read_i32(_lib.I_L_INDICES), s.read_i32(_lib.I_DIAG_POS)
    ref = o.trace["xval"][-1]
    diag = ref[dp]
    assert np.all(diag > 0)
    rows = np.repeat(np.arange(s.K), np.diff(ip))
    return float(np.max(np.abs(xval - ref) / np.sqrt(diag[rows] * diag[ix])))


@pytest.mark.parametrize("name,D,eta", B_CASES, ids=["%s-D%d-eta%g" % c for c in B_CASES])
def test_block_shapes_and_every_entry_of_x(name, D, eta, monkeypatch):
    got, o, s = sync_run(name, D, eta, monkeypatch, leg="B")
    if eta in STEP2.get(name, ()):
        info = s.read(_lib.F_EXPM_INFO)
        assert info[1] >= 2, ("the larger step is expected to take two Lanczos steps", info)
    ratio = entrywise_ratio(s, got["xval"], o)
    print("mfshape leg D %s D %d eta %g: largest |x - oracle| / sqrt(X_ii X_jj) %.3e" % (name, D, eta, ratio))
    assert ratio <= 1e-3
    s.close()


ROWSUM_CASES = [("hub", 125), ("cap", 29), ("cap", 125)]


@pytest.mark.parametrize("rowsums", ["slabs", "separate-pass"])
@pytest.mark.parametrize("name,D", ROWSUM_CASES, ids=["%s-D%d" % c for c in ROWSUM_CASES])
def test_row_sums_of_x_from_the_sddmm_slabs(name, D, rowsums, monkeypatch):
    nit = 12
    mg.apply_switches(monkeypatch, name, {"MMW_NO_SDDMM_ROWSUMS": "1"} if rowsums != "slabs" else None)
    state = mg.state(name)
    s = _lib.Solver(D, state, nit, ETA_ROWSUMS, rank_radio=1, dtype=_lib.F32)
    s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)
    assert s.read(_lib.F_SPMM_KIND)[0] == 3.0
    snaps = run_calls(s, [nit], 5)
    info = s.read(_lib.F_DUAL_INFO)
    assert s.read(_lib.F_SPMM_KIND)[1] == 1.0
    o = device_oracle(mg.state_key(name))(s.sketch, state, D, nit, ETA_ROWSUMS, 5, [nit])
    s.close()
    e = figures(snaps[0], o, 0)
    print("mfshape leg D %s D %d %s: info %s X_half %.3e others %.3e" % (name, D, rowsums, info, e[0], e[1]))
    assert (info[0] > 0) if rowsums == "slabs" else (info[0] == 0), info
    compare_calls(snaps, o, nit)


# ---- leg C ------------------------------------------------------------------------------------------------------------------
C_WIDTHS = [("4", 29), ("4", 61), ("4", 125), ("4", 221), ("8", 221)]


@pytest.mark.parametrize("form", ["hi+lo", "one-half"])
@pytest.mark.parametrize("gt,D", C_WIDTHS, ids=["gt%s-D%d" % c for c in C_WIDTHS])
@pytest.mark.parametrize("name", ["j9", "j9r20", "j9cap48", "hub"])
def test_first_order_forms_on_the_shipped_path(name, gt, D, form, monkeypatch):
    nit, n1, seed = 48, 24, 9
    key = mg.state_key(name)
    eta = (ETA_FIRST if form == "hi+lo" else ETA_FIRST16)[key]
    mg.apply_switches(monkeypatch, name, {"MMW_MF_GT": gt, **({"MMW_NO_FIRST_A16": "1"} if form == "hi+lo" else {})})
    mid, end, o, info, replays = follow(mg.state(name), D, nit, n1, eta, seed, rank_radio=1, oracle=device_oracle(key))
    for tag, got, idx in (("mid", mid, 0), ("end", end, 1)):
        e = figures(got, o, idx)
        print("mfshape leg C %s gt %s D %d %s eta %g %s: info %s replays %d X_half %.3e others %.3e" % (name, gt, D, form, eta, tag, info, replays, e[0], e[1]))
    if form == "hi+lo":
        assert info[2] >= nit // 3 and info[3] == 0 and replays == 0, (info, replays)
    else:
        assert info[3] >= nit // 3, info
    compare(mid, o, 0, False, nit)
    compare(end, o, 1, True, nit)


# ---- leg E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handle", ["f64", "f64-full-tile", "f32-no-mfma"])
@pytest.mark.parametrize("D", [29, 125])
@pytest.mark.parametrize("name", ["hub", "j9", "cap"])
def test_lds_staged_kernels_on_the_designed_graphs(name, D, handle, monkeypatch):
    if handle == "f64-full-tile":
        monkeypatch.setenv("MMW_FULL_TILE", "1")
    if handle == "f32-no-mfma":
        monkeypatch.setenv("MMW_NO_MFMA", "1")
    dtype, tol, bar = (_lib.F32, 1e-7, 1e-5) if handle == "f32-no-mfma" else (_lib.F64, 1e-12, 1e-9)
    sk, o = uploaded(mg.state_key(name), D, ETA_LDS, NIT, 1)
    s = _lib.Solver(D, mg.state(name), NIT, ETA_LDS, rank_radio=1, dtype=dtype)
    s.set_expm(_lib.EXPM_LANCZOS, 16, tol)
    assert s.read(_lib.F_BLOCKING)[0] == 1.0
    assert s.read(_lib.F_SPMM_KIND)[0] == (1.0 if handle == "f64-full-tile" else 2.0)
    s.iterate(NIT, sk)
    err = relerr(s.read(_lib.F_XHALF), o.trace["X_half"][-1])
    print("mfshape leg E %s D %d %s: X_half %.3e" % (name, D, handle, err))
    assert err < bar
    s.close()
