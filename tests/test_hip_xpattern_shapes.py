"""X on the pattern at every row layout of the dense block, held to a float64 evaluation of the handle's own X_half.

Every iteration computes X[a,b] = <y_a, y_b> / tr on the fixed pattern (y the rows of X_half = exp(L/2)R, tr = sum ||y_k||^2 / K): the
quantity the DUAL phase reads.  Which instantiation computes it follows from the padded row (make_layout, csrc/expm_engine.h): rows of
at most 32 lanes are powers of two and G = 64 / LPR rows share a wave; wider rows are multiples of 8 lanes (40, 48, 56, 64: NCH 1; then
NCH 2, 3, 4 chunks of a wave).  The handle hands out both sides of the operation (MMW_F_XHALF, MMW_F_XVAL) and rank_radio gives any width
D = Z * rank_radio, so X is compared with xpattern_cases.x_from_half of the X_half the handle returned: the error of the exponential
drops out, and the bound is a count of roundings (xpattern_cases.C_GENERIC, c_lds, C_DIAG) instead of a trajectory bar.

After every iteration of every case (check_iteration):
  off-diagonal  |x_e - ref_e| <= c u sqrt(ref_aa ref_bb)         a dropped lane or column is 1/D of that scale, a mis-paired reduction O(1)
  diagonal      |x_kk - ref_kk| <= 8 u ref_kk                     the row norms and the trace slabs
  symmetry      X - X^T on the pattern is exactly zero            every edge is stored through `mirror`
  running sum   F_XAVG after == F_XAVG before + F_XVAL in the handle's type, bit for bit; unchanged by the last iteration
  continuity    relerr(F_XVAL, the oracle's X on the pattern) under the trajectory bars (1e-9 fp64, 1e-4 fp32)

  Leg G  the generic kernels (MMW_BLOCKING=0: k_sddmm<T, NCH>, norms and trace from k_lz_combine): dense130, er300 and k3 at every width
         of xpattern_cases.WIDTHS; dense130 again under EXPM_TAYLOR (norms from k_rownorm2) at a ragged, a three-chunk and a largest row;
         and one call of three iterations against three calls of one, bit for bit, at the rows that are no power of two and the chunked
         ones (inside a call the running sum moves into the LOSS pass).
  Leg B  the LDS-staged kernels on journal12 (k_sddmm_blk2 on fp64 and on fp32 with MMW_NO_MFMA, k_sddmm_blk with MMW_FULL_TILE) at
         widths that end inside, on and one past a 128-byte and a 256-byte tile.

Before this file k_sddmm took its transposed reduction at every one-chunk row of at least 4 lanes; that reduction pairs lanes LPR/2 and
LPR/4 apart and is only valid for a power of two.  At LPR 40, 48 and 56 (fp64 65 <= D <= 112, fp32 129 <= D <= 224 on the generic
path) the off-diagonal check was red; those rows now take the wave sums in an instantiation of their own, k_sddmm<T, 1, false>
(holds the measured table).

Every case prints its worst normalised errors (in units of u) before it asserts.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import xpattern_cases as xc  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32 = xc.F64, xc.F32


def check_iteration(s, dtype, c_off, before, last, xval_oracle):
    """The five checks on the X the handle just made; returns (worst off-diagonal, worst diagonal error in units of u, failures)."""
    u = xc.UNIT[dtype]
    ip, ix = s.read_i32(_lib.I_L_INDPTR), s.read_i32(_lib.I_L_INDICES)
    diag = s.read_i32(_lib.I_DIAG_POS)
    rows = np.repeat(np.arange(s.K), np.diff(ip))
    xv, after = s.read(_lib.F_XVAL), s.read(_lib.F_XAVG)
    ref = xc.x_from_half(ip, ix, s.read(_lib.F_XHALF))
    fails = []
    assert np.array_equal(ix[diag], np.arange(s.K))
    off = rows != ix
    scale = np.sqrt(ref[diag][rows] * ref[diag][ix])
    e_off = float(np.max(np.abs(xv - ref)[off] / (u * scale[off]))) if off.any() else 0.0
    e_diag = float(np.max(np.abs(xv - ref)[diag] / (u * ref[diag])))
    if not np.all(np.isfinite(xv)):
        fails.append("X is not finite")
    if not e_off <= c_off:
        worst = np.flatnonzero(off)[np.argmax(np.abs(xv - ref)[off] / scale[off])]
        fails.append("off-diagonal: %.3g u > %d u at (%d, %d); %d of %d entries over" % (e_off, c_off, rows[worst], ix[worst],
                                                                                         int(np.sum(np.abs(xv - ref)[off] > c_off * u * scale[off])), int(off.sum())))
    if not e_diag <= xc.C_DIAG:
        fails.append("diagonal: %.3g u > %d u" % (e_diag, xc.C_DIAG))
    X = xc.pattern_csr(ip, ix, xv)
    if (X - X.T).data.any():
        fails.append("X is not symmetric")
    T = xc.NPTYPE[dtype]
    want = before if last else (before.astype(T) + xv.astype(T)).astype(np.float64)
    if not np.array_equal(after, want):
        fails.append("running sum: %d entries differ" % int(np.sum(after != want)))
    err = relerr(xv, xval_oracle)
    if not err < xc.BAR[dtype]:
        fails.append("continuity: %.3g" % err)
    return e_off, e_diag, fails


def run_case(leg, name, dtype, D, c_off, method=_lib.EXPM_LANCZOS, blocking=None, kind=None):
    Z, rr = xc.slots(D)
    LPR, G, NCH, Dpad = xc.layout(D, dtype)
    sk, o = xc.sketches(name, D), xc.oracle(name, D)
    s = _lib.Solver(Z, xc.state(name), xc.NIT, xc.ETA, rank_radio=rr, dtype=dtype)
    try:
        assert s.read(_lib.F_BLOCKING)[0] == blocking, s.read(_lib.F_BLOCKING)
        assert (s.D, s.Dpad) == (D, LPR * xc.VEC[dtype])  # the restated layout is the library's
        s.set_expm(method, 16, xc.TOL[dtype])
        worst, fails = [0.0, 0.0], []
        for i in range(xc.NIT):
            before = s.read(_lib.F_XAVG)
            s.iterate(1, sk[i])
            e_off, e_diag, f = check_iteration(s, dtype, c_off, before, i + 1 == xc.NIT, o.trace["xval"][i])
            worst = [max(worst[0], e_off), max(worst[1], e_diag)]
            fails += ["iteration %d: %s" % (i, m) for m in f]
        if kind is not None:
            assert s.read(_lib.F_SPMM_KIND)[0] == kind, s.read(_lib.F_SPMM_KIND)
    finally:
        s.close()
    print("XPATTERN leg %s %s %s %s D %d LPR %d G %d NCH %d: off-diagonal %.2f u (bound %d), diagonal %.2f u (bound %d)"
          % (leg, xc.NAME[dtype], name, "taylor" if method == _lib.EXPM_TAYLOR else "lanczos", D, LPR, G, NCH, worst[0], c_off, worst[1], xc.C_DIAG))
    assert not fails, fails


def _generic_cases():
    out = []
    for dtype in (F64, F32):
        for name in xc.GENERIC_STATES:
            for D, LPR, G, NCH in xc.widths_for(name, dtype):
                out.append(pytest.param(name, dtype, D, id="%s-%s-D%d-LPR%d-NCH%d" % (xc.NAME[dtype], name, D, LPR, NCH)))
    return out


# ---- Leg G: the generic kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,D", _generic_cases())
def test_generic_sddmm_at_every_row_layout(name, dtype, D, monkeypatch):
    monkeypatch.setenv("MMW_BLOCKING", "0")
    run_case("G", name, dtype, D, xc.C_GENERIC[dtype], blocking=0.0)


@pytest.mark.parametrize("dtype,D", [(dt, D) for dt in (F64, F32) for D in xc.TAYLOR_WIDTHS[dt]],
                         ids=["%s-D%d" % (xc.NAME[dt], D) for dt in (F64, F32) for D in xc.TAYLOR_WIDTHS[dt]])
def test_generic_sddmm_with_the_taylor_paths_row_norms(dtype, D, monkeypatch):
    """EXPM_TAYLOR: the norms and the trace slabs come from k_rownorm2 instead of the Lanczos combination."""
    monkeypatch.setenv("MMW_BLOCKING", "0")
    run_case("G", "dense130", dtype, D, xc.C_GENERIC[dtype], method=_lib.EXPM_TAYLOR, blocking=0.0)


@pytest.mark.parametrize("dtype,D", [(dt, D) for dt in (F64, F32) for D in xc.CHUNK_WIDTHS[dt]],
                         ids=["%s-D%d" % (xc.NAME[dt], D) for dt in (F64, F32) for D in xc.CHUNK_WIDTHS[dt]])
def test_one_call_of_three_iterations_equals_three_calls(dtype, D, monkeypatch):
    """Inside a call the X of an iteration joins the running sum in the next iteration's LOSS pass; between calls in a pass of its own."""
    monkeypatch.setenv("MMW_BLOCKING", "0")
    Z, rr = xc.slots(D)
    sk = xc.sketches("dense130", D)
    got = []
    for calls in ((xc.NIT,), (1,) * xc.NIT):
        s = _lib.Solver(Z, xc.state("dense130"), xc.NIT, xc.ETA, rank_radio=rr, dtype=dtype)
        assert s.read(_lib.F_BLOCKING)[0] == 0.0
        s.set_expm(_lib.EXPM_LANCZOS, 16, xc.TOL[dtype])
        i = 0
        for n in calls:
            s.iterate(n, sk[i:i + n])
            i += n
        got.append((s.read(_lib.F_XVAL), s.read(_lib.F_XAVG)))
        s.close()
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
    assert np.all(np.isfinite(got[0][1])) and got[0][1].any()


# ---- Leg B: the LDS-staged kernels -----------------------------------------------------------------------------------------------
# handle kind -> (type, switches, MMW_F_SPMM_KIND[0] of the kernels it is meant to run on: 2 half tiles, 1 full tiles)
LDS_KINDS = {"f64-half": (F64, {}, 2.0), "f64-full": (F64, {"MMW_FULL_TILE": "1"}, 1.0), "f32-half": (F32, {"MMW_NO_MFMA": "1"}, 2.0)}


@pytest.mark.parametrize("kind,D", [(k, D) for k in LDS_KINDS for D in xc.LDS_WIDTHS[LDS_KINDS[k][0]]],
                         ids=["%s-D%d" % (k, D) for k in LDS_KINDS for D in xc.LDS_WIDTHS[LDS_KINDS[k][0]]])
def test_lds_staged_sddmm_at_the_tile_edges(kind, D, monkeypatch):
    dtype, switches, spmm_kind = LDS_KINDS[kind]
    for k in ("MMW_BLOCKING", "MMW_FULL_TILE", "MMW_NO_MFMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    run_case("B " + kind, "journal12", dtype, D, xc.c_lds(dtype, xc.layout(D, dtype)[3]), blocking=1.0, kind=spmm_kind)
