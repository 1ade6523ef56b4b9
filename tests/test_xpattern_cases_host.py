"""CPU-only: the cases of tests/helpers/xpattern_cases.py are what test_hip_xpattern_shapes.py takes them for.

That file holds X on the pattern to a float64 evaluation of the handle's own X_half at every row layout of the dense block.  It only
reaches a layout if the width written for it gives that layout, it only meets the unrolled edge loop's remainders if the states have
the rows claimed, and its reference only counts if it is the oracle's x_on_pattern.  A change to make_layout (csrc/expm_engine.h)
or to a generator that moved one of these would leave the device suite green and off the edge; here it is red instead.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, RUN_CASES, load_golden, state_from
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import xpattern_cases as xc  # noqa: E402

DTYPES = [xc.F64, xc.F32]
IDS = [xc.NAME[d] for d in DTYPES]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_width_gives_the_layout_written_beside_it(dtype):
    for D, LPR, G, NCH in xc.WIDTHS[dtype]:
        assert xc.layout(D, dtype) == (LPR, G, NCH, LPR * xc.VEC[dtype]), D
        assert G == (64 // LPR if LPR <= 32 else 1) and NCH == (LPR + 63) // 64
    for table in (xc.TAYLOR_WIDTHS, xc.CHUNK_WIDTHS):
        assert set(table[dtype]) <= {w[0] for w in xc.WIDTHS[dtype]}
    for D in xc.LDS_WIDTHS[dtype]:
        xc.layout(D, dtype)
    with pytest.raises(ValueError):
        xc.layout(512 * xc.VEC[dtype] // 2 + 1, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_widths_reach_every_layout(dtype):
    lprs = {w[1] for w in xc.WIDTHS[dtype] if w[3] == 1}
    assert lprs == {1, 2, 4, 8, 16, 32, 40, 48, 56, 64}
    assert {w[3] for w in xc.WIDTHS[dtype]} == {1, 2, 3, 4}
    assert max(w[0] for w in xc.WIDTHS[dtype]) == 256 * xc.VEC[dtype]  # the widest block the library takes
    # ragged rows (the last lanes of the padded row hold no column) and exact ones both occur
    assert any(-(-w[0] // xc.VEC[dtype]) < w[1] for w in xc.WIDTHS[dtype]) and any(w[0] == w[1] * xc.VEC[dtype] for w in xc.WIDTHS[dtype])
    # the rows no power of two and the chunked ones are the widths of the one-call-of-three test
    assert {xc.layout(D, dtype)[0] for D in xc.CHUNK_WIDTHS[dtype]} == {40, 48, 56, 72, 136, 200, 256}
    assert [xc.layout(D, dtype)[2] for D in xc.TAYLOR_WIDTHS[dtype]] == [1, 3, 4]
    # the LDS-staged kernels' widths end inside, on and one past a 128-byte and a 256-byte tile
    per128 = 128 // (16 // xc.VEC[dtype])
    assert {per128 - 1, per128, per128 + 1, 2 * per128 - 1, 2 * per128, 2 * per128 + 1} <= set(xc.LDS_WIDTHS[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_slot_counts_multiply_to_the_width(dtype):
    for name in xc.GENERIC_STATES + ("journal12",):
        K = xc.state(name)[0].shape[0]
        widths = [w[0] for w in xc.widths_for(name, dtype)] if name != "journal12" else xc.LDS_WIDTHS[dtype]
        for D in widths:
            Z, rr = xc.slots(D)
            assert Z * rr == D and 2 <= Z <= 64 and rr >= 1
            assert Z < K or name == "k3"  # (on K = 3 the slot counts 2 and 3, as csr_cases runs it)
    k3 = [w[0] for w in xc.widths_for("k3", dtype)]
    assert all(D % 2 == 0 or D % 3 == 0 for D in k3) and len(k3) >= 8
    assert {w[1] for w in xc.widths_for("k3", dtype) if w[3] == 1} >= {1, 40, 56, 64} and {w[3] for w in xc.widths_for("k3", dtype)} == {1, 2, 3, 4}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_library_pads_the_rows_as_restated(dtype):
    """A host-only handle (device = -1) reports the padded row make_layout gave it."""
    state = xc.state("er300")
    for D, LPR, G, NCH in xc.WIDTHS[dtype]:
        Z, rr = xc.slots(D)
        s = _lib.Solver(Z, state, xc.NIT, xc.ETA, rank_radio=rr, dtype=dtype, device=-1)
        assert (s.D, s.Dpad) == (D, LPR * xc.VEC[dtype]), D
        s.close()


def test_the_states_have_the_rows_claimed():
    # dense130: row r has 129 - r upper-triangular edges
    p = orc.Pattern(2, xc.state("dense130"))
    up = xc.upper_counts(p.indptr, p.col)
    assert np.array_equal(up, 129 - np.arange(130))
    for G in (1, 2, 4, 8, 16, 32, 64):  # every remainder of the edge loop's step (G rows of a wave x 4 edges in flight), rows past 64 edges
        assert set(up % (4 * G)) == set(range(min(4 * G, 130)))
    assert up.max() > 64 and up[-1] == 0
    # er300: user 5 keeps its diagonal only; other rows than the last end at their diagonal too, and short and long rows occur
    p = orc.Pattern(2, xc.state("er300"))
    up = xc.upper_counts(p.indptr, p.col)
    assert p.indptr[6] - p.indptr[5] == 1 and p.col[p.indptr[5]] == 5
    none = np.flatnonzero(up == 0)
    assert up[-1] == 0 and len(set(none) - {5, 299}) >= 1
    assert set(range(1, 9)) <= set(up) and up.max() > 16
    assert p.E_asso > 0
    # k3: one edge (0, 2), row 1 isolated, no association pairs
    p = orc.Pattern(2, xc.state("k3"))
    assert p.K == 3 and p.nnzL == 5 and p.E_asso == 0 and list(xc.upper_counts(p.indptr, p.col)) == [1, 0, 0]
    # journal12: rows of many lengths for the LDS-staged kernels' entry tables
    p = orc.Pattern(2, xc.state("journal12"))
    assert p.K == 691 and p.E_asso > 0 and xc.upper_counts(p.indptr, p.col).max() >= 8


@pytest.mark.parametrize("name", RUN_CASES)
def test_the_reference_is_the_oracles_x_on_pattern(name):
    g = load_golden("run_" + name)
    p = orc.Pattern(int(g["Z"]), state_from(g))
    for X_half in g["X_half_it"]:
        want = orc.x_on_pattern(p, X_half)
        got = xc.x_from_half(p.indptr, p.col, X_half)
        assert got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), np.max(np.abs(got - want) / np.abs(want))
        # and from the float32 rounding of the block, widened: what a fp32 handle returns
        got32 = xc.x_from_half(p.indptr, p.col, X_half.astype(np.float32))
        assert np.all(np.abs(got32 - want) <= 1e-5 * np.sqrt(np.outer(want[p.diag_pos], want[p.diag_pos])[p.row, p.col]))


def test_the_bounds_are_the_counts_written():
    assert xc.C_GENERIC == {xc.F64: 32, xc.F32: 16} and xc.C_DIAG == 8
    assert xc.UNIT == {xc.F64: 2.0 ** -53, xc.F32: 2.0 ** -24}
    # the LDS-staged kernels: fp64 as the generic ones; fp32 by the tiles of the row, 21 at the widest row of the table
    assert all(xc.c_lds(xc.F64, xc.layout(D, xc.F64)[3]) == 32 for D in xc.LDS_WIDTHS[xc.F64])
    assert [xc.c_lds(xc.F32, xc.layout(D, xc.F32)[3]) for D in xc.LDS_WIDTHS[xc.F32]] == [13, 13, 13, 14, 14, 14, 16, 17, 21]
