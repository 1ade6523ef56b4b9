"""CPU-only: the designed graphs of tests/helpers/mfma_graphs.py give the matrix-core blocks their table names, and both blockings
keep their invariants on them.

test_hip_mfma_shapes.py runs these graphs on the device because of their blocks: one-row blocks, blocks of exactly 4 k-steps, a
24-k-step hub block beside them, unions cut by the 640-column cap, a second row tile that holds one row.  A change to
build_mfma_blocking (csrc/blocking.h) that moves one of these shapes would leave the device suite green and silently off the
edge; here it is red instead.  The blocks are read from what a host-only handle (device = -1) reports under MMW_HOST_BLOCKING /
MMW_HOST_BLOCKING_HIST; the invariants are the library's own verifier (MMW_CHECK_BLOCKING).
"""
import os
import re
import sys

import pytest

from conftest import ROOT
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mfma_graphs as mg  # noqa: E402


def host_report(name, monkeypatch, capfd):
    """(usable, ok, blocks, row tiles, k-steps, [(rows, k-steps) per block]) of a host-only fp32 handle on the case."""
    mg.apply_switches(monkeypatch, name, {"MMW_HOST_BLOCKING": "1", "MMW_HOST_BLOCKING_HIST": "1"})
    capfd.readouterr()
    s = _lib.Solver(29, mg.state(name), 3, 0.05, rank_radio=1, dtype=_lib.F32, device=-1)
    s.close()
    err = capfd.readouterr().err
    lds = re.search(r"\[mmw\] host blocking .*: usable (\d) half-tile (\d) blocks (\d+)", err)
    mc = re.search(r"\[mmw\] matrix-core blocking .*: ok (\d) blocks (\d+) .* row tiles (\d+) k-steps (\d+)\n((?:\d+:\d+ )*)\n", err)
    assert lds and mc, err
    hist = [tuple(int(x) for x in b.split(":")) for b in mc.group(5).split()]
    return int(lds.group(1)), int(mc.group(1)), int(mc.group(2)), int(mc.group(3)), int(mc.group(4)), hist


@pytest.mark.parametrize("name", sorted(mg.SHAPES))
def test_designed_graphs_give_the_blocks_their_table_names(name, monkeypatch, capfd):
    usable, ok, nb, mt, ksteps, hist = host_report(name, monkeypatch, capfd)
    want_nb, want_mt, want_ks, want_min, want_max = mg.SHAPES[name]
    assert usable == 1 and ok == 1, "a device handle runs the matrix-core kernels only when both blockings accept the graph"
    assert (nb, mt, ksteps) == (want_nb, want_mt, want_ks), hist
    assert len(hist) == nb and sum(k for _, k in hist) == ksteps
    assert (min(k for _, k in hist), max(k for _, k in hist)) == (want_min, want_max), hist
    assert all(1 <= r <= 32 * mt and k % 4 == 0 for r, k in hist), hist
    rows = [r for r, _ in hist]
    if name in ("hub", "hubr32"):
        assert rows.count(1) == 5 - mt and (2, 4) in hist, hist        # one-row blocks (the rows that hold only their diagonal) ...
        assert (64 // (3 - mt), 24) in hist, hist                   # ... beside the hub's 24-k-step block, in one launch
    if name == "cap":
        assert sorted(r for r, k in hist if k == 40) == [60, 62], hist  # cut by the 640-column cap before they reached 64 rows
        assert hist[-1] == (6, 28), hist
    if name == "j9cap48":
        assert {k for _, k in hist} == {4} and min(rows) == 1 and max(rows) == 30, hist
    if name == "j9r20":
        assert rows == [20] * 12 + [3], hist
    if name == "b97r33":
        assert hist == [(33, 4), (33, 8), (31, 4)], hist           # row 33 of a block is alone in the second row tile
    if name == "one64":
        assert hist == [(64, 4)], hist


def test_the_dense_graph_is_taken_by_the_matrix_core_blocking_only(monkeypatch, capfd):
    """Ten 64:40 blocks, but an LDS-staged blocking without reuse: a device handle runs it on the generic kernels, so it is no
    device case -- and the case on which the verifier used to read SDDMM tables that were never built."""
    usable, ok, nb, mt, ksteps, hist = host_report("dense", monkeypatch, capfd)
    assert (usable, ok, nb, mt, ksteps) == (0, 1, 10, 2, 400) and set(hist) == {(64, 40)}, hist


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(mg.SHAPES) + ["k2048r64", "dense"])
def test_blocking_invariants_on_the_designed_graphs(name, dtype, monkeypatch):
    """The library's verifier on both blockings (and on the matrix-core blocking at 64, 32 and 7 rows per block).  On `dense` the
    LDS-staged blocking is not usable and its SDDMM tables are not built: the verifier skips that section and still checks the
    rest and the matrix-core blocking (it used to index the empty tables)."""
    mg.apply_switches(monkeypatch, name, {"MMW_CHECK_BLOCKING": "1"})
    state = mg.state(name)
    s = _lib.Solver(29, state, 3, 0.05, rank_radio=1, dtype=_lib.F32 if dtype == "f32" else _lib.F64, device=-1)  # MMWError on a violated invariant
    assert s.K == state[0].shape[0]
    s.close()
