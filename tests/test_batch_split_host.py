"""Host side of the batch's split mode (no GPU): the entry is declared, exported and bound; a host-only batch refuses it; the rule
behind set_split("auto") respects its clamps; the column-slice arithmetic (D, parts) -> (W, G)."""
import os

import pytest

from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import journal_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_batch(cells, Zs):
    made = {c: journal_graph(c, 75e-4, 0) for c in set(cells)}
    return _lib.BatchSolver(Zs, [made[c] for c in cells], 3, 0.04, device=-1)


def test_split_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_set_split(mmw_batch* b, const int32_t* parts);" in hdr
    assert "#define MMW_BATCH_MAX_PARTS %d" % _lib.BATCH_MAX_PARTS in hdr
    assert "mmw_batch_set_split" in _lib.EXPORTS
    getattr(_lib.lib(), "mmw_batch_set_split")
    from sig_sdp_mmw_amd import batch
    import inspect
    for fn in (batch.search_many, batch.run_with_state_many, batch.convergence_many, batch.online_many, batch.compare_many, batch.single.__init__):
        assert inspect.signature(fn).parameters["split"].default is None, fn


def test_host_only_batch_refuses_the_split():
    b = host_batch([5, 6], [12, 12])
    for parts in (2, [1, 4], "auto", None):
        with pytest.raises(_lib.MMWError, match="device -1"):
            b.set_split(parts)
    assert b.split_parts is None
    L = _lib.lib()
    assert L.mmw_batch_set_split(b._h, None) == -3  # MMW_ERR_STATE
    assert b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_set_split(None, None) < 0
    with pytest.raises(_lib.MMWError):
        b.set_split([2, 2, 2])  # one count per instance
    with pytest.raises(_lib.MMWError):
        b.set_split("all")
    b.close()


def clamps_hold(b, parts):
    assert len(parts) == b.B
    for p, s in zip(parts, b.sizes):
        assert 1 <= p <= min(_lib.BATCH_MAX_PARTS, -(-s["D"] // 8)), (p, s)


def test_suggest_split_on_host_sizes():
    # an all-small batch (more equal instances than compute units: every share is below one workgroup)
    small = host_batch([5] * 320, [12] * 320)
    assert small.suggest_split() == [1] * 320
    assert small.suggest_split(cus=304) == [1] * 320
    small.close()
    # one K = 675 instance among cell-5 ones is the straggler: it gets the largest share
    mixed = host_batch([5, 5, 15, 5, 5, 5], [12, 12, 45, 12, 12, 12])
    assert mixed.sizes[2]["K"] == 675
    for cus in (64, 256, 304):
        parts = mixed.suggest_split(cus=cus)
        clamps_hold(mixed, parts)
        assert parts[2] == max(parts) > 1 and all(p < parts[2] for i, p in enumerate(parts) if i != 2), parts
    # the column cap: D = 90 allows 12 slices however many compute units are offered
    assert mixed.suggest_split(cus=100000)[2] == 12
    mixed.close()
    # the sweep's range of sizes, and the clamp at MMW_BATCH_MAX_PARTS
    sweep = host_batch(list(range(5, 16)) * 2, [12, 14, 16, 20, 24, 28, 32, 36, 40, 42, 45] * 2)
    clamps_hold(sweep, sweep.suggest_split())
    clamps_hold(sweep, sweep.suggest_split(cus=8))
    sweep.close()
    wide = host_batch([15], [200])
    assert wide.sizes[0]["D"] == 400
    assert wide.suggest_split() == [_lib.BATCH_MAX_PARTS]
    wide.close()


# (D, parts) -> (W, G) of the cases of tests/test_hip_batch_split.py, which compares every slice's result on the GPU
SLICES = [((4, 4), (8, 1)), ((3, 2), (8, 1)), ((80, 16), (8, 10)), ((64, 3), (24, 3)), ((170, 7), (32, 6)), ((257, 16), (24, 11)),
          ((24, 2), (16, 2)), ((512, 32), (16, 32)), ((512, 1), (512, 1)), ((7, 32), (8, 1)), ((9, 32), (8, 2))]


@pytest.mark.parametrize("arg,want", SLICES)
def test_column_slices(arg, want):
    D, parts = arg
    W, G = _lib.BatchSolver.split_slices(D, parts)
    assert (W, G) == want
    assert W % 8 == 0 and 1 <= G <= parts and (G - 1) * W < D <= G * W
