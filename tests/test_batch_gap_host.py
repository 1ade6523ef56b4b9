"""Host side of the batched solver's duality-gap log (no GPU): the two entries are declared, exported and bound; a host-only batch
refuses them; the arena accounting of the batch (sizes, the 96 MiB-per-instance limit) is what it was before the gap existed."""
import os

import numpy as np
import pytest

from conftest import RUN_CASES, load_golden, state_from
from sig_sdp_mmw_amd import _lib

GAP_SYMBOLS = ["mmw_batch_set_gap", "mmw_batch_read_gap"]
BATCH_MAX_BYTES = 96 << 20  # kernels_batch.h


def test_gap_symbols_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmw_hip.h")).read()
    L = _lib.lib()
    for name in GAP_SYMBOLS:
        assert name + "(" in hdr, name
        assert name in _lib.EXPORTS, name
        getattr(L, name)
    assert "mmw.py:79-117" in hdr  # the reference lines the entries replace are named where they are documented
    assert hasattr(_lib.BatchSolver, "set_gap") and hasattr(_lib.BatchSolver, "gap_log")
    from sig_sdp_mmw_amd import batch
    assert callable(batch.convergence_many)


def test_host_only_batch_refuses_the_gap():
    gs = [load_golden("run_" + n) for n in RUN_CASES]
    b = _lib.BatchSolver([int(g["Z"]) for g in gs], [state_from(g) for g in gs], 3, 0.05, device=-1)
    with pytest.raises(_lib.MMWError, match="device -1"):
        b.set_gap(True)
    with pytest.raises(_lib.MMWError, match="device -1"):
        b.set_gap(False, 10)
    with pytest.raises(_lib.MMWError):
        b.gap_log(0)
    # the raw entries: negative status and a message, no exception
    L = _lib.lib()
    out = np.zeros(4)
    assert L.mmw_batch_set_gap(b._h, 1, 0) < 0
    assert b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_read_gap(b._h, 0, _lib._pd(out), 0) < 0
    assert L.mmw_batch_read_gap(b._h, 99, _lib._pd(out), 0) < 0
    assert L.mmw_batch_set_gap(None, 1, 0) < 0 and L.mmw_batch_read_gap(None, 0, _lib._pd(out), 4) < 0
    b.close()


def batch_instance_bytes(p, D):
    """Arena bytes of one instance as tests/test_batch_host.py counts them: the gap's work space is not part of the arena."""
    K, nnz, C, EA = p.K, p.nnzL, p.C, p.E_asso
    return (5 * nnz + 6 * K + 4 * C + 4 * K * D + 4 + 64) * 8 + (K + 1 + 3 * nnz + K + EA) * 4


def test_sizes_and_the_arena_limit_did_not_move():
    from oracle import mmw_oracle as orc
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    state = er_contention_graph(4096, 0.0187, 1)
    p = orc.Pattern(256, state)
    over, under = batch_instance_bytes(p, 512), batch_instance_bytes(p, 510)
    assert 0 < over - BATCH_MAX_BYTES < 1 << 20 and 0 < BATCH_MAX_BYTES - under < 1 << 20, (over, under)
    with pytest.raises(_lib.MMWError, match="instance 0: instance needs %d bytes, over the batch limit %d" % (over, BATCH_MAX_BYTES)):
        _lib.BatchSolver([256], [state], 5, 0.05, device=-1)
    b = _lib.BatchSolver([255], [state], 5, 0.05, device=-1)
    assert (b.sizes[0]["K"], b.sizes[0]["D"], b.sizes[0]["nnzL"], b.sizes[0]["C"]) == (4096, 510, p.nnzL, p.C)
    with pytest.raises(_lib.MMWError):
        b.set_gap(True)
    b._load_sizes()  # a refused set_gap leaves the sizes alone
    assert (b.sizes[0]["K"], b.sizes[0]["D"], b.sizes[0]["nnzL"], b.sizes[0]["C"], b.sizes[0]["iter"]) == (4096, 510, p.nnzL, p.C, 0)
    b.close()
    gs = [load_golden("run_" + n) for n in RUN_CASES]
    Zs = [int(g["Z"]) for g in gs]
    b = _lib.BatchSolver(Zs, [state_from(g) for g in gs], [int(g["nit"]) for g in gs], 0.05, device=-1)
    for i, g in enumerate(gs):
        s = _lib.Solver(Zs[i], state_from(g), int(g["nit"]), 0.05, device=-1)
        assert (b.sizes[i]["K"], b.sizes[i]["Z"], b.sizes[i]["D"], b.sizes[i]["nnzL"], b.sizes[i]["C"]) == (s.K, s.Z, s.D, s.nnzL, s.C)
        s.close()
    b.close()
