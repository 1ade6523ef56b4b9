"""Host side of the batched solver (no GPU): exported symbols, per-instance state processing equal to mmw_create's, limits."""
import ctypes

import numpy as np
import pytest

from conftest import RUN_CASES, load_golden, state_from
from sig_sdp_mmw_amd import _lib

BATCH_SYMBOLS = ["mmw_batch_create", "mmw_batch_destroy", "mmw_batch_sizes", "mmw_batch_set_slots", "mmw_batch_reset", "mmw_batch_set_eta",
                 "mmw_batch_set_expm", "mmw_batch_iterate", "mmw_batch_read_f64", "mmw_batch_read_i32", "mmw_batch_sketch", "mmw_batch_export"]
IFIELDS = [_lib.I_L_INDPTR, _lib.I_L_INDICES, _lib.I_ST_INDPTR, _lib.I_ST_INDICES, _lib.I_GAIN_X, _lib.I_GAIN_Y, _lib.I_ASSO_X,
           _lib.I_ASSO_Y, _lib.I_DIAG_POS, _lib.I_ASSO_POS]


def test_batch_symbols_are_declared_and_exported():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmw_hip.h")).read()
    L = _lib.lib()
    for name in BATCH_SYMBOLS:
        assert name + "(" in hdr, name
        assert name in _lib.EXPORTS, name
        getattr(L, name)


def golden_batch():
    gs = [load_golden("run_" + n) for n in RUN_CASES]
    return gs, [state_from(g) for g in gs]


def test_host_batch_equals_host_handles():
    gs, states = golden_batch()
    Zs = [int(g["Z"]) for g in gs]
    b = _lib.BatchSolver(Zs, states, [int(g["nit"]) for g in gs], 0.05, device=-1)
    for i, (g, st) in enumerate(zip(gs, states)):
        s = _lib.Solver(Zs[i], st, int(g["nit"]), 0.05, device=-1)
        assert (b.sizes[i]["K"], b.sizes[i]["Z"], b.sizes[i]["D"], b.sizes[i]["nnzL"], b.sizes[i]["C"]) == (s.K, s.Z, s.D, s.nnzL, s.C)
        for f in IFIELDS:
            assert np.array_equal(b.read_i32(i, f), s.read_i32(f)), (i, f)
        for f in (_lib.F_S_SUM, _lib.F_NORM_H, _lib.F_ST_DATA):
            assert np.array_equal(b.read(i, f), s.read(f)), (i, f)
        s.close()
    # a host-only batch holds no iterate
    with pytest.raises(_lib.MMWError):
        b.read(0, _lib.F_Y)
    with pytest.raises(_lib.MMWError):
        b.iterate(1, None, [0] * len(gs))
    b.close()


def test_oversize_instances_are_refused_with_a_message():
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    small = er_contention_graph(60, 0.1, 1)
    # D = Z * rank_radio over the batch limit (512)
    with pytest.raises(_lib.MMWError, match="D = 600 exceeds the batch limit"):
        _lib.BatchSolver([300], [small], 5, 0.05, device=-1)
    # K over the batch limit (4096)
    big = er_contention_graph(4200, 0.0005, 2)
    with pytest.raises(_lib.MMWError, match="K = 4200 exceeds the batch limit"):
        _lib.BatchSolver([4, 4], [small, big], 5, 0.05, device=-1)
    # the raw entry: negative status, message set, no exception, *out stays NULL
    L = _lib.lib()
    h = ctypes.c_void_p()
    one = np.array([1], dtype=np.int32)
    rc = L.mmw_batch_create(ctypes.byref(h), -1, 0, _lib._pi(one), _lib._pi(one), 2, 0.05, _lib._pi(one), None, None, None, None, None, None, None)
    assert rc < 0 and not h.value
    assert b"mmw_batch_create" in L.mmw_last_error()


BATCH_MAX_BYTES = 96 << 20  # kernels_batch.h


def batch_instance_bytes(p, D):
    """Arena bytes of one instance as BatchCore::fp64_words / int_words count them (csrc/batch_core.h), from the oracle's pattern."""
    K, nnz, C, EA = p.K, p.nnzL, p.C, p.E_asso
    return (5 * nnz + 6 * K + 4 * C + 4 * K * D + 4 + 64) * 8 + (K + 1 + 3 * nnz + K + EA) * 4


def test_arena_bytes_limit_refuses_just_over_and_accepts_just_under():
    """K = 4 096 (the K limit) and D = 512 (the D limit): an ER density of 0.0187 puts the instance 6 152 bytes over 96 MiB, and the
    same graph at Z = 255 (D = 510) 255 992 bytes under it.  The nnzL <= 2^22 limit cannot fire first at K <= 4 096: 2^22 pattern
    entries alone take 52 bytes each in the arena (5 fp64 and 3 int32 words), 218 MB, far over 96 MiB, so every instance that reaches
    it has already been refused by the byte count."""
    from oracle import mmw_oracle as orc
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    assert 52 * (1 << 22) > BATCH_MAX_BYTES
    state = er_contention_graph(4096, 0.0187, 1)
    p = orc.Pattern(256, state)
    over, under = batch_instance_bytes(p, 512), batch_instance_bytes(p, 510)
    # conditions on the inputs: just over at D = 512, just under at D = 510, both far below the nnzL limit
    assert 0 < over - BATCH_MAX_BYTES < 1 << 20 and 0 < BATCH_MAX_BYTES - under < 1 << 20, (over, under)
    assert p.nnzL < 1 << 22
    with pytest.raises(_lib.MMWError, match="instance 0: instance needs %d bytes, over the batch limit %d" % (over, BATCH_MAX_BYTES)):
        _lib.BatchSolver([256], [state], 5, 0.05, device=-1)
    # a second instance that is fine does not hide the first's refusal, and the index names the one that is over
    small = er_contention_graph(60, 0.1, 1)
    with pytest.raises(_lib.MMWError, match="instance 1: instance needs %d bytes" % over):
        _lib.BatchSolver([4, 256], [small, state], 5, 0.05, device=-1)
    b = _lib.BatchSolver([255], [state], 5, 0.05, device=-1)
    assert (b.sizes[0]["K"], b.sizes[0]["D"], b.sizes[0]["nnzL"], b.sizes[0]["C"]) == (4096, 510, p.nnzL, p.C)
    b.close()


def test_host_only_batch_refuses_set_slots_and_bad_expm_settings():
    gs, states = golden_batch()
    b = _lib.BatchSolver([int(g["Z"]) for g in gs], states, 3, 0.05, device=-1)
    with pytest.raises(_lib.MMWError):
        b.set_slots([4] * len(gs), 3)  # host-only batch: no iterate to reset
    with pytest.raises(_lib.MMWError):
        b.set_expm(17, 1e-9)
    b.close()
