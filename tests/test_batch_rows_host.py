"""Host side of the batch's row split (no GPU): the entries are declared, exported and bound; a host-only batch refuses the setting
and still answers the row ranges; the boundary rule on hand-made indptrs (rows without entries, K < rows, rows = 1, one dense row) is a
cover of [0, K) with every part at most ceil(nnzL / rows) entries plus the longest row; the rule behind set_row_split("auto")."""
import inspect
import os

import numpy as np
import pytest

from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.graphs import journal_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_batch(cells, Zs):
    made = {c: journal_graph(c, 75e-4, 0) for c in set(cells)}
    return _lib.BatchSolver(Zs, [made[c] for c in cells], 3, 0.04, device=-1)


def test_row_split_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_set_row_split(mmw_batch* b, const int32_t* rows);" in hdr
    assert "int mmw_batch_row_ranges(mmw_batch* b, int32_t inst, int32_t rows, int32_t* out);" in hdr
    assert "#define MMW_BATCH_MAX_ROW_PARTS %d" % _lib.BATCH_MAX_ROW_PARTS in hdr
    assert "MMW_F_SPLIT_CALL = %d," % _lib.F_SPLIT_CALL in hdr
    L = _lib.lib()
    p_i32 = type(L.mmw_batch_set_split.argtypes[1])
    for name in ("mmw_batch_set_row_split", "mmw_batch_row_ranges"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).restype is _lib.C.c_int
    assert L.mmw_batch_set_row_split.argtypes == [_lib.C.c_void_p, L.mmw_batch_set_split.argtypes[1]]
    assert L.mmw_batch_row_ranges.argtypes == [_lib.C.c_void_p, _lib.C.c_int32, _lib.C.c_int32, L.mmw_batch_set_split.argtypes[1]]
    assert p_i32 is not None
    for fn in (batch.search_many, batch.run_with_state_many, batch.convergence_many, batch.online_many, batch.compare_many, batch.single.__init__):
        assert inspect.signature(fn).parameters["row_split"].default is None, fn


def test_host_only_batch_refuses_the_row_split_and_answers_the_ranges():
    b = host_batch([5, 6], [12, 12])
    for rows in (2, [1, 4], "auto", None):
        with pytest.raises(_lib.MMWError, match="device -1"):
            b.set_row_split(rows)
    assert b.row_split_parts is None
    L = _lib.lib()
    assert L.mmw_batch_set_row_split(b._h, None) == -3  # MMW_ERR_STATE
    assert b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_set_row_split(None, None) < 0
    with pytest.raises(_lib.MMWError, match="one part count per instance"):
        b.set_row_split([2, 2, 2])
    # a bad string: the message of the other setters, under this one's name
    with pytest.raises(_lib.MMWError, match='set_row_split: parts must be an int, one int per instance, "auto" or None'):
        b.set_row_split("all")
    with pytest.raises(_lib.MMWError, match="set_row_split: parts must be an int"):
        batch._row_split(b, "rows")
    # the ranges come from the host pattern: the library's boundaries are the rule's, on real patterns
    for i in range(b.B):
        indptr = b.read_i32(i, _lib.I_L_INDPTR)
        for rows in (1, 2, 3, 7, 64):
            got = b.row_ranges(i, rows)
            assert got == _lib.BatchSolver.row_bounds(indptr, rows), (i, rows)
            check_cover(indptr, rows, got)
    for bad in (0, _lib.BATCH_MAX_ROW_PARTS + 1):
        with pytest.raises(_lib.MMWError, match="outside"):
            b.row_ranges(0, bad)
    with pytest.raises(_lib.MMWError):
        b.row_ranges(2, 2)
    b.close()


def check_cover(indptr, rows, bd):
    """contiguous, ordered, a cover of [0, K); every part holds at most ceil(nnzL / rows) entries plus the longest row"""
    indptr = [int(x) for x in indptr]
    K, nnz = len(indptr) - 1, indptr[-1]
    assert len(bd) == rows + 1 and bd[0] == 0 and bd[-1] == K
    assert all(a <= b for a, b in zip(bd, bd[1:]))
    longest = max([indptr[k + 1] - indptr[k] for k in range(K)] + [0])
    for p in range(rows):
        assert indptr[bd[p + 1]] - indptr[bd[p]] <= -(-nnz // rows) + longest, (p, bd)


def indptr_of(lengths):
    return [0] + [int(x) for x in np.cumsum(lengths)]


def test_row_bounds_by_hand():
    rb = _lib.BatchSolver.row_bounds
    # equal rows: equal parts
    assert rb(indptr_of([2] * 8), 4) == [0, 2, 4, 6, 8]
    assert rb(indptr_of([2] * 8), 1) == [0, 8]
    # rows not dividing K: boundary p is the first row whose prefix reaches p nnzL / rows (10 p / 3: 4 and 7 entries -> rows 2 and 4)
    assert rb(indptr_of([2] * 5), 3) == [0, 2, 4, 5]
    # K < rows: ranges of one row, then empty ones
    assert rb(indptr_of([1, 1]), 3) == [0, 1, 2, 2]
    assert rb(indptr_of([3]), 4) == [0, 1, 1, 1, 1]
    # rows without entries, at the front, inside and at the end: 6 entries in rows 1, 3, 4
    ip = indptr_of([0, 2, 0, 2, 2, 0])
    assert rb(ip, 3) == [0, 2, 4, 6]
    assert rb(ip, 1) == [0, 6]
    # nnzL = 0: every boundary but the last is 0, the last part owns all rows
    assert rb(indptr_of([0, 0, 0]), 2) == [0, 0, 3]
    # one row with more than half of the entries: the parts that would start inside it are empty
    dense = indptr_of([1, 1, 20, 1, 1])
    assert rb(dense, 6) == [0, 3, 3, 3, 3, 3, 5]
    for ip_, rows in ((ip, 3), (dense, 6), (dense, 64), (indptr_of([2] * 5), 3), (indptr_of([0, 0, 0]), 2), (indptr_of([3]), 4)):
        check_cover(ip_, rows, rb(ip_, rows))
    # a star graph of K = 65 (hub row 0 with 65 entries, 64 leaves with 2): the hub's part stands alone, the next four are empty
    star = indptr_of([65] + [2] * 64)
    bd = rb(star, 16)
    check_cover(star, 16, bd)
    assert bd[:7] == [0, 1, 1, 1, 1, 1, 5], bd


def test_suggest_row_split_on_host_sizes():
    # more equal instances than compute units: every share is below one workgroup
    small = host_batch([5] * 320, [12] * 320)
    assert small.suggest_row_split() == [1] * 320
    small.close()
    # one instance alone gets all compute units: ceil(256 / G) rows with G = 1 slice, clamped by ceil(K / 64) rows
    for cell, Z in ((15, 45), (9, 32), (5, 12)):
        one = host_batch([cell], [Z])
        K = one.sizes[0]["K"]
        assert one.suggest_row_split() == [min(64, -(-K // 64))]
        assert one.suggest_row_split(cus=3) == [min(3, -(-K // 64))]
        assert one.suggest_row_split(cus=1) == [1]
        one.close()
    # the straggler of a mixed batch gets the rows; shares follow w_i = nnzL_i D_i
    mixed = host_batch([5, 5, 15, 5, 5, 5], [12, 12, 45, 12, 12, 12])
    w = [s["nnzL"] * s["D"] for s in mixed.sizes]
    for cus in (8, 64, 256):
        rows = mixed.suggest_row_split(cus=cus)
        want = [max(1, min(int(round(wi * cus / sum(w))), 64, -(-s["K"] // 64))) for wi, s in zip(w, mixed.sizes)]
        assert rows == want, (cus, rows, want)
        assert rows[2] == max(rows)
    # with column slices G the rows are the share divided by G, rounded up
    mixed.split_parts = [1, 1, 8, 1, 1, 1]  # (a host-only batch takes no setting: what set_split would have recorded)
    G = _lib.BatchSolver.split_slices(mixed.sizes[2]["D"], 8)[1]
    share = int(round(w[2] * 256 / sum(w)))
    assert mixed.suggest_row_split()[2] == max(1, min(-(-share // G), 64, -(-675 // 64)))
    mixed.close()
