"""Host side of the batch's head split (no GPU): the entries and the constants are declared, exported and bound; `head_split=` is a
keyword of the workflows; a host-only batch refuses the setting and still answers the head ranges, which are the row split's rule;
the setters' messages under this setter's name; the rule behind set_head_split("auto")."""
import inspect
import os

import pytest

from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.graphs import journal_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_batch(cells, Zs):
    made = {c: journal_graph(c, 75e-4, 0) for c in set(cells)}
    return _lib.BatchSolver(Zs, [made[c] for c in cells], 3, 0.04, device=-1)


def test_head_split_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_set_head_split(mmw_batch* b, const int32_t* parts);" in hdr
    assert "int mmw_batch_head_ranges(mmw_batch* b, int32_t inst, int32_t parts, int32_t* out);" in hdr
    assert "#define MMW_BATCH_MAX_HEAD_PARTS %d" % _lib.BATCH_MAX_HEAD_PARTS in hdr and _lib.BATCH_MAX_HEAD_PARTS == 64
    assert "MMW_F_HEAD_CALL = %d," % _lib.F_HEAD_CALL in hdr
    # the next free id: no other field holds it, and the split's record kept its own
    ids = [v for k, v in vars(_lib).items() if k.startswith("F_") and isinstance(v, int) and k not in ("F32", "F64")]
    assert ids.count(_lib.F_HEAD_CALL) == 1 and _lib.F_HEAD_CALL == max(ids) and _lib.F_SPLIT_CALL == 22
    L = _lib.lib()
    for name in ("mmw_batch_set_head_split", "mmw_batch_head_ranges"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).restype is _lib.C.c_int
    assert L.mmw_batch_set_head_split.argtypes == L.mmw_batch_set_row_split.argtypes
    assert L.mmw_batch_head_ranges.argtypes == L.mmw_batch_row_ranges.argtypes


def test_head_split_is_a_keyword_of_the_seven_workflows():
    for fn in (batch.search_many, batch.run_with_state_many, batch.convergence_many, batch.online_many, batch.online_resolve_many,
               batch.compare_many, batch.single.__init__):
        par = inspect.signature(fn).parameters
        assert par["head_split"].default is None, fn
        names = list(par)
        assert names.index("head_split") > names.index("row_split") > names.index("split"), fn


def test_host_only_batch_refuses_the_head_split_and_answers_the_ranges():
    b = host_batch([5, 6], [12, 12])
    for parts in (2, [1, 4], "auto", None):
        with pytest.raises(_lib.MMWError, match="device -1"):
            b.set_head_split(parts)
    assert b.head_split_parts is None
    L = _lib.lib()
    assert L.mmw_batch_set_head_split(b._h, None) == -3  # MMW_ERR_STATE
    assert b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_set_head_split(None, None) < 0
    # the record is kept on the host: zeros before any call
    assert b.head_call() == {"on": False, "launches": 0, "widest": 0}
    # the ranges come from the host pattern: the row split's rule, on real patterns
    for i in range(b.B):
        indptr = b.read_i32(i, _lib.I_L_INDPTR)
        for parts in (1, 2, 3, 7, 64):
            got = b.head_ranges(i, parts)
            assert got == _lib.BatchSolver.row_bounds(indptr, parts), (i, parts)
            assert got == b.row_ranges(i, parts)
            assert got[0] == 0 and got[-1] == b.sizes[i]["K"] and all(x <= y for x, y in zip(got, got[1:]))
    for bad in (0, _lib.BATCH_MAX_HEAD_PARTS + 1):
        with pytest.raises(_lib.MMWError, match=r"mmw_batch_head_ranges: parts = %d is outside \[1, 64\]" % bad):
            b.head_ranges(0, bad)
    with pytest.raises(_lib.MMWError):
        b.head_ranges(2, 2)
    b.close()


def test_bad_counts_and_bad_strings_get_the_setters_messages():
    b = host_batch([5, 6], [12, 12])
    with pytest.raises(_lib.MMWError, match="set_head_split: one part count per instance"):
        b.set_head_split([2, 2, 2])
    with pytest.raises(_lib.MMWError, match='set_head_split: parts must be an int, one int per instance, "auto" or None'):
        b.set_head_split("all")
    with pytest.raises(_lib.MMWError, match="set_head_split: parts must be an int"):
        batch._head_split(b, "rows")
    batch._head_split(b, None)  # None: the setter is not called at all
    assert b.head_split_parts is None
    b.close()


def test_suggest_head_split_on_host_sizes():
    # more equal instances than compute units: every share is below one workgroup
    small = host_batch([5] * 320, [12] * 320)
    assert small.suggest_head_split() == [1] * 320
    small.close()
    # one instance alone gets all compute units, clamped by 64 and by ceil(K / 64) parts; it follows `cus`
    for cell, Z in ((15, 45), (9, 32), (5, 12)):
        one = host_batch([cell], [Z])
        K = one.sizes[0]["K"]
        assert one.suggest_head_split() == [min(64, -(-K // 64))]
        assert one.suggest_head_split(cus=3) == [min(3, -(-K // 64))]
        assert one.suggest_head_split(cus=1) == [1]
        one.close()
    # the straggler of a mixed batch gets the most; shares follow nnzL_i, not D_i
    mixed = host_batch([5, 5, 15, 5, 5, 5], [12, 12, 45, 12, 12, 12])
    w = [s["nnzL"] for s in mixed.sizes]
    for cus in (8, 64, 256):
        parts = mixed.suggest_head_split(cus=cus)
        want = [max(1, min(int(round(wi * cus / sum(w))), 64, -(-s["K"] // 64))) for wi, s in zip(w, mixed.sizes)]
        assert parts == want, (cus, parts, want)
        assert parts[2] == max(parts)
    assert mixed.suggest_head_split(cus=64)[2] > 1
    # the column split does not enter the rule
    before = mixed.suggest_head_split()
    mixed.split_parts = [1, 1, 8, 1, 1, 1]
    assert mixed.suggest_head_split() == before
    # an instance that sits out gets 1 and does not weigh
    mixed.active = [True, True, False, True, True, True]
    assert mixed.suggest_head_split(cus=64)[2] == 1
    mixed.close()
