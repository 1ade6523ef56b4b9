"""Host side of the batch factor's split (no GPU): the entry is declared, exported and bound; the workflows carry the keyword; a
host-only batch refuses the setting; the partition of a round's row pairs into items; the rule behind set_factor_split("auto")."""
import inspect
import os
import re

import pytest

from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_batch(states, Zs):
    return _lib.BatchSolver(Zs, states, 3, 0.04, device=-1)


def test_factor_split_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_set_factor_split(mmw_batch* b, const int32_t* parts);" in hdr
    assert int(re.search(r"MMW_F_FACTOR_CALL = (\d+)", hdr).group(1)) == _lib.F_FACTOR_CALL
    assert "mmw_batch_set_factor_split" in _lib.EXPORTS
    getattr(_lib.lib(), "mmw_batch_set_factor_split")
    for fn in (batch.search_many, batch.run_with_state_many, batch.online_many, batch.compare_many, batch.single.__init__):
        assert inspect.signature(fn).parameters["factor_split"].default is None, fn


def test_host_only_batch_refuses_the_factor_split():
    b = host_batch([journal_graph(5, 75e-4, 0), journal_graph(6, 75e-4, 0)], [12, 12])
    for parts in (2, [1, 4], "auto", None):
        with pytest.raises(_lib.MMWError, match="device -1"):
            b.set_factor_split(parts)
    assert b.factor_split_parts is None
    L = _lib.lib()
    assert L.mmw_batch_set_factor_split(b._h, None) == -3  # MMW_ERR_STATE
    assert b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_set_factor_split(None, None) < 0
    with pytest.raises(_lib.MMWError):
        b.set_factor_split([2, 2, 2])  # one count per instance
    with pytest.raises(_lib.MMWError):
        b.set_factor_split("all")
    assert b.factor_split_parts is None
    assert b.factor_call() == {"path": 0, "launches": 0, "sweeps": 0, "widest": 0}  # no factor call yet
    b.close()


def test_factor_split_needs_the_batch_epilogue():
    st = [er_contention_graph(5, 0.5, 1)]
    for fs in (2, "auto", [3]):
        with pytest.raises(ValueError, match="factor_split"):
            batch.search_many(st, nit=2, epilogue="handle", factor_split=fs)
        with pytest.raises(ValueError, match="factor_split"):
            batch.run_with_state_many(0, [3], st, nit=2, factor_split=fs)
        with pytest.raises(ValueError, match="factor_split"):
            batch.single(st[0], nit=2, epilogue="handle", factor_split=fs)


@pytest.mark.parametrize("K", [2, 3, 5, 31, 32, 33, 34, 64, 65, 675, 1023, 1024])
@pytest.mark.parametrize("parts", [1, 2, 3, 7, 32])
def test_factor_items(K, parts):
    P = -(-(K + (K & 1)) // 2)
    items = _lib.BatchSolver.factor_items(K, parts)
    assert 1 <= len(items) <= parts
    assert len(items) == -(-P // -(-P // parts))
    at = 0
    for p0, n in items:  # contiguous and non-empty: 0 ... P - 1 exactly once
        assert p0 == at and 1 <= n <= -(-P // parts)
        at += n
    assert at == P


def test_suggest_factor_split_on_host_sizes():
    b = host_batch([er_contention_graph(K, 0.2, 1) for K in (2, 31, 32, 33)] + [journal_graph(15, 75e-4, 0), er_contention_graph(1024, 0.01, 4)],
                   [2, 4, 4, 4, 45, 8])
    assert [s["K"] for s in b.sizes] == [2, 31, 32, 33, 675, 1024]
    assert b.suggest_factor_split() == [1, 1, 1, 2, 22, 32]
    b.active[4] = False  # an instance that sits out
    assert b.suggest_factor_split() == [1, 1, 1, 2, 1, 32]
    b.close()
