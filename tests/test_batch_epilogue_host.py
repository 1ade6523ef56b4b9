"""Host side of the batched epilogue (no GPU): mmw_batch_factor / mmw_batch_round / mmw_batch_round_randv are declared, exported and
bound, a host-only batch refuses them, and the Python layer refuses an unknown `epilogue=` before it touches a device."""
import os
import re

import numpy as np
import pytest

from conftest import RUN_CASES, load_golden, state_from
from sig_sdp_mmw_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mmw_batch_factor", "mmw_batch_round", "mmw_batch_round_randv"]


def test_epilogue_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
        assert name in _lib.EXPORTS, name
        getattr(L, name)
    for ref in ("mmw.py:213-216", "sdp_solver.py:18-107"):  # the reference lines the entries replace are named where they are documented
        assert ref in hdr, ref
    for method in ("factor", "read_factor", "factor_info", "round", "round_randv"):
        assert hasattr(_lib.BatchSolver, method), method
    # one limit, stated once in the header and mirrored by the binding; every sweep instance (K <= 675) fits
    limit = int(re.search(r"#define MMW_BATCH_EPILOGUE_MAX_K (\d+)", hdr).group(1))
    assert _lib.BATCH_EPILOGUE_MAX_K == limit >= 704
    assert int(re.search(r"MMW_F_FACTOR_INFO = (\d+)", hdr).group(1)) == _lib.F_FACTOR_INFO


def test_host_only_batch_refuses_the_epilogue():
    gs = [load_golden("run_" + n) for n in RUN_CASES]
    b = _lib.BatchSolver([int(g["Z"]) for g in gs], [state_from(g) for g in gs], 3, 0.05, device=-1)
    with pytest.raises(_lib.MMWError, match="device -1"):
        b.factor()
    with pytest.raises(_lib.MMWError, match="device -1"):
        b.factor(take=[True] + [False] * (b.B - 1), ranks=[3] * b.B)
    with pytest.raises(_lib.MMWError, match="device -1"):
        b.round(10, np.arange(b.B))
    with pytest.raises(_lib.MMWError):
        b.read_factor(0)
    with pytest.raises(_lib.MMWError):
        b.round_randv(0, 1, 0)
    # the raw entries: negative status and a message, no exception
    L = _lib.lib()
    assert L.mmw_batch_factor(b._h, None, None, None) == -3  # MMW_ERR_STATE
    assert b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_factor(None, None, None, None) < 0
    assert L.mmw_batch_round(b._h, None, 10, 1, None, None, None, None) < 0
    out = np.zeros(4)
    assert L.mmw_batch_round_randv(b._h, 0, 1, 0, _lib._pd(out), 4) == -3
    assert L.mmw_batch_round_randv(b._h, 99, 1, 0, _lib._pd(out), 4) < 0
    b.close()


@pytest.mark.parametrize("value", ["", "device", "Batch", None, 1])
def test_unknown_epilogue_raises_value_error(value):
    g = load_golden("run_" + RUN_CASES[0])
    st = state_from(g)
    with pytest.raises(ValueError, match="epilogue"):
        batch.search_many([st], nit=2, epilogue=value)
    with pytest.raises(ValueError, match="epilogue"):
        batch.run_with_state_many(0, [4], [st], nit=2, epilogue=value)
    with pytest.raises(ValueError, match="epilogue"):
        batch.single(st, epilogue=value)
