"""The device CSR entry point on the host (device = -1, no HIP call): mmw_csr_* keep host copies, mmw_csr_bounds and the validation of
mmw_create_from_csr run the very `__host__ __device__` statements the kernels run (csrc/pattern_csr_device.h: csr_check_row,
csr_lower) in a plain loop, and the handle is mmw_create's.  The cases are tests/helpers/csr_cases.py's, shared with the GPU tests."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import csr_cases as cc  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation  # noqa: E402

NEW = ["mmw_csr_upload", "mmw_csr_wrap", "mmw_csr_destroy", "mmw_csr_sizes", "mmw_csr_pointers", "mmw_csr_state", "mmw_csr_bounds", "mmw_create_from_csr"]


def test_symbols_are_exported_and_listed():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n


@pytest.mark.parametrize("name", list(cc.CASES))
def test_upload_round_trips_the_seven_arrays(name):
    state, _ = cc.case(name)
    K, want = _lib._state_arrays(state)
    c = _lib.DeviceCSR.upload(state, device=-1)
    assert (c.K, c.nnzS, c.nnzQ) == (K, want[1].size, want[4].size)
    S, Q, h = c.state()
    got = (S.indptr, S.indices, S.data, Q.indptr, Q.indices, Q.data, h)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert c.pointers() == [0] * 7  # nothing lies on a device
    c.close()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_bounds_are_the_host_set_bounds(name):
    state, _ = cc.case(name)
    c = _lib.DeviceCSR.upload(state, device=-1)
    assert c.bounds() == tuple(int(x) for x in binary_search_relaxation().set_bounds(state))
    assert binary_search_relaxation().set_bounds(c.device_state()) == c.bounds()
    c.close()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_handle_from_csr_is_the_handle_from_the_state(name):
    state, Z = cc.case(name)
    a = _lib.Solver(Z, state, 3, 0.04, device=-1)
    for k, v in cc.EXPECTED_SIZES.get(name, {}).items():
        assert getattr(a, k) == v, k  # (the shapes the cases were chosen for, accepted by the host build)
    c = _lib.DeviceCSR.upload(state, device=-1)
    b = _lib.Solver.from_csr(c, Z, 3, 0.04)
    cc.assert_same_pattern(a, b)
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("kind", list(cc.MALFORMED))
def test_malformed_input_is_refused_in_mmw_creates_words(kind):
    """One of each kind of §2's list that a K = 6 state can show (a pattern beyond int32 needs 2^31 entries).  The words are the ones
    mmw_create answers the same arrays with; indptr[K] != nnz is the kind only this entry point can see."""
    K, Z, arrays = cc.malformed(kind)
    words = cc.MALFORMED[kind]
    if kind != "indptr_end":
        said = cc.mmw_create_message(K, Z, arrays)
        assert said is not None and words in said, said
    c = _lib.DeviceCSR.upload_arrays(K, arrays, device=-1)
    with pytest.raises(_lib.MMWError) as ei:
        _lib.Solver.from_csr(c, Z, 3, 0.04)
    assert words in str(ei.value), str(ei.value)
    c.close()


def test_the_valid_state_behind_the_malformed_ones_is_accepted():
    arrays = cc.valid6()
    assert cc.mmw_create_message(6, 3, arrays) is None
    c = _lib.DeviceCSR.upload_arrays(6, arrays, device=-1)
    b = _lib.Solver.from_csr(c, 3, 3, 0.04)
    assert b.K == 6 and b.E_asso == 2
    b.close(); c.close()


def test_first_error_is_the_lowest_class_then_row():
    """Two spoiled fields: a Q diagonal in row 0 (class 6) and an unsorted S row further down (class 4): the unsorted row is reported.
    Two unsorted rows: the message is the same, and an out-of-range column anywhere wins over both."""
    K, Z, arrays = cc.malformed("q_diagonal")
    sp, si = arrays[0], arrays[1]
    row = max(k for k in range(6) if sp[k + 1] - sp[k] >= 2)
    si[sp[row]], si[sp[row] + 1] = si[sp[row] + 1], si[sp[row]]
    c = _lib.DeviceCSR.upload_arrays(K, arrays, device=-1)
    with pytest.raises(_lib.MMWError, match="S_gain must be canonical CSR"):
        _lib.Solver.from_csr(c, Z, 3, 0.04)
    with pytest.raises(_lib.MMWError, match="S_gain must be canonical CSR"):
        c.bounds()  # the bounds read columns as addresses too: same verdict first
    c.close()
    arrays[4][arrays[3][2]] = 77  # Q row 2: column out of range
    c = _lib.DeviceCSR.upload_arrays(K, arrays, device=-1)
    with pytest.raises(_lib.MMWError, match="Q_asso column index out of range"):
        _lib.Solver.from_csr(c, Z, 3, 0.04)
    c.close()


def test_wrap_refuses_what_it_cannot_borrow():
    with pytest.raises(_lib.MMWError, match="int64"):
        class T:  # a tensor-like with int64 indices
            dtype = "torch.int64"
            def data_ptr(self): return 4096
            def numel(self): return 3
        _lib.DeviceCSR.wrap(T(), 0, 0, 4096, 0, 0, 4096, K=2, nnzS=0, nnzQ=0)
    with pytest.raises(_lib.MMWError, match="null address"):
        _lib.DeviceCSR.wrap(4096, 0, 0, 4096, 0, 0, 4096, K=2, nnzS=1, nnzQ=0)
    with pytest.raises(_lib.MMWError, match="nnzS is needed"):
        _lib.DeviceCSR.wrap(4096, 4096, 4096, 4096, 0, 0, 4096, K=2)
    with pytest.raises(_lib.MMWError, match="device -1"):
        _lib.DeviceCSR.wrap(4096, 0, 0, 4096, 0, 0, 4096, K=2, nnzS=0, nnzQ=0, device=-1)
