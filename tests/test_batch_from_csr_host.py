"""mmw_batch_create_from_csr without a GPU: the symbol, the host-only form (every state with device = -1) against
mmw_batch_create(device = -1) on the same arrays, the validation's words by instance, the refusals that need no device, and the
routing of the batch workflows on stubs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import csr_cases as cc  # noqa: E402
from sig_sdp_mmw_amd import _lib, batch  # noqa: E402

NIT, ETA = 3, 0.04
NAMES = list(cc.CASES)


def test_symbol_is_declared_exported_and_wrapped():
    txt = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_create_from_csr(mmw_batch** out, int32_t B, mmw_csr* const* csr, const int32_t* Z" in txt
    assert "mmw_batch_create_from_csr" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "mmw_batch_create_from_csr")
    assert callable(getattr(_lib.BatchSolver, "from_csr", None))
    for n in ("kernels_batch_csr_pattern.h", "batch_from_csr.h"):
        assert os.path.exists(os.path.join(ROOT, "sig_sdp_mmw_amd", "csrc", n)), n


def test_host_only_batch_of_every_case_is_mmw_batch_creates():
    states = [cc.case(n)[0] for n in NAMES]
    Zs = [cc.case(n)[1] for n in NAMES]
    csrs = [_lib.DeviceCSR.upload(s, device=-1) for s in states]
    a = _lib.BatchSolver.from_csr(csrs, Zs, NIT, ETA)
    b = _lib.BatchSolver(Zs, states, NIT, ETA, device=-1)
    for c in csrs:
        c.close()  # the batch keeps nothing of them
    assert (a.B, a.nits, a.device) == (b.B, b.nits, b.device) and a.device == -1
    assert a.sizes == b.sizes
    for i, n in enumerate(NAMES):
        for k, v in cc.EXPECTED_SIZES.get(n, {}).items():
            assert a.sizes[i][k] == v, (n, k)
        for f in cc.I_FIELDS:
            assert np.array_equal(a.read_i32(i, getattr(_lib, f)), b.read_i32(i, getattr(_lib, f))), (n, f)
        for f in cc.F_FIELDS:
            x, y = a.read(i, getattr(_lib, f)), b.read(i, getattr(_lib, f))
            assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), (n, f)
        assert [int(v) for v in a.read(i, _lib.BATCH_F_BUILD_INFO)] == [0, 1]
    with pytest.raises(_lib.MMWError, match="device -1"):
        a.iterate(1, None, np.arange(len(NAMES), dtype=np.uint64))
    a.close(); b.close()


def test_a_device_state_and_a_repeated_state_are_taken():
    state, Z = cc.case("er65")
    c = _lib.DeviceCSR.upload(state, device=-1)
    a = _lib.BatchSolver.from_csr([c.device_state(), c], [Z, Z - 1], NIT, ETA)
    assert a.sizes[0]["nnzL"] == a.sizes[1]["nnzL"] == 4225 and (a.sizes[0]["Z"], a.sizes[1]["Z"]) == (Z, Z - 1)
    assert np.array_equal(a.read_i32(0, _lib.I_L_INDICES), a.read_i32(1, _lib.I_L_INDICES))
    a.close(); c.close()
    with pytest.raises(_lib.MMWError, match="entry 0 is not an open DeviceCSR"):
        _lib.BatchSolver.from_csr([c], [Z], NIT, ETA)
    with pytest.raises(_lib.MMWError, match="entry 0 is not an open DeviceCSR"):
        _lib.BatchSolver.from_csr([state], [Z], NIT, ETA)


def _valid():
    return _lib.DeviceCSR.upload_arrays(6, cc.valid6(), device=-1)


@pytest.mark.parametrize("kind", list(cc.MALFORMED))
def test_malformed_instance_is_refused_by_instance_in_mmw_creates_words(kind):
    K, Z, arrays = cc.malformed(kind)
    words = cc.MALFORMED[kind]
    if kind != "indptr_end":
        said = cc.mmw_create_message(K, Z, arrays)
        assert said is not None and words in said, said
    good, good2, bad = _valid(), _valid(), _lib.DeviceCSR.upload_arrays(K, arrays, device=-1)
    with pytest.raises(_lib.MMWError) as ei:
        _lib.BatchSolver.from_csr([good, bad, good2], [3, Z, 3], NIT, ETA)
    assert "instance 1: " + words in str(ei.value), str(ei.value)
    if kind not in ("zero_norm_H",):  # (that one is the host path's own refusal, in mmw_batch_create's name)
        assert "mmw_batch_create_from_csr: instance 1: " in str(ei.value), str(ei.value)
    ok = _lib.BatchSolver.from_csr([good, good2], [3, 3], NIT, ETA)  # the valid states are still usable
    assert ok.sizes[0]["K"] == 6 and ok.sizes[0]["E_asso"] == 2
    for h in (ok, good, good2, bad):
        h.close()


def test_the_lower_of_two_bad_instances_is_named():
    bad1 = _lib.DeviceCSR.upload_arrays(6, cc.malformed("q_diagonal")[2], device=-1)
    bad2 = _lib.DeviceCSR.upload_arrays(6, cc.malformed("unsorted")[2], device=-1)
    good = _valid()
    with pytest.raises(_lib.MMWError) as ei:
        _lib.BatchSolver.from_csr([good, bad1, bad2], [3, 3, 3], NIT, ETA)
    assert "mmw_batch_create_from_csr: instance 1: " + cc.MALFORMED["q_diagonal"] in str(ei.value), str(ei.value)
    with pytest.raises(_lib.MMWError) as ei:
        _lib.BatchSolver.from_csr([bad2, bad1, good], [3, 3, 3], NIT, ETA)
    assert "mmw_batch_create_from_csr: instance 0: " + cc.MALFORMED["unsorted"] in str(ei.value), str(ei.value)
    for h in (bad1, bad2, good):
        h.close()


def _raw(handles, Zs, nits, B=None, rank_radio=2):
    """The C entry itself: (status, message, *out)."""
    L = _lib.lib()
    out = C.c_void_p(12345)  # a marker: a refusal leaves *out untouched
    B = len(handles) if B is None else B
    arr = (C.c_void_p * max(1, len(handles)))(*handles)
    rc = L.mmw_batch_create_from_csr(C.byref(out), B, arr, _lib._pi(_lib._i32(Zs)), rank_radio, ETA, _lib._pi(_lib._i32(nits)))
    return rc, L.mmw_last_error().decode(), out.value


def test_refusals_that_need_no_device():
    good = _valid()
    h = good._h.value
    rc, msg, out = _raw([h], [3], [NIT], B=0)
    assert rc == -1 and "mmw_batch_create_from_csr: B must be >= 1" in msg and out == 12345
    rc, msg, out = _raw([h, None, h], [3, 3, 3], [NIT] * 3)
    assert rc == -1 and "mmw_batch_create_from_csr: instance 1: null pointer" in msg and out == 12345
    rc, msg, out = _raw([h, h], [3, 3], [NIT, 0])
    assert rc == -1 and "mmw_batch_create_from_csr: instance 1: nit must be >= 1" in msg and out == 12345
    rc, msg, out = _raw([h, h], [3, 1], [NIT, NIT])
    assert rc == -1 and "mmw_batch_create_from_csr: instance 1: Z must be >= 2" in msg and out == 12345
    rc, msg, out = _raw([h, h], [3, 300], [NIT, NIT])
    assert rc == -1 and "mmw_batch: instance 1: D = 600 exceeds the batch limit 512 (run it on a handle)" in msg and out == 12345
    K = 4097
    eye = scipy.sparse.identity(K, format="csr", dtype=np.float64)
    big = _lib.DeviceCSR.upload((eye, scipy.sparse.csr_matrix((K, K), dtype=np.float64), np.ones(K)), device=-1)
    rc, msg, out = _raw([h, big._h.value], [3, 3], [NIT, NIT])
    assert rc == -1 and "mmw_batch: instance 1: K = 4097 exceeds the batch limit 4096 (run it on a handle)" in msg and out == 12345
    # the same two in mmw_batch_create's own words
    with pytest.raises(_lib.MMWError, match=r"D = 600 exceeds the batch limit 512"):
        _lib.BatchSolver([300], [good.state()], NIT, ETA, device=-1)
    with pytest.raises(_lib.MMWError, match="one slot count per state"):
        _lib.BatchSolver.from_csr([good], [3, 3], NIT, ETA)
    rc, msg, out = _raw([h], [3], [NIT])
    assert rc == 0 and out not in (None, 12345)
    assert _lib.lib().mmw_batch_destroy(C.c_void_p(out)) == 0
    good.close(); big.close()


# ---- the workflows' routing, on stubs -------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _stub_csr(device, K=6):
    """A DeviceCSR that holds no handle: enough for the routing, which reads its type and its device."""
    c = _lib.DeviceCSR._new(device)
    c.K = K
    c.bounds = lambda: (2, 4)
    return c


@pytest.fixture
def routes(monkeypatch):
    seen = []

    class Stub:
        def __init__(self, Zs, states, *a, **k):
            seen.append(("host", list(states)))
            raise _Stop()

        @classmethod
        def from_csr(cls, csrs, Zs, *a, **k):
            seen.append(("csr", list(csrs)))
            raise _Stop()
    monkeypatch.setattr(_lib, "BatchSolver", Stub)
    return seen


def _run_all(states, seen):
    Zs = [3] * len(states)
    calls = (lambda: batch.run_with_state_many(0, Zs, states, nit=NIT), lambda: batch.convergence_many(Zs, states, NIT, ETA),
             lambda: batch.search_many(states, nit=NIT))
    for call in calls:
        with pytest.raises(_Stop):
            call()
    kinds = [k for k, _ in seen]
    del seen[:]
    return kinds


def test_workflows_route_device_csr_states_and_nothing_else(routes):
    a, b = _stub_csr(0), _stub_csr(0)
    assert batch._csr_route([a.device_state(), b.device_state()]) == [a, b]
    assert _run_all([a.device_state(), b.device_state(), a.device_state()], routes) == ["csr"] * 3
    triple = cc.case("k3")[0]
    host_csr = _lib.DeviceCSR.upload(triple, device=-1)
    other = _stub_csr(1)

    class Env:  # a DeviceState of something that is not a DeviceCSR (a DeviceEnv)
        K = 3

        def state(self):
            return triple

        def bounds(self):
            return (2, 4)
    for states in ([triple, triple], [a.device_state(), triple], [triple, a.device_state()], [host_csr.device_state()] * 2,
                   [a.device_state(), host_csr.device_state()], [a.device_state(), other.device_state()], [_lib.DeviceState(Env())],
                   [a, b]):  # (a bare DeviceCSR is not a state)
        assert batch._csr_route(states) is None
    assert _run_all([triple, triple], routes) == ["host"] * 3
    assert _run_all([a.device_state(), triple], routes) == ["host"] * 3
    assert _run_all([host_csr.device_state()], routes) == ["host"] * 3
    host_csr.close()


def test_handles_of_a_routed_batch_come_from_the_owner():
    made = []

    class Owner:
        def solver(self, Z, nit, eta, rank_radio=2, dtype=_lib.F64):
            made.append((Z, nit, eta, rank_radio, dtype))

            class H:
                pass
            h = H()
            h.Z = Z
            h.close = lambda: None
            return h
    hs = batch._Handles(["never read"], NIT, ETA, 2, 0, owners=[Owner()])
    h = hs.get(0, 5)
    assert made == [(5, NIT, ETA, 2, _lib.F64)] and hs.get(0, 5) is h
    hs.close()
