"""The solver handle built on the device from a CSR state that lies there (mmw_csr_*, mmw_create_from_csr, csrc/pattern_csr_device.h)
against the handle mmw_create builds on the host from the same arrays: every list, every value and -- the pattern and the blocking being
the same -- every bit of three iterations.  The cases (tests/helpers/csr_cases.py) are the smallest shapes at which the kernels can go
wrong: K = 2, no Q at all, rows on and over the 64-lane boundary, gains stored on association pairs, stored zeros, missing diagonals."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import csr_cases as cc  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = {"f32": _lib.F32, "f64": _lib.F64}


assert_same_handle = cc.assert_same_handle


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(cc.CASES))
def test_handle_from_device_csr_is_the_handle_from_the_host_state(name, dtype):
    state, Z = cc.case(name)
    a = _lib.Solver(Z, state, 3, 0.04, dtype=DTYPES[dtype])
    c = _lib.DeviceCSR.upload(state)
    assert c.bounds() == tuple(int(x) for x in binary_search_relaxation().set_bounds(state))
    b = _lib.Solver.from_csr(c, Z, 3, 0.04, dtype=DTYPES[dtype])
    c.close()  # the handle keeps no reference to the state
    assert_same_handle(a, b, Z)
    a.close(); b.close()


def test_rounding_on_a_handle_from_device_csr():
    """The rounding side (S_gain without diagonal and stored zeros, Q, h_max) filled from the device lists: the host-built handle's slots."""
    state, _ = cc.case("er120")
    Z = 6
    a = _lib.Solver(Z, state, 1, 0.04)
    c = _lib.DeviceCSR.upload(state)
    b = _lib.Solver.from_csr(c, Z, 1, 0.04)
    rng = np.random.default_rng(2)
    for Zr in (Z, 5):
        gX = rng.standard_normal((a.K, 2 * (Z - 1)))
        rv = rng.standard_normal((3, Zr, gX.shape[1]))
        rv /= np.linalg.norm(rv, axis=2, keepdims=True)
        za, ra = a.round(Zr, gX, rv)
        zb, rb = b.round(Zr, gX, rv)
        assert np.array_equal(za, zb) and np.array_equal(ra, rb)
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("name", ["er120_zeros", "k3"])
def test_borrowed_pointers(name):
    """wrap on the addresses of an uploaded state (K = 3: the Q pointers are null): the same handle."""
    state, Z = cc.case(name)
    a = _lib.Solver(Z, state, 3, 0.04)
    up = _lib.DeviceCSR.upload(state)
    ptr = up.pointers()
    if name == "k3":
        assert ptr[4] == 0 and ptr[5] == 0 and all(ptr[i] for i in (0, 1, 2, 3, 6))
    w = _lib.DeviceCSR.wrap(*ptr, K=up.K, nnzS=up.nnzS, nnzQ=up.nnzQ)
    assert w.bounds() == up.bounds()
    S, Q, h = w.state()
    S0, Q0, h0 = up.state()
    assert np.array_equal(S.indices, S0.indices) and np.array_equal(S.data, S0.data) and np.array_equal(Q.indptr, Q0.indptr) and np.array_equal(h, h0)
    b = _lib.Solver.from_csr(w, Z, 3, 0.04)
    assert_same_handle(a, b, Z)
    a.close(); b.close(); w.close(); up.close()


def test_state_borrowed_from_torch():
    """er120 moved to the device as torch sparse-CSR tensors, borrowed by DeviceCSR.from_torch: the same handle (and wrap refuses torch's own
    int64 index arrays).  A torch build that ships its own HIP runtime has to touch the device before the library's first HIP call in a
    process (bench.py's order), so the case runs in a fresh interpreter: tests/helpers/csr_torch_child.py."""
    pytest.importorskip("torch")
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "csr_torch_child.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "from_torch ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bisection_on_a_device_resident_csr_state():
    """test_bisection_on_a_device_resident_state on DeviceCSR.device_state(): bounds from the device count pass, handles by mmw_create_from_csr,
    the state never materialised on the host, a colouring feasible against the host matrices."""
    from sig_sdp_mmw_amd.mmw import mmw
    state, _ = cc.case("journal16")
    csr = _lib.DeviceCSR.upload(state)
    assert tuple(int(x) for x in binary_search_relaxation().set_bounds(state)) == csr.bounds()
    dstate = csr.device_state()
    bs = binary_search_relaxation()
    bs.verbose = False
    alg = mmw(nit=60, eta=0.04, dtype="f32", rng="device", seed=1)
    bs.feasibility_check_alg = alg
    np.random.seed(0)
    z_vec, Z, rem = bs.run(dstate)
    assert dstate._host is None, "the search must not have pulled the state to the host"
    assert rem == 0 and Z >= csr.bounds()[0]
    S, Q, h = state
    So = S.copy().tolil(); So.setdiag(0); So = So.tocsr()
    for zz in range(Z):
        mem = np.where(z_vec == zz)[0]
        assert np.all(np.asarray(So[mem][:, mem].sum(axis=0)).ravel() <= h[mem] + 1e-12) and Q[mem][:, mem].nnz == 0
    alg.close(); csr.close()


@pytest.mark.parametrize("kind", cc.DEVICE_SAFE)
def test_malformed_input_is_refused_on_the_device(kind):
    """Only the kinds whose bad value is never used as an address.  The refusal leaves nothing behind: the valid state builds and iterates."""
    K, Z, arrays = cc.malformed(kind)
    c = _lib.DeviceCSR.upload_arrays(K, arrays)
    with pytest.raises(_lib.MMWError) as ei:
        _lib.Solver.from_csr(c, Z, 3, 0.04)
    assert cc.MALFORMED[kind] in str(ei.value), str(ei.value)
    with pytest.raises(_lib.MMWError) as ei:
        c.bounds()
    assert cc.MALFORMED[kind] in str(ei.value), str(ei.value)
    c.close()
    good = _lib.DeviceCSR.upload_arrays(6, cc.valid6())
    b = _lib.Solver.from_csr(good, Z, 3, 0.04)
    b.iterate(1, None, seed=1)
    assert np.all(np.isfinite(b.read(_lib.F_XVAL)))
    b.close(); good.close()
