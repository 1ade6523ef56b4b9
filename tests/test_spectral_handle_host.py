"""Host side of the spectral baseline on the solver handle (no GPU): the Laplacian on the L pattern as a device = -1 handle states it
(MMW_F_LAPLACIAN, csrc/kernels_spectral.h: the same row function the kernel's lanes run) against the NumPy restatement
(tests/helpers/laplacian_pattern.py, bitwise) and against `sdp_solver.spectral_laplacian` (SciPy sums in another order: 4 m eps d_max,
m the longest pattern row, d_max the largest degree), the entry's declaration and refusals, and the routing of `spectral_sdp_solver`
where no device is involved.
"""
import os
import sys
import types

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import laplacian_pattern as LP  # noqa: E402

from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver, spectral_laplacian, spectral_sdp_solver  # noqa: E402

EPS = 2.0 ** -52


def hand_state():
    """6 users: 0..4 hear each other with asymmetric gains, except that 0 and 1 share an access point and no gain (their pattern entry
    is there through Q alone); S[2, 3] is a stored zero next to a non-zero S[3, 2]; user 5 is isolated.  Own gain 4 on the diagonal."""
    W = np.zeros((6, 6))
    W[:5, :5] = np.random.default_rng(11).uniform(0.1, 2.0, size=(5, 5))
    np.fill_diagonal(W, 4.0)
    W[0, 1] = W[1, 0] = 0.0
    S = scipy.sparse.csr_matrix(W)
    S.sort_indices()
    row2 = slice(S.indptr[2], S.indptr[3])
    at = S.indptr[2] + int(np.nonzero(S.indices[row2] == 3)[0][0])
    S.data[at] = 0.0  # stays in the structure
    assert S.nnz == 36 - 10 - 2 and S[2, 3] == 0.0 and S[3, 2] != 0.0
    Q = scipy.sparse.csr_matrix(([1.0, 1.0], ([0, 1], [1, 0])), shape=(6, 6))
    return S, Q, np.full(6, 100.0)


STATES = {"journal5": lambda: journal_graph(5), "er120": lambda: er_contention_graph(120, 0.05, 1), "hand": hand_state}


@pytest.fixture(scope="module", params=sorted(STATES))
def case(request):
    st = STATES[request.param]()
    s = _lib.Solver(2, st, 1, 0.1, device=-1)
    c = types.SimpleNamespace(name=request.param, state=st, K=s.K, ip=s.read_i32(_lib.I_L_INDPTR), ix=s.read_i32(_lib.I_L_INDICES), lap=s.laplacian())
    s.close()
    return c


def test_laplacian_is_bitwise_the_restatement(case):
    want = LP.laplacian_on_pattern(case.state[0], case.ip, case.ix)
    assert case.lap.shape == want.shape == case.ix.shape and case.lap.dtype == np.float64
    assert case.lap.tobytes() == want.tobytes(), case.name


def test_laplacian_against_scipy(case):
    ref = spectral_laplacian(case.state[0]).toarray()
    got = LP.scatter(case.K, case.ip, case.ix, case.lap)
    m = int(np.max(np.diff(case.ip)))
    dmax = float(np.max(np.diag(ref)))
    err = float(np.max(np.abs(got - ref)))
    print("[spectral-handle] %-8s K %4d longest row %3d: max |L - scipy| %.3e, bar %.3e" % (case.name, case.K, m, err, 4 * m * EPS * dmax))
    assert err <= 4 * m * EPS * dmax, case.name


def test_laplacian_is_exactly_symmetric_and_zero_on_pure_q_entries(case):
    got = LP.scatter(case.K, case.ip, case.ix, case.lap)
    assert np.array_equal(got, got.T), case.name
    pure = LP.pure_q_entries(case.state, case.ip, case.ix)
    assert np.all(case.lap[pure] == 0.0), case.name
    if case.name == "hand":
        rows = np.repeat(np.arange(case.K), np.diff(case.ip))
        assert sorted(zip(rows[pure].tolist(), case.ix[pure].tolist())) == [(0, 1), (1, 0)]
        dp = case.ix == rows
        assert case.lap[dp][5] == 0.0 and np.all(case.lap[dp][:5] > 0.0)  # the isolated user's degree
        at23 = np.nonzero((rows == 2) & (case.ix == 3))[0][0]
        assert case.lap[at23] == -case.state[0][3, 2]  # the stored zero adds nothing


def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_factor_spectral(mmw_solver* s, int32_t Z, int32_t index_order, double* out, uint64_t seed);" in hdr
    for field in ("MMW_F_LAPLACIAN = 27", "MMW_F_SPECTRAL_INFO = 28", "MMW_F_SPECTRAL_EIG = 29"):
        assert field in hdr, field
    assert "mmw_factor_spectral" in _lib.EXPORTS
    getattr(_lib.lib(), "mmw_factor_spectral")
    for name in ("factor_spectral", "laplacian", "spectral_info", "spectral_eig", "factor_row_norms"):
        assert hasattr(_lib.Solver, name), name


def test_refusals_of_a_host_only_handle():
    st = journal_graph(3)
    s = _lib.Solver(2, st, 1, 0.1, device=-1)
    L = _lib.lib()
    K = s.K
    for bad in (0, K + 1):  # the argument is looked at before anything else, the kind of handle included
        assert L.mmw_factor_spectral(s._h, bad, 0, None, 0) == -1 and b"must be in [1, K = %d]" % K in L.mmw_last_error(), bad
        with pytest.raises(_lib.MMWError, match="status -1"):
            s.factor_spectral(bad)
    assert L.mmw_factor_spectral(s._h, 3, 2, None, 0) == -1
    assert L.mmw_factor_spectral(s._h, 3, 0, None, 0) == -3 and b"host-only" in L.mmw_last_error()
    with pytest.raises(_lib.MMWError, match="status -3"):
        s.factor_spectral(3)
    with pytest.raises(_lib.MMWError, match="status -3"):
        s.factor_spectral(3, resident=True, index_order=True)
    assert L.mmw_factor_spectral(None, 3, 0, None, 0) == -1
    with pytest.raises(_lib.MMWError, match="status -1.*wrong length"):
        s.read(_lib.SOLVER_F_LAPLACIAN, s.nnzL + 1)
    s.close()


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, A, **kw):
        self.calls.append((A, kw))
        K, Z = A.shape[0], kw["k"]
        rng = np.random.default_rng(K + Z)
        return np.arange(Z, dtype=np.float64), rng.standard_normal((K, Z))


@pytest.fixture(scope="module")
def big_state():
    st = er_contention_graph(1100, 0.01, 1)
    assert st[0].shape[0] == 1100 > _lib.BATCH_EPILOGUE_MAX_K
    return st


@pytest.mark.parametrize("kwargs", [{}, {"handle": False}, {"handle": True, "device": -1}, {"device": -1}])
def test_routing_that_stays_on_eigsh(big_state, monkeypatch, kwargs):
    rec = Recorder()
    monkeypatch.setattr(scipy.sparse.linalg, "eigsh", rec)
    alg = spectral_sdp_solver(100, 2, 1., **kwargs)
    assert alg.handle is bool(kwargs.get("handle", False))
    ok, blk = alg.run_with_state(0, 12, big_state)
    assert ok is True and isinstance(blk, np.ndarray) and blk.shape == (1100, 12)
    assert len(rec.calls) == 1
    A, kw = rec.calls[0]
    assert kw == {"k": 12, "which": "LM", "return_eigenvectors": True, "tol": 1e-5}  # the reference's own arguments (sdp_solver.py:178)
    assert (A != spectral_laplacian(big_state[0])).nnz == 0
    assert np.max(np.abs(np.linalg.norm(blk, axis=1) - 1.0)) <= 4 * EPS
    logs = alg.LOGGED_NP_DATA
    assert sorted(logs) == ["spectral_problem_setup", "spectral_solve"] and all(logs[k][0, 3:5].tolist() == [12.0, 1100.0] for k in logs)
    assert alg._dev is None  # no handle was made


def test_index_order_applied_twice_still_orders_and_a_device_scaled_block_passes_through():
    x = np.random.default_rng(2).standard_normal((300, 7))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    once = spectral_sdp_solver.index_ordered(x)
    assert once.tobytes() == rand_sdp_solver.index_ordered(x).tobytes()
    twice = spectral_sdp_solver.index_ordered(once)
    assert np.all(np.diff(np.linalg.norm(twice, axis=1)) < 0.0)
    done = _lib.DeviceFactor(types.SimpleNamespace(K=300), 7, 1, index_ordered=True)
    assert spectral_sdp_solver.index_ordered(done) is done
    plain = _lib.DeviceFactor(types.SimpleNamespace(K=300), 7, 1)
    assert plain.index_ordered is False
