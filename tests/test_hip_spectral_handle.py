"""The spectral baseline on the solver handle (mmw_factor_spectral, csrc/kernels_spectral.h + Factorizer::run's eigenvector export): the
row-normalised top-Z eigenvector block of the state's Laplacian at any K, against `numpy.linalg.eigh` (tests/helpers/spectral_oracle.py).

Cases: the smallest that reach each branch of Factorizer::run (the filter runs only when K > 384 and 4 b < 3 K; the first dense
eigensolve is skipped when b > 96).  relgap = (lambda_Z - lambda_Z+1) / lambda_1 of the dense spectrum; every test asserts
relgap >= 1e-3 from its own `Dense` first.

  case    state                                K     Z    b     relgap   what it reaches
  exact   journal_graph(10)                    200   3    K     8.9e-2   one exact Rayleigh-Ritz on the whole space
  edge    journal_graph(14)                    392   4    16    3.8e-2   just past the K <= 384 switch, filter on
  j16     journal_graph(16)                    512   12   24    3.4e-2   filter, locality blocking
  big5    journal_graph(23)                    1058  5    17    2.6e-2   beyond the batch's limit
  big23   journal_graph(23)                    1058  23   35    1.9e-2   as above, wider block
  skiprr  journal_graph(23)                    1058  97   116   3.3e-3   b > 96: first eigensolve skipped
  er      er_contention_graph(1100, 0.01, 1)   1100  12   24    1.4e-2   no locality to find; 1099 of 1100 rows >= tau

each in fp64 and fp32.  Bars (tol_T = 1e-9 / 2e-5, the factor's own stopping constants; eps_T = 2^-52 / 2^-23; m the longest pattern
row; none comes from the device's output):
  residual     max_i ||L v_i - theta_i v_i|| / lambda_1 <= 4 tol_T, computed here in NumPy from the block read back (rows scaled back by
               MMW_F_FACTOR_ROWNORM) and MMW_F_SPECTRAL_EIG; the 4 covers the row-norm round trip and, in fp32, the products' rounding
  eigenvalues  |theta_i - lambda_i| <= (tol_T + 16 m eps_T) lambda_1: a Ritz-value residual bound plus the SpMM's rounding (16: the
               batch test's factor)
  projector    max |V^ V^T - V V^T| <= sqrt(2 Z) 4 tol_T / relgap (Davis-Kahan on the residual block, Frobenius norm)
  Gram         on the rows of norm >= tau = 1e-3: that bar / tau^2
Everything else is bit equality.  One of them carries a condition the handle's design sets ("from the generator"): a handle
made by mmw_create_from_env blocks its rows by position, so its products sum in another order than mmw_create's; with the pattern-only
order (MMW_ENV_RCM=1, the switch tests/test_hip_env.py compares under) the three creators give the same bits, and with its own order
the handle meets the residual bar and its Laplacian is still bitwise the restatement.
"""
import functools
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import laplacian_pattern as LP  # noqa: E402
import spectral_oracle as SO  # noqa: E402

from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph, journal_graph_device  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver, spectral_sdp_solver  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {  # name: (state, K, Z, b)
    "exact": ("j10", 200, 3, 200),
    "edge": ("j14", 392, 4, 16),
    "j16": ("j16", 512, 12, 24),
    "big5": ("j23", 1058, 5, 17),
    "big23": ("j23", 1058, 23, 35),
    "skiprr": ("j23", 1058, 97, 116),
    "er": ("er", 1100, 12, 24),
}
DTYPES = {"f64": (_lib.F64, 1e-9, 2.0 ** -52), "f32": (_lib.F32, 2e-5, 2.0 ** -23)}
SEED = 3


@functools.lru_cache(maxsize=None)
def state(key):
    if key == "er":
        return er_contention_graph(1100, 0.01, 1)
    if key == "k6":
        return er_contention_graph(6, 0.5, 1)
    return journal_graph(int(key[1:]))


@functools.lru_cache(maxsize=None)
def dense(key):
    return SO.Dense(state(key)[0])


@functools.lru_cache(maxsize=None)
def result(case, dt):
    """One handle per (case, dtype): the plain block on the host, its record, a second call, the index-ordered block."""
    key, K, Z, b = CASES[case]
    s = _lib.Solver(8, state(key), 1, 0.1, dtype=DTYPES[dt][0])
    r = types.SimpleNamespace()
    r.N = s.factor_spectral(Z, seed=SEED)
    r.info, r.eig, r.rown = s.spectral_info(), s.spectral_eig(Z), s.factor_row_norms()
    r.m = int(np.max(np.diff(s.read_i32(_lib.I_L_INDPTR))))
    r.again = s.factor_spectral(Z, seed=SEED)
    r.rown_again = s.factor_row_norms()
    r.ordered = s.factor_spectral(Z, seed=SEED, index_order=True)
    r.kind = s.read(_lib.F_SPMM_KIND, 2)[0]
    s.close()
    return r


def bars(d, Z, m, dt):
    _, tol, eps = DTYPES[dt]
    relgap = d.relgap(Z)
    pbar = np.sqrt(2.0 * Z) * 4.0 * tol / relgap if relgap > 0 else float("inf")
    return relgap, 4.0 * tol, (tol + 16.0 * m * eps) * d.lam_max(), pbar


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_block_against_the_dense_restatement(case, dt):
    key, K, Z, b = CASES[case]
    d = dense(key)
    relgap, rbar, ebar, pbar = bars(d, Z, 0, dt)
    assert relgap >= 1e-3, (case, relgap)
    assert d.K == K
    r = result(case, dt)
    relgap, rbar, ebar, pbar = bars(d, Z, r.m, dt)
    N, rown, eig = r.N, r.rown, r.eig
    assert N.shape == (K, Z) and eig.shape == (Z,) and rown.shape == (K,) and not np.any(np.isnan(N))
    assert r.info["Z"] == Z and r.info["block"] == b, r.info
    assert r.info["theta_Z"] == eig[0] and np.all(np.diff(eig) >= 0.0)
    assert (r.info["theta_next"] <= eig[0]) if b > Z else (r.info["theta_next"] == 0.0)
    if dt == "f64":
        assert r.info["mfma_passes"] == 0
    n = np.linalg.norm(N, axis=1)
    # unit rows, or exactly zero ones (16 eps: 9 roundings in the device's sum of squares, its root and the division, as many in NumPy's norm)
    assert np.all((n == 0.0) | (np.abs(n - 1.0) <= 16 * SO.EPS)) and np.array_equal(n == 0.0, rown == 0.0)
    lam, V = d.top(Z)
    lam1 = d.lam_max()
    Vd = SO.unnormalised_from(N, rown)
    resid = float(np.max(np.linalg.norm(d.L @ Vd - Vd * eig, axis=0))) / lam1
    eerr = float(np.max(np.abs(eig - lam)))
    perr = float(np.max(np.abs(SO.projector(Vd) - SO.projector(V))))
    rows = SO.big_rows(V)
    gerr = SO.gram_distance(N, SO.normalise_rows(V), rows)
    print("[spectral-handle] %-6s %s K %4d Z %2d b %3d relgap %.2e: outer %d, device residual %.2e, SpMM kind %d, matrix-core passes %d; "
          "residual %.2e (bar %.1e), eigenvalues %.2e (%.1e), projector %.2e (%.1e), Gram on %d rows %.2e (%.1e)"
          % (case, dt, K, Z, b, relgap, r.info["outer"], r.info["resid"], r.kind, r.info["mfma_passes"], resid, rbar, eerr, ebar, perr, pbar,
             int(rows.sum()), gerr, pbar / SO.TAU ** 2))
    assert resid <= rbar, (case, dt, "residual", resid, rbar)
    assert eerr <= ebar, (case, dt, "eigenvalues", eerr, ebar)
    assert perr <= pbar, (case, dt, "projector", perr, pbar)
    assert gerr <= pbar / SO.TAU ** 2, (case, dt, "Gram", gerr, pbar / SO.TAU ** 2)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_same_seed_same_bits_and_index_order_is_the_host_scaling(case, dt):
    r = result(case, dt)
    assert r.again.tobytes() == r.N.tobytes() and r.rown_again.tobytes() == r.rown.tobytes()
    assert r.ordered.tobytes() == rand_sdp_solver.index_ordered(r.N).tobytes()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_z_equal_k_takes_the_constant_vector(dt):
    st = state("k6")
    d = dense("k6")
    K = Z = 6
    assert d.K == K
    _, tol, eps = DTYPES[dt]
    s = _lib.Solver(2, st, 1, 0.1, dtype=DTYPES[dt][0])
    N = s.factor_spectral(Z, seed=SEED)
    eig, rown, info = s.spectral_eig(Z), s.factor_row_norms(), s.spectral_info()
    m = int(np.max(np.diff(s.read_i32(_lib.I_L_INDPTR))))
    s.close()
    assert info["block"] == K and info["theta_next"] == 0.0
    ebar = (tol + 16.0 * m * eps) * d.lam_max()
    assert float(np.max(np.abs(eig - d.lam))) <= ebar, (eig, d.lam)
    V = SO.unnormalised_from(N, rown)
    off = float(np.max(np.abs(V.T @ V - np.eye(K))))
    print("[spectral-handle] Z = K = 6 %s: eigenvalue error %.2e (bar %.1e), |V^T V - I| %.2e (bar %.1e)" % (dt, float(np.max(np.abs(eig - d.lam))), ebar, off, 16 * K * eps))
    assert off <= 16 * K * eps


def three_handles(env, st, Z, dt):
    csr = _lib.DeviceCSR.upload(st)
    return [_lib.Solver(Z, st, 1, 0.1, dtype=dt), _lib.Solver.from_env(env, Z, 1, 0.1, dtype=dt), _lib.Solver.from_csr(csr, Z, 1, 0.1, dtype=dt)], csr


def test_three_creators_give_the_same_laplacian_and_the_same_block(monkeypatch):
    st, env = journal_graph_device(14)
    Z = 4
    d = SO.Dense(st[0])
    assert d.relgap(Z) >= 1e-3
    want = None
    blocks = {}
    for variant in ("rcm", "spatial"):
        if variant == "rcm":
            monkeypatch.setenv("MMW_ENV_RCM", "1")
        else:
            monkeypatch.delenv("MMW_ENV_RCM")
        hs, csr = three_handles(env, st, 8, _lib.F64)
        for who, s in zip(("create", "from_env", "from_csr"), hs):
            lap = s.laplacian()
            if want is None:
                want = LP.laplacian_on_pattern(st[0], s.read_i32(_lib.I_L_INDPTR), s.read_i32(_lib.I_L_INDICES))
            assert lap.tobytes() == want.tobytes(), (variant, who, "laplacian")
            N = s.factor_spectral(Z, seed=SEED)
            assert s.laplacian().tobytes() == want.tobytes()
            blocks[(variant, who)] = (N, s.spectral_eig(Z), s.factor_row_norms())
            s.close()
        csr.close()
    env.close()
    ref = blocks[("rcm", "create")]
    for k in (("rcm", "from_env"), ("rcm", "from_csr"), ("spatial", "create"), ("spatial", "from_csr")):
        assert blocks[k][0].tobytes() == ref[0].tobytes() and blocks[k][1].tobytes() == ref[1].tobytes() and blocks[k][2].tobytes() == ref[2].tobytes(), k
    N, eig, rown = blocks[("spatial", "from_env")]  # its own row blocks: the same bar as every block
    Vd = SO.unnormalised_from(N, rown)
    resid = float(np.max(np.linalg.norm(d.L @ Vd - Vd * eig, axis=0))) / d.lam_max()
    print("[spectral-handle] from_env with its spatial row blocks: residual %.2e, bitwise the pattern-order block: %s" % (resid, N.tobytes() == ref[0].tobytes()))
    assert resid <= 4e-9


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mmw_factor_afterwards_gives_the_bits_of_a_fresh_handle(dt):
    st = state("j16")
    Z, nit = 8, 3
    rank = 2 * (Z - 1)
    out = []
    for spectral_first in (False, True):
        s = _lib.Solver(Z, st, nit, 0.04, dtype=DTYPES[dt][0])
        s.iterate(nit, None, seed=5)
        if spectral_first:
            s.factor_spectral(12, seed=SEED)
            s.factor_spectral(40, seed=SEED, resident=True, index_order=True)
            assert s.factor_row_norms().shape == (s.K,)
        out.append(s.factor(rank, seed=7))
        with pytest.raises(_lib.MMWError, match="status -3.*not a spectral one"):
            s.factor_row_norms()
        s.close()
    assert out[0].tobytes() == out[1].tobytes()


def test_round_on_the_resident_block_is_round_on_its_host_copy_and_the_oracles():
    st = state("j16")
    Z = 12
    s = _lib.Solver(Z, st, 1, 0.1)
    assert s.spectral_info() == {"outer": 0, "resid": 0.0, "Z": 0, "block": 0, "theta_Z": 0.0, "theta_next": 0.0, "mfma_passes": 0}
    host = s.factor_spectral(Z, seed=SEED, index_order=True)
    blk = s.factor_spectral(Z, seed=SEED, resident=True, index_order=True)
    assert isinstance(blk, _lib.DeviceFactor) and blk.index_ordered and blk.shape == (s.K, Z)
    rv = np.random.default_rng(4).standard_normal((2, Z, Z))
    rv /= np.linalg.norm(rv, axis=2, keepdims=True)
    z_dev, rem_dev = s.round(Z, blk, rv)
    assert blk._host is None  # read where it lies
    z_host, rem_host = s.round(Z, host, rv)
    assert np.asarray(blk).tobytes() == host.tobytes()
    s.close()
    assert np.array_equal(z_dev, z_host) and np.array_equal(rem_dev, rem_host)
    for a in range(2):
        zo, _, remo, un = orc.rounding_one_attempt(Z, host, st, rv[a])
        zo = np.where(un, -1, zo).astype(np.int32)
        print("[spectral-handle] round attempt %d: left over %d (oracle %d), %d slots differ" % (a, rem_dev[a], remo, int(np.sum(z_dev[a] != zo))))
        assert int(rem_dev[a]) == remo and np.array_equal(z_dev[a], zo)


def test_class_routes_device_states_and_large_states_to_the_handle(monkeypatch):
    st, env = journal_graph_device(23)
    K = st[0].shape[0]
    assert K == 1058
    Z = 23
    # the host path's result, for the surface only (eigenvector signs differ, so the slots may)
    host_alg = spectral_sdp_solver(100, 2, 1., device=-1)
    np.random.seed(8)
    ok, hblk = host_alg.run_with_state(0, Z, st)
    hz, hZ, hrem = host_alg.rounding(Z, hblk, st)
    host_alg.close()

    def no_host(self):
        raise AssertionError("the state was copied to the host")
    monkeypatch.setattr(_lib.DeviceState, "host", no_host)
    for what, the_state in (("device state", env.device_state()), ("K 1100 host state", state("er"))):
        alg = spectral_sdp_solver(100, 2, 1., handle=True)
        np.random.seed(8)
        ok, blk = alg.run_with_state(0, Z, the_state)
        assert ok is True and isinstance(blk, _lib.DeviceFactor) and blk.index_ordered, what
        handle = alg._dev[2]
        assert blk.shape == (handle.K, Z)
        z_vec, Zo, rem = alg.rounding(Z, blk, the_state)
        assert alg._dev[2] is handle and blk._host is None, what  # the cached handle rounded the block where it lies
        assert Zo == Z == hZ and z_vec.shape == (handle.K,) and z_vec.dtype == hz.dtype and type(rem) is type(hrem), what
        assert np.all((0 <= z_vec) & (z_vec < Z)) and 0 <= rem <= handle.K
        logs = alg.LOGGED_NP_DATA
        assert sorted(logs) == ["spectral_problem_setup", "spectral_solve"], what
        assert all(logs[k].shape == (1, 6) and logs[k][0, 3:5].tolist() == [float(Z), float(handle.K)] and logs[k][0, 5] >= 0.0 for k in logs), what
        print("[spectral-handle] class on the handle, %s: left over %d (host path on the journal state %d), solve %.0f us"
              % (what, rem, hrem, logs["spectral_solve"][0, 5]))
        alg.close()
    # a host state within the batch's limit keeps the batch path, handle or not
    small = state("j10")
    alg = spectral_sdp_solver(100, 2, 1., handle=True)
    ok, blk = alg.run_with_state(0, 3, small)
    assert isinstance(blk, np.ndarray) and alg._dev is None
    env.close()
