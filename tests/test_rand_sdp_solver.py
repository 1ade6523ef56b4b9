"""`sdp_solver.rand_sdp_solver` (the reference's sdp_solver.py:109-114) under the reference's class protocol on a seeded global stream:
the embedding is the NumPy draws of the reference's expression, and after `run_with_state` and `rounding` the stream stands where a
restatement of the two calls leaves it (the rounding through the oracle's `rounding_one_attempt` on the same draws).

The norms of the embedding's rows are 1 to the last bit, so `argsort(-norm)` on the block itself sorts rounding noise (75 users, four
distinct norms): the class visits the users in index order and says so by handing the rounding `rand_sdp_solver.index_ordered(gX)`.
The restatement gives the oracle the same block, on which the oracle's order is the index order by a margin of 2^-32 per user."""
import numpy as np
import pytest

from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd.graphs import journal_graph
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver, sdp_solver

RHO = 75e-4


def restated_embedding(K, Z, rank_radio):
    r = np.random.randn(K, Z * rank_radio)
    return r / np.linalg.norm(r, axis=1, keepdims=True)


@pytest.mark.parametrize("Z,rank_radio", [(2, 2), (9, 2), (5, 3)])
def test_embedding_is_the_numpy_draws_and_leaves_the_stream_where_the_reference_does(Z, rank_radio):
    state = journal_graph(5, RHO, seed=3)
    K = state[0].shape[0]
    alg = rand_sdp_solver(rank_radio=rank_radio)
    assert isinstance(alg, sdp_solver) and alg.nit == 100
    np.random.seed(11)
    ok, gX = alg.run_with_state(0, Z, state)
    after = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(11)
    want = restated_embedding(K, Z, rank_radio)
    assert ok is True and gX.shape == (K, Z * rank_radio) and np.array_equal(gX, want)
    assert np.array_equal(np.random.get_state()[1], after[0]) and np.random.get_state()[2] == after[1]
    np.testing.assert_allclose(np.linalg.norm(gX, axis=1), 1.0, rtol=1e-14)


@pytest.mark.gpu
@pytest.mark.parametrize("Z", [12, 9])
def test_rounding_of_the_embedding_is_the_restatements_and_so_is_the_stream(Z):
    """Z = 12 has room (the first attempt leaves nobody over), Z = 9 leaves users over in all 10 attempts (worked out with the oracle on
    the CPU): both ends of sdp_solver.py:18-25."""
    state = journal_graph(5, RHO, seed=3)
    K = state[0].shape[0]
    alg = rand_sdp_solver()
    np.random.seed(5)
    _, gX = alg.run_with_state(0, Z, state)
    z_vec, Zr, rem = alg.rounding(Z, gX, state)
    alg.close()
    pos = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(5)
    want = restated_embedding(K, Z, 2)
    assert np.array_equal(gX, want)
    visit = rand_sdp_solver.index_ordered(want)
    assert np.array_equal(np.argsort(-np.linalg.norm(visit, axis=1), kind="stable"), np.arange(K)) and np.min(-np.diff(np.linalg.norm(visit, axis=1))) > 2.0 ** -33
    for _ in range(10):
        rv = np.random.randn(Z, want.shape[1])
        rv = rv / np.linalg.norm(rv, axis=1, keepdims=True)
        zo, Zo, remo, _ = orc.rounding_one_attempt(Z, visit, state, rv)
        if remo == 0:
            break
    print("[rand-sdp] Z %d: left over %d (restatement %d)" % (Z, rem, remo))
    assert Zr == Zo == Z and int(rem) == remo and np.array_equal(z_vec, zo)
    assert (remo == 0) == (Z == 12)
    assert np.array_equal(np.random.get_state()[1], pos[0]) and np.random.get_state()[2] == pos[1]
