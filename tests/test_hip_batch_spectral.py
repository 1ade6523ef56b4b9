"""The spectral baseline inside the batch (mmw_batch_factor_spectral, csrc/kernels_batch_spectral.h): the row-normalised top-Z
eigenvector block of the state's Laplacian from the batch's dense Jacobi, against `numpy.linalg.eigh` (tests/helpers/spectral_oracle.py).

Shapes, all in ONE batch (and each alone):
  one_ap  K 2,   Z 2    Z = K: eigsh refuses it, the Jacobi does not; the eigenvalue 0 enters the block as a zero column
  c3      K 27,  Z 8    odd K: the tournament has a bye
  c5      K 75,  Z 12   cell 5, seed 1
  c8      K 192, Z 12   localised eigenvectors: 65 users with a row norm below 1e-3
  c10     K 300, Z 12   epi_jacobi<8>
  c15     K 675, Z 20   epi_jacobi<12>
  c17     K 867, Z 20   epi_jacobi<16>
  iso     K 6,   Z 3    hand-made, user 5 isolated: its row must be exactly zero
  diag    K 5,   Z 2    S_gain diagonal: L = 0, the factor is all zeros
and K 1024 once, under the factor split only.

Bars (the form is Davis-Kahan with a backward error of K eps ||L||; the constant 16 is not measured on the device):
  eigenvalues lambda_Z, lambda_Z+1 of the record   |l^ - l| <= 16 K 2^-52 lambda_1
  projector V V^T (V = block x MMW_F_FACTOR_ROWNORM)  max entry <= 16 K 2^-52 / relgap,   relgap = (lambda_Z - lambda_Z+1) / lambda_1
  Gram N N^T on the users of row norm >= 1e-3        <= that bound / 1e-6
The projector and Gram bars are skipped where relgap < 1e-6 (here: Z = K, whose lambda_Z is the Laplacian's 0, and L = 0), and the
record must then report the degenerate cut itself.  Everything else is bit equality: alone / in the batch / under a partial take,
the split chain against the single launch, kind 0 before and after, the resident fields.
"""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spectral_oracle as SO  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import _state_at, er_contention_graph, journal_graph, journal_graph_device, mobile_drop  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import spectral_sdp_solver  # noqa: E402
from test_hip_batch_shapes import FIELDS  # noqa: E402

pytestmark = pytest.mark.gpu

RHO, ETA, NATT = 75e-4, 0.04, 2
NAMES = ["one_ap", "c3", "c5", "c8", "c10", "c15", "c17", "iso", "diag"]
ZS = [2, 8, 12, 12, 12, 20, 20, 3, 2]
KS = [2, 27, 75, 192, 300, 675, 867, 6, 5]
SEEDS = np.arange(700, 700 + len(NAMES), dtype=np.uint64)


def hand_state(W, K):
    """(S_gain, Q_asso, h_max) with the given off-diagonal gains, own gain 4 on the diagonal, nobody associated, room for everybody."""
    S = scipy.sparse.csr_matrix(np.asarray(W, dtype=np.float64) + 4.0 * np.eye(K))
    S.sort_indices()
    return S, scipy.sparse.csr_matrix((K, K)), np.full(K, 100.0)


@functools.lru_cache(maxsize=None)
def state(name):
    if name == "one_ap":
        return _state_at(np.array([[3.0, 4.0], [15.5, 12.25]]), np.array([[10.0, 10.0]]))[0]
    if name == "iso":  # users 0..4 all hear each other, asymmetric gains; nothing to or from user 5
        W = np.zeros((6, 6))
        W[:5, :5] = np.random.default_rng(6).uniform(0.1, 2.0, size=(5, 5))
        np.fill_diagonal(W, 0.0)
        return hand_state(W, 6)
    if name == "diag":
        return hand_state(np.zeros((5, 5)), 5)
    if name == "k1024":
        return er_contention_graph(1024, 0.01, 1)
    cell, seed = {"c3": (3, 0), "c5": (5, 1), "c8": (8, 0), "c10": (10, 0), "c15": (15, 0), "c17": (17, 0)}[name]
    return journal_graph(cell, RHO, seed)


@functools.lru_cache(maxsize=None)
def dense(name):
    return SO.Dense(state(name)[0])


def result(b, i):
    """Everything the call leaves for instance i: (block, record bytes, record, row norms)."""
    return b.read_factor(i), b.read(i, _lib.F_FACTOR_INFO, 5).tobytes(), b.factor_info(i), b.factor_row_norms(i)


def same(got, want, what):
    assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), (what, "factor")
    assert got[1] == want[1], (what, "record", got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes(), (what, "row norms")


def same_slots(got, want, idx, what):
    for i in idx:
        assert np.array_equal(got[0][i], want[0][i]) and np.array_equal(got[1][i], want[1][i]) and got[2][i] == want[2][i], (what, NAMES[i], "slots")


class Full:
    pass


@pytest.fixture(scope="module")
def full():
    f = Full()
    f.states = [state(n) for n in NAMES]
    assert [s[0].shape[0] for s in f.states] == KS
    f.b = b = _lib.BatchSolver(ZS, f.states, 1, ETA)
    b.iterate(1, None, SEEDS)  # every resident field is live
    f.before = [[b.read(i, w) for w in FIELDS] for i in range(len(NAMES))]
    # kind 0 on c5 before any spectral call: parity mode on the instance's own X
    f.c5 = NAMES.index("c5")
    f.xavg = [None] * len(NAMES)
    f.xavg[f.c5] = b.read(f.c5, _lib.F_XVAL)
    f.take5 = [i == f.c5 for i in range(len(NAMES))]
    b.factor(take=f.take5, xavg=f.xavg)
    f.kind0 = (b.read_factor(f.c5).copy(), b.read(f.c5, _lib.F_FACTOR_INFO, 5).tobytes())
    b.factor_spectral()
    assert b.factor_call() == {"path": 0, "launches": 1, "sweeps": 0, "widest": len(NAMES)}
    f.res = [result(b, i) for i in range(len(NAMES))]
    f.slots = b.round(NATT, SEEDS, stop_at_first=False)
    yield f
    b.close()


def check_against_the_restatement(name, Z, res):
    """The three bars for one instance; returns the table row (K, Z, sweeps, relgap, eigenvalue / projector / Gram ratio)."""
    N, _, info, rown = res
    d = dense(name)
    K = d.K
    lam1, relgap = d.lam_max(), d.relgap(Z)
    desc = d.lam[::-1]
    assert N.shape == (K, Z) and info["rank"] == Z and 1 <= info["sweeps"] < 30 and not np.any(np.isnan(N)) and not np.any(np.isnan(rown))
    n = np.linalg.norm(N, axis=1)
    assert np.all((n == 0.0) | (np.abs(n - 1.0) <= 4 * SO.EPS)), name  # unit rows, or exactly zero ones
    assert np.array_equal(n == 0.0, rown == 0.0), name
    # eigenvalues
    ebar = 16 * K * SO.EPS * lam1
    eerr = max(abs(info["sigma_rank"] - desc[Z - 1]), abs(info["sigma_next"] - (desc[Z] if Z < K else 0.0)))
    if Z == K:
        assert info["sigma_next"] == 0.0
    r_eig = eerr / ebar if ebar > 0 else float(eerr > 0)
    r_proj = r_gram = float("nan")
    if relgap < 1e-6:  # a degenerate cut: no bar on the kept space, and the record says so itself
        assert info["sigma_rank"] - info["sigma_next"] <= 1e-6 * lam1 + 2 * ebar, name
    else:
        V = d.top(Z)[1]
        pbar = 16 * K * SO.EPS / relgap
        Vd = SO.unnormalised_from(N, rown)
        r_proj = float(np.max(np.abs(SO.projector(Vd) - SO.projector(V)))) / pbar
        rows = SO.big_rows(V)
        r_gram = SO.gram_distance(N, SO.normalise_rows(V), rows) / (pbar / SO.TAU ** 2)
    print("[batch-spectral] %-7s K %4d Z %2d: %2d sweeps, max |cos| %.1e, relgap %.3e, ratios to the bars: eigenvalues %.3f, projector %.2e, Gram %.2e"
          % (name, K, Z, info["sweeps"], info["max_cos"], relgap, r_eig, r_proj, r_gram))
    assert r_eig <= 1.0, (name, "eigenvalues", r_eig)
    if relgap >= 1e-6:
        assert r_proj <= 1.0, (name, "projector", r_proj)
        assert r_gram <= 1.0, (name, "Gram", r_gram)
    return r_eig, r_proj, r_gram


# ---- 1. against the dense restatement
@pytest.mark.parametrize("name", NAMES)
def test_block_matches_the_dense_restatement(full, name):
    i = NAMES.index(name)
    check_against_the_restatement(name, ZS[i], full.res[i])


def test_degenerate_cuts_are_the_two_expected_ones_and_no_other():
    deg = [n for n, Z in zip(NAMES, ZS) if dense(n).relgap(Z) < 1e-6]
    assert deg == ["one_ap", "diag"]


# ---- 2. zero rows
def test_isolated_user_and_zero_laplacian_keep_exact_zeros_and_round(full):
    iso, diag = NAMES.index("iso"), NAMES.index("diag")
    N, _, info, rown = full.res[iso]
    assert not np.any(N[5]) and rown[5] == 0.0 and np.all(rown[:5] > 0.0) and not np.any(np.isnan(N))
    assert np.max(np.abs(np.linalg.norm(N[:5], axis=1) - 1.0)) <= 4 * SO.EPS
    N, _, info, rown = full.res[diag]
    assert not np.any(N) and not np.any(rown) and info["sigma_rank"] == 0.0 and info["sigma_next"] == 0.0 and info["sweeps"] == 1
    z, rem, used = full.slots
    for i in (iso, diag):  # Z allows: nobody interferes beyond h_max and nobody shares an access point
        assert used[i] == NATT and np.all(rem[i] == 0) and np.all((0 <= z[i]) & (z[i] < ZS[i])), NAMES[i]
    one = NAMES.index("one_ap")  # K = 2 = Z rounds as well: the two users share their access point and take one slot each
    assert np.all(rem[one] == 0) and all(sorted(z[one][a].tolist()) == [0, 1] for a in range(NATT))


# ---- 3. the rounding of the block is the oracle's, in index order
def index_ordered(fac):
    """What test_hip_batch_gm.py hands the oracle for a block of unit rows: row k scaled by 2^(K/2 - k) states the batch's visiting
    order (index order) to `argsort(-norm)` and changes no user's preferences; a zero row stays zero and is visited last, where the
    index puts the isolated user too."""
    K = fac.shape[0]
    assert K // 2 + 1 < 500
    return np.ldexp(fac, (K // 2 - np.arange(K))[:, None])


@pytest.mark.parametrize("name", ["one_ap", "c3", "c8", "c17", "iso", "diag"])
def test_round_is_the_oracles_rounding_of_the_block_read_back(full, name):
    i = NAMES.index(name)
    z, rem, used = full.slots
    assert used[i] == NATT
    for a in range(NATT):
        rv = full.b.round_randv(i, int(SEEDS[i]), a)
        assert rv.shape == (ZS[i], ZS[i])
        zo, _, remo, un = orc.rounding_one_attempt(ZS[i], index_ordered(full.res[i][0]), full.states[i], rv)
        zo = np.where(un, -1, zo).astype(np.int32)
        print("[batch-spectral] round %s attempt %d: left over %d (oracle %d), %d slots differ" % (name, a, rem[i][a], remo, int(np.sum(z[i][a] != zo))))
        assert int(rem[i][a]) == remo and np.array_equal(z[i][a], zo), (name, a)


# ---- 4. bitwise: alone, under a partial take, with explicit Zs
@pytest.mark.parametrize("name", NAMES)
def test_each_instance_alone_is_bitwise_the_batch(full, name):
    i = NAMES.index(name)
    one = _lib.BatchSolver([ZS[i]], [full.states[i]], 1, ETA)
    one.factor_spectral([ZS[i]])  # (no iteration has run on this batch)
    same(result(one, 0), full.res[i], (name, "alone"))
    z, rem, used = one.round(NATT, [SEEDS[i]], stop_at_first=False)
    one.close()
    assert np.array_equal(z[0], full.slots[0][i]) and np.array_equal(rem[0], full.slots[1][i]) and used[0] == full.slots[2][i], name


def test_partial_take_is_bitwise_and_the_others_have_no_factor(full):
    b = full.b
    take = [i % 2 == 0 for i in range(len(NAMES))]
    idx = [i for i in range(len(NAMES)) if take[i]]
    b.factor_spectral(take=take)
    for i in idx:
        same(result(b, i), full.res[i], (NAMES[i], "take"))
    same_slots(b.round(NATT, SEEDS, take=take, stop_at_first=False), full.slots, idx, "take")
    with pytest.raises(_lib.MMWError, match="status -3.*instance 1 has no factor"):
        b.round(NATT, SEEDS, take=[i == 1 for i in range(len(NAMES))])
    with pytest.raises(_lib.MMWError, match="instance 1 has no factor"):
        b.read_factor(1)
    # another Z than the slot count: the block's width follows Z, the rounding keeps the instance's slots
    Zs = list(ZS)
    c3 = NAMES.index("c3")
    Zs[c3] = 27
    b.factor_spectral(Zs, take=[i == c3 for i in range(len(NAMES))])
    N = b.read_factor(c3)
    assert N.shape == (27, 27) and b.factor_info(c3)["rank"] == 27 and b.round_randv(c3, 1, 0).shape == (ZS[c3], 27)
    b.factor_spectral(take=[i == c3 for i in range(len(NAMES))])
    same(result(b, c3), full.res[c3], ("c3", "again"))


# ---- 5. bitwise: the split chain against the single launch
@pytest.mark.parametrize("parts", [3, 32, "mixed"])
def test_factor_split_is_bitwise_the_single_launch(full, parts):
    b = full.b
    p = [[1, 3, 32][i % 3] for i in range(len(NAMES))] if parts == "mixed" else [parts] * len(NAMES)
    b.set_factor_split(p)
    try:
        b.factor_spectral()
        call = b.factor_call()
        assert call["path"] == 1 and call["widest"] == sum(len(_lib.BatchSolver.factor_items(K, q)) for K, q in zip(KS, p))
        for i in range(len(NAMES)):
            same(result(b, i), full.res[i], (NAMES[i], "parts", p[i]))
        same_slots(b.round(NATT, SEEDS, stop_at_first=False), full.slots, range(len(NAMES)), ("parts", parts))
    finally:
        b.set_factor_split(None)
    b.factor_spectral(take=[i == 0 for i in range(len(NAMES))])
    assert b.factor_call()["path"] == 0
    same(result(b, 0), full.res[0], "back on the single launch")


def test_k1024_under_the_split_matches_the_restatement():
    st = state("k1024")
    b = _lib.BatchSolver([8], [st], 1, ETA)
    b.set_factor_split(32)
    b.factor_spectral()
    assert b.factor_call()["path"] == 1
    res = result(b, 0)
    z, rem, used = b.round(1, [5])
    b.close()
    check_against_the_restatement("k1024", 8, res)
    assert used[0] == 1 and z[0].shape == (1, 1024)


# ---- 6. kind 0 and the resident fields do not move
def test_kind0_factor_and_every_field_are_what_they_were(full):
    b = full.b
    for i in range(len(NAMES)):
        for w, was in zip(FIELDS, full.before[i]):
            assert np.array_equal(b.read(i, w), was), (NAMES[i], w)
    b.factor(take=full.take5, xavg=full.xavg)
    assert b.read_factor(full.c5).tobytes() == full.kind0[0].tobytes() and b.read(full.c5, _lib.F_FACTOR_INFO, 5).tobytes() == full.kind0[1]
    with pytest.raises(_lib.MMWError, match="status -3.*not a spectral one"):
        b.factor_row_norms(full.c5)
    b.set_factor_split(3)
    b.factor(take=full.take5, xavg=full.xavg)
    b.set_factor_split(None)
    assert b.read_factor(full.c5).tobytes() == full.kind0[0].tobytes() and b.read(full.c5, _lib.F_FACTOR_INFO, 5).tobytes() == full.kind0[1]
    b.factor_spectral(take=full.take5)
    same(result(b, full.c5), full.res[full.c5], "after kind 0")


# ---- 7. refusals by name, before anything runs
def test_refusals_by_name(full):
    b = full.b
    c3 = NAMES.index("c3")
    for bad, what in ((0, "Z = 0"), (28, "Z = 28"), (-1, "Z = -1")):
        Zs = list(ZS)
        Zs[c3] = bad
        b.factor_spectral(take=[i == c3 for i in range(len(NAMES))])
        with pytest.raises(_lib.MMWError, match=r"status -1.*mmw_batch_factor_spectral: instance %d: %s must be in \[1, K = 27\]" % (c3, what)):
            b.factor_spectral(Zs)
    same(result(b, c3), full.res[c3], "a refused call leaves the factors")
    from test_hip_batch_online import geometry, host_state
    over = _lib.BatchSolver([8, 8], [state("c5"), host_state(*geometry("over"))], 1, ETA)
    with pytest.raises(_lib.MMWError, match="status -1.*mmw_batch_factor_spectral: instance 1: K = 1025 exceeds the epilogue limit 1024"):
        over.factor_spectral()
    with pytest.raises(_lib.MMWError, match="status -3.*instance 0 has no factor"):
        over.round(1, [1, 2], take=[True, False])
    over.factor_spectral(take=[True, False])
    assert over.read_factor(0).shape == (75, 8)
    over.close()


# ---- 8. the Python surface
def test_baselines_many_spectral_is_the_same_steps_done_by_hand():
    drops = [mobile_drop(5, RHO, 3), mobile_drop(7, RHO, 1)]
    B = len(drops)
    env = _lib.BatchEnv([d.ap_locs for d in drops], [d.K for d in drops], min_sinr=batch.min_sinr_dec())
    env.move([d.sta_locs for d in drops])
    states = [env.state(i) for i in range(B)]
    Zs = [8, 12]
    b = _lib.BatchSolver(Zs, states, 1, ETA)
    sd = np.array([batch.probe_seed(5, i, 0x40000 | 3) for i in range(B)], dtype=np.uint64)
    own = None
    for src, rnd in ((b, lambda: b.round(10, sd)), ((b, env), lambda: b.round_env(env, 10, sd))):
        got = batch.baselines_many(src, Zs, methods=("spectral",), seed=5)
        own = got if own is None else own
        b.factor_spectral(Zs)
        z, rem, used = rnd()
        for i in range(B):
            f = batch._finish(z, rem, used, i, Zs[i], int(sd[i]))
            assert sorted(got[i]) == ["spectral"] and np.array_equal(got[i]["spectral"][0], f[0]) and got[i]["spectral"][1:] == f[1:]
            assert np.all((0 <= f[0]) & (f[0] < Zs[i]))
    mixed = batch.baselines_many(b, Zs, methods=("rand", "spectral"), seed=5)
    assert sorted(mixed[0]) == ["rand", "spectral"] and all(np.array_equal(mixed[i]["spectral"][0], own[i]["spectral"][0]) for i in range(B))
    assert sorted(batch.baselines_many(b, Zs, seed=5)[0]) == ["masso", "mgain", "rand"]
    with pytest.raises(ValueError, match="slot counts are not Zs"):
        batch.baselines_many(b, [8, 13], methods=("spectral",))
    b.close()
    env.close()


def test_class_on_the_device_is_factor_spectral_of_a_batch_of_one():
    st = state("c3")
    alg = spectral_sdp_solver(100, 2, 1.)
    ok, blk = alg.run_with_state(0, 8, st)
    b = _lib.BatchSolver([8], [st], 1, ETA)
    b.factor_spectral()
    want = b.read_factor(0)
    b.close()
    assert ok is True and blk.shape == (27, 8) and blk.tobytes() == want.tobytes()
    logs = alg.LOGGED_NP_DATA
    assert sorted(logs) == ["spectral_problem_setup", "spectral_solve"] and all(logs[k].shape == (1, 6) and logs[k][0, 3:5].tolist() == [8.0, 27.0] for k in logs)
    np.random.seed(3)
    z_vec, Z, rem = alg.rounding(8, blk, st)
    assert Z == 8 and z_vec.shape == (27,) and np.all((0 <= z_vec) & (z_vec < 8)) and rem >= 0
    alg.close()
    # a device-resident state goes through its host copy
    denv = journal_graph_device(3, RHO, 0)[1]
    ds = _lib.DeviceState(denv)
    ok, blk2 = alg.run_with_state(1, 8, ds)
    d = SO.Dense(ds.host()[0])
    denv.close()
    V = d.top(8)[1]
    assert blk2.shape == (27, 8) and SO.gram_distance(blk2, SO.normalise_rows(V), SO.big_rows(V)) <= 16 * 27 * SO.EPS / d.relgap(8) / SO.TAU ** 2
