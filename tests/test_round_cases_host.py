"""CPU-only: the designed rounding instances of tests/helpers/round_cases.py reach what they were designed for.

test_hip_round_limits.py runs these instances on the device because of one path each: a chunk of the preference window, the rows
beyond it, a neighbour list longer than the register window, a tie, a seam of the ranking tiles, an interaction at the edge of the
schedule's window.  A test like that passes just as well when its instance misses the path, so the conditions are asserted here,
on the trace of the CPU reference alone -- they are conditions of the instances, not measurements.  The reference itself is tied to
the pinned oracle on every rounding fixture of tests/golden/run_*.npz (tie-free, so the stable sorts change nothing there).
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, state_from
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import round_cases as rc  # noqa: E402


def ref(case, a=0, **kw):
    state, Z, gX, rv = case
    return rc.reference_attempt(Z, gX, state, rv[a], **kw)


def test_reference_equals_the_pinned_oracle_on_every_fixture(run_case):
    name, g = run_case
    state = state_from(g)
    for pre, Zk, gXk in (("att_", "round_Z", "round_gX"), ("small_att_", "small_Z", "small_gX")):
        Z, gX = int(g[Zk]), g[gXk]
        for a in range(g[pre + "randv"].shape[0]):
            rv = rc.normalise(g[pre + "randv"][a])
            zo, _, remo, un = orc.rounding_one_attempt(Z, gX, state, rv, randint=lambda Zs, size: np.full(size, -1))
            z, rem, tr = rc.reference_attempt(Z, gX, state, rv)
            assert rem == remo == int(g[pre + "rem"][a]), (name, pre, a)
            assert np.array_equal(z, zo.astype(np.int64)), (name, pre, a)
            assert np.array_equal(z[~un], g[pre + "z"][a][~un].astype(np.int64))
            # the trace agrees with the result: a placed user's slot is the entry of its preference list at its depth
            pref = np.argsort(-(rv @ gX.T), axis=0, kind="stable")
            placed = np.flatnonzero(z >= 0)
            assert np.array_equal(pref[tr.depth[placed], placed], z[placed])
            assert np.all(tr.depth[z < 0] == Z) and all(len(tr.rejected[k]) == tr.depth[k] for k in range(len(z)))


def all_cases():
    yield "clique330", rc.shared_order_clique(330, 330)
    yield "clique325", rc.shared_order_clique(330, 325)
    yield "clique_mixed", rc.shared_order_clique(330, 325, signs="mixed")
    yield "hubs", rc.hubs_and_leaves()
    for n in rc.TIE_CASES:
        yield n, rc.tie_cases(n)
    for Dp, Z, K in rc.PROJECTION_CASES:
        yield "proj%d_%d_%d" % (Dp, Z, K), rc.projection_edges(Dp, Z, K)
    for n in rc.CHAIN_CASES:
        yield n, rc.order_chains(n)
    yield "global_slots", rc.global_slots()


def test_every_instance_is_a_state_the_handle_accepts():
    for name, (state, Z, gX, rv) in all_cases():
        rc.check_state(state)
        K = state[0].shape[0]
        assert gX.shape[0] == K and rv.ndim == 3 and rv.shape[1:] == (Z, gX.shape[1]), name
        if K <= 1700:  # build_pattern itself, on a host-only handle
            _lib.Solver(2, state, 1, 0.1, device=-1).close()


@pytest.mark.parametrize("Z,rem_want", [(330, 0), (325, 5)])
def test_clique_walks_every_chunk_of_the_preference_window(Z, rem_want):
    case = rc.shared_order_clique(330, Z)
    z, rem, tr = ref(case)
    assert rem == rem_want
    depths = set(tr.depth[z >= 0].tolist())
    assert {0, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, Z - 1} <= depths
    assert int((tr.depth == Z).sum()) == rem_want and np.all(z[tr.depth == Z] == -1)
    assert tr.qdeg.max() == 329 > 64
    # every rejection of a clique user is check (c), and the deepest ones come from Q positions on both sides of 64
    pos = [p for _, _, c, ps in tr.rejections() for p in ps if c == rc.CHECK_C]
    assert min(pos) < 64 < max(pos) and all(c == rc.CHECK_C for k, _, c, _ in tr.rejections() if k < 330)
    # outside the clique: check (a) decides at a slot beyond the register window, and the next user there is not kept out
    assert Z - 1 >= 256 and z[332] == Z - 1 and tr.rejected[333] == [(Z - 1, rc.CHECK_A, ())] and z[333] == Z - 2
    assert z[334] == Z - 1 and tr.rejected[334] == ()
    at = {int(k): i for i, k in enumerate(tr.order)}
    assert at[332] == 0 and at[333] - at[332] > 64 and at[334] - at[333] > 64 and at[334] < 300
    zc = z[:330]
    assert sorted(zc[zc >= 0].tolist()) == list(range(Z))  # one user of the access point per slot, every slot taken


def test_mixed_clique_fills_both_ends():
    case = rc.shared_order_clique(330, 325, signs="mixed")
    (S, Q, h), Z, gX, rv = case
    z, rem, tr = ref(case)
    zc = z[:330]
    assert rem == 5 and sorted(zc[zc >= 0].tolist()) == list(range(Z))
    order = tr.order[np.isin(tr.order, np.arange(330))]
    assert z[order[gX[order, 0] > 0][0]] == 0 and z[order[gX[order, 0] < 0][0]] == Z - 1
    # the last placed users walk through their own side's slots into the other side's; five walk the whole list
    assert int((tr.depth == Z).sum()) == 5 and 128 < tr.depth[z >= 0].max() < Z - 1


def test_hubs_are_refused_through_the_far_end_of_their_lists():
    state, Z, gX, rv, info = rc.hubs_and_leaves_info()
    z, rem, tr = rc.reference_attempt(Z, gX, state, rv[0])
    hubs, t, W = info["hubs"], info["t"], info["W"]
    assert tuple(int(tr.deg[h]) for h in hubs) == rc.HUB_DEGS and rem == 0
    pos_of = {k: [i for i, u in enumerate(tr.order) if u == k][0] for k in hubs + [W]}
    assert [pos_of[h] for h in hubs] == list(range(1495, 1499)) and pos_of[W] == 1499  # leaves, then the hubs in order, then W
    hp = info["hub_pref"]
    assert tr.rejected[hubs[0]] == [(int(hp[0, 0]), rc.CHECK_B, (255,))]       # the last register of the window
    assert tr.rejected[hubs[1]] == [(int(hp[1, 0]), rc.CHECK_B, (256,))]       # the first element beyond it
    assert tr.rejected[hubs[2]] == [(int(hp[2, 0]), rc.CHECK_B, (299,))] and z[hubs[2]] == t
    r3 = tr.rejected[hubs[3]]
    assert [x[:2] for x in r3] == [(t, rc.CHECK_B), (int(hp[3, 1]), rc.CHECK_B)] and r3[1][2] == (699,) and len(r3[0][2]) == 2
    assert z[hubs[3]] == hp[3, 2]
    assert tr.rejected[W] == [(t, rc.CHECK_A, ())]
    # without what hub 2 adds from beyond its register window, hub 3 and W take t
    z2, rem2, tr2 = rc.reference_attempt(Z, gX, state, rv[0], drop_adds={hubs[2]: 256})
    assert z2[hubs[3]] == t and z2[W] == t and tr2.rejected[hubs[3]] == () and tr2.rejected[W] == ()
    assert np.array_equal(np.flatnonzero(z2 != z), np.sort([hubs[3], W]))


@pytest.mark.parametrize("name", rc.TIE_CASES)
def test_tie_rules_decide_the_output(name):
    case = rc.tie_cases(name)
    state, Z, gX, rv = case
    K = gX.shape[0]
    z, rem, tr = ref(case)
    nrm = np.linalg.norm(gX, axis=1)
    assert np.all(np.diff(nrm[tr.order]) <= 0)
    tied = nrm[tr.order][1:] == nrm[tr.order][:-1]
    assert np.all(np.diff(tr.order)[tied] > 0) and tied.sum() > K // 2
    if name.startswith("equal"):
        assert np.array_equal(tr.order, np.arange(K))
    if name == "blocks4097":
        run = (np.arange(K) + 128) // 256
        assert np.array_equal(np.diff(run[tr.order]) == 0, tied) and len(set(nrm.tolist())) == 17
        for seam in range(256, K, 256):  # every run of equal keys straddles a tile seam, in index order
            i = int(np.flatnonzero(tr.order == seam - 1)[0])
            assert tr.order[i + 1] == seam
    if name == "mixed300":
        assert (nrm == 0).sum() >= 20 and len(np.unique(gX, axis=0)) < K - 20
        d = gX[nrm == 3.0]
        assert len(np.unique(np.abs(d).max(axis=1))) == 2  # (3, 0, 0) and (1, 2, 2): equal in norm, not in direction
    assert np.array_equal(rv[0, 0], rv[0, 1]) and tr.depth.max() >= 2
    zo = ref(case, order_ties="higher")[0]
    zp = ref(case, pref_ties="higher")[0]
    assert not np.array_equal(zo, z), "the visiting order's tie rule does not decide this case: choose another seed or state"
    assert not np.array_equal(zp, z), "the preference lists' tie rule does not decide this case: choose another seed or state"


def test_projection_cases_cover_the_padding_edges():
    Dps, Zs, Ks = (set(c[i] for c in rc.PROJECTION_CASES) for i in range(3))
    assert Dps == {1, 3, 4, 5, 63, 64, 65, 130} and Zs == {2, 15, 16, 17, 65} and Ks == {17, 63, 64, 65, 130}
    for Dp, Z, K in rc.PROJECTION_CASES:
        case = rc.projection_edges(Dp, Z, K)
        assert case[3].shape == (3, Z, Dp)
        z, rem, tr = ref(case)
        assert tr.qdeg.max() >= min(Z, K) - 1
        assert tr.depth.max() >= max(1, min(Z, K) // 2), "the clique's users must walk deep into their preference lists"


def swapped(order, i, j):
    o = np.array(order)
    o[i], o[j] = o[j], o[i]
    return o


@pytest.mark.parametrize("name,lag", [("path", 1), ("lag32", 32), ("lag33", 33)])
def test_chain_pairs_compete(name, lag):
    case = rc.order_chains(name)
    K = case[2].shape[0]
    z, rem, tr = ref(case)
    assert np.array_equal(tr.order, np.arange(K))
    if name == "path":
        assert K > 8192  # one user per step: the steps cross the schedule's staging chunk
    # a user that its predecessor in the chain kept out of a slot: deciding the two the other way round changes the result
    found = 0
    for k, zz, c, pos in tr.rejections(rc.CHECK_C):
        if k >= lag and z[k - lag] == zz and found < 3:
            z2 = ref(case, order=swapped(tr.order, k - lag, k))[0]
            found += int(not np.array_equal(z2, z))
    assert found >= 1
    assert sum(1 for _ in tr.rejections(rc.CHECK_C)) > K // 8


def test_common_out_neighbour_pairs_compete_at_every_lag():
    case = rc.order_chains("common")
    (S, Q, h), Z, gX, rv = case
    z, rem, tr = ref(case)
    assert np.array_equal(tr.order, np.arange(gX.shape[0]))
    assert sorted(rc.COMMON_PAIRS) == [1, 8, 31, 32]
    for lag, pairs in rc.COMMON_PAIRS.items():
        for x, y in pairs:
            assert y - x == lag and S[x, y] == 0 and S[y, x] == 0 and Q[x, y] == 0
            (n,) = [int(c) for c in S[x].indices if c != x]
            assert [int(c) for c in S[y].indices if c != y] == [n]
            assert n < x and z[x] == z[n] and tr.rejected[x] == () and tr.rejected[y] == [(int(z[n]), rc.CHECK_B, (0,))]
            z2 = ref(case, order=swapped(tr.order, x, y))[0]
            assert z2[y] == z[n] and z2[x] != z[n]


def test_global_slot_case_is_beyond_the_lds_table():
    state, Z, gX, rv = rc.global_slots()
    K = gX.shape[0]
    assert 8 * Z * 4 <= 150 * 1024 < 8 * Z * 4 + 4 * K and Z > 256
    z, rem, tr = rc.reference_attempt(Z, gX, state, rv[0])
    assert rem == 0 and tr.depth.max() >= 1
