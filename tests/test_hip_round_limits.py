"""GPU: mmw_round at the edges of its windows, tiles, tie rules and schedule -- EXACT agreement of the integer slot assignment and
of the remainder with the CPU reference of tests/helpers/round_cases.py on instances designed to reach one path each (the preference
window of k_greedy_b and the rows beyond it, neighbour and association lists longer than their register windows, ties in both sorts,
the tile and group seams of k_rank_count, the zero padding of k_project_mfma, interactions at the edge of the schedule's window, the
slot table in global memory), plus the refusal of a slot count the greedy kernel cannot hold.  test_round_cases_host.py asserts,
without a GPU, that every instance reaches its path.  No tolerance anywhere: the outputs are integers.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from sig_sdp_mmw_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import round_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

BUILDERS = {"clique330": lambda: rc.shared_order_clique(330, 330),
            "clique325": lambda: rc.shared_order_clique(330, 325),
            "clique_mixed": lambda: rc.shared_order_clique(330, 325, signs="mixed"),
            "clique_batch": lambda: rc.shared_order_clique(330, 325, signs="mixed", nbatch=3),
            "hubs": rc.hubs_and_leaves,
            "hubs_batch": lambda: rc.hubs_and_leaves(nbatch=3),
            "global_slots": rc.global_slots}
BUILDERS.update({n: functools.partial(rc.tie_cases, n) for n in rc.TIE_CASES})
BUILDERS.update({"proj_D%d_Z%d_K%d" % c: functools.partial(rc.projection_edges, *c) for c in rc.PROJECTION_CASES})
BUILDERS.update({n: functools.partial(rc.order_chains, n) for n in rc.CHAIN_CASES})


@functools.lru_cache(maxsize=None)
def case(name):
    """(state, Z, gX, randv, [(z, rem) of the reference per batch entry]), computed once and left unchanged."""
    state, Z, gX, rv = BUILDERS[name]()
    want = [rc.reference_attempt(Z, gX, state, rv[a])[:2] for a in range(rv.shape[0])]
    gX.setflags(write=False)
    rv.setflags(write=False)
    return state, Z, gX, rv, want


def check(got, want, what):
    z, rem = got
    assert len(want) == z.shape[0] == rem.shape[0]
    for a, (zr, remr) in enumerate(want):
        assert int(rem[a]) == remr, (what, a)
        assert np.array_equal(z[a], zr), (what, a, np.flatnonzero(z[a] != zr)[:8])


@pytest.mark.parametrize("name", [n for n in BUILDERS if not n.endswith("_batch")])
def test_designed_instance_matches_the_reference_exactly(name):
    state, Z, gX, rv, want = case(name)
    s = _lib.Solver(2, state, 1, 0.1)  # the handle's own Z is independent of round's
    check(s.round(Z, gX, rv), want, name)
    s.close()


@pytest.mark.parametrize("name", ["clique_batch", "hubs_batch"])
def test_batch_entries_are_independent_and_buffers_are_reused(name):
    state, Z, gX, rv, want = case(name)
    assert rv.shape[0] == 3
    s = _lib.Solver(2, state, 1, 0.1)
    check(s.round(Z, gX, rv), want, name)
    for a in range(3):  # each entry equals its own solo call
        check(s.round(Z, gX, rv[a]), want[a:a + 1], (name, "solo", a))
    # the same handle with a smaller Z and a smaller D': the buffers are reused, nothing stale is read
    K = gX.shape[0]
    rng = np.random.default_rng(7)
    Z2, Dp2 = (5, 3) if gX.shape[1] > 3 else (40, 1)  # (the clique's D' is 1 already: a smaller Z only)
    gX2 = rng.standard_normal((K, Dp2)) * rng.uniform(0.2, 2.0, size=(K, 1))
    rv2 = rng.standard_normal((2, Z2, Dp2))
    rv2 = rc.normalise(rv2) if Dp2 > 1 else rv2  # (normalised rows of one column are +-1: nothing but ties)
    want2 = [rc.reference_attempt(Z2, gX2, state, rv2[a])[:2] for a in range(2)]
    again = s.round(Z2, gX2, rv2)
    check(again, want2, (name, "smaller"))
    f = _lib.Solver(2, state, 1, 0.1)
    fresh = f.round(Z2, gX2, rv2)
    f.close()
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1])
    check(s.round(Z, gX, rv), want, (name, "back"))
    s.close()


def test_a_slot_count_beyond_the_lds_is_refused_before_anything_runs():
    """Z = 4801: 8 rows of Z flags no longer fit the 150 KiB the greedy kernel may take.  The refusal comes before any allocation,
    copy, launch or timer bracket, so the handle and its kernel timers are as they were."""
    state, Z, gX, rv, want = case("proj_D5_Z17_K65")
    K = gX.shape[0]
    s = _lib.Solver(2, state, 1, 0.1)
    big = np.zeros((1, 4801, 1))
    with pytest.raises(_lib.MMWError, match="exceed the greedy kernel's LDS"):
        s.round(4801, np.ones((K, 1)), big)
    check(s.round(Z, gX, rv), want, "after the refusal")
    s.set_profile(1)
    check(s.round(Z, gX, rv), want, "timed")
    with pytest.raises(_lib.MMWError, match="exceed the greedy kernel's LDS"):
        s.round(4801, np.ones((K, 1)), big)
    kt = s.kernel_times()
    assert kt["project"][1] == 1 and kt["greedy"][1] == 1 and kt["project"][0] > 0 and kt["greedy"][0] > 0
    check(s.round(Z, gX, rv), want, "timed, after the refusal")
    kt = s.kernel_times()
    assert kt["project"][1] == 2 and kt["greedy"][1] == 2
    s.set_profile(0)
    s.close()
