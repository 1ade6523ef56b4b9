"""The head split of the batched solver (`BatchSolver.set_head_split`, csrc/kernels_batch_head.h): the head of an iteration as the
launches [gap] avg, dual, fold, loss (and plan on the row split's path), the row sums of X as a launch of their own, must give, bit for
bit, what the single-launch kernel `k_mmw_batch` gives.

The cases, their states, slot counts, step sizes and exponential settings are those of the same names in
tests/test_hip_batch_shapes.py; the single-launch references and their iteration counts are those of tests/test_hip_batch_rows.py
(imported from there, so one run serves both files).  (head parts, column parts, row parts) and what a case reaches:

  case                  K, D       head, parts, rows   what it reaches
  tiny                  2, 4       3, 1, 1             an empty row range
  d_gt_k                5, 80      7, 16, 1            more parts than rows; the column split's path
  odd_d                 75, 3      4, 1, 4             the row split's path; K not divisible
  ng8                   243, 64    3, 3, 3
  ng3_substeps (eta 5)  300, 170   5, 7, 5
  ng1_group2            675, 257   11, 16, 1           K and C wrap the 512-thread map of every fold
  ng1_group2_alone      675, 257   11, 1, 1            the head split alone
  fallback              300, 24    2, 1, 2             one iteration
  limits                4096, 512  64, 32, 64          one iteration

The star graph of tests/test_hip_batch_rows.py (K = 65) at 16 head parts: the hub's part stands alone and four parts are empty.  Its Q
is empty (E_asso = 0); so is the hand-made K = 3 state's, which mmw_batch_create accepts.

The mixed batch has one rank_radio and one (max_order, tol) for all its instances, as every batch has (see tests/test_hip_batch_rows.py,
whose instances, seeds and solo references it shares), with per-instance head parts, one of them 1.

Mutations of csrc/kernels_batch_head.h and csrc/batch_head.h, tried by hand once each and not committed; the whole file was run
against each, and these tests turned red:
  * the fold using a per-part partial of `tot` (the terms c < K and the rest reduced apart, then added): every case but fallback, the
    empty Q, the four mixed batches, the refusals test;
  * a row range starting one row late (in the work table, for every part but the first): all twenty tests;
  * `k_batch_head_x` taking the trace with another thread map (contiguous chunks of ceil(K / 512) rows per thread, which is the
    single launch's map up to K = 512): ng1_group2, ng1_group2_alone, the four mixed batches, the "auto" test (K = 675 each); limits
    (K = 4096, one iteration) stayed green;
  * the missing barrier in `k_batch_head_loss` (a race, so what it shows varies from run to run): odd_d and the philox mixed batch.
"""
import functools

import numpy as np
import pytest
import scipy.sparse

import test_hip_batch_rows as rows_t
import test_hip_batch_shapes as shapes
from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation
from sig_sdp_mmw_amd.graphs import journal_graph

pytestmark = pytest.mark.gpu

FIELDS = rows_t.FIELDS
CASE = rows_t.CASE
fields, assert_same, calls_of = rows_t.fields, rows_t.assert_same, rows_t.calls_of
assert FIELDS == (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_SKETCH,
                  _lib.F_EXPM_INFO)
# id: (case, head parts, column parts, row parts)
HEAD = {"tiny": ("tiny", 3, 1, 1), "d_gt_k": ("d_gt_k", 7, 16, 1), "odd_d": ("odd_d", 4, 1, 4), "ng8": ("ng8", 3, 3, 3),
        "ng3_substeps": ("ng3_substeps", 5, 7, 5), "ng1_group2": ("ng1_group2", 11, 16, 1), "ng1_group2_alone": ("ng1_group2", 11, 1, 1),
        "fallback": ("fallback", 2, 1, 2), "limits": ("limits", 64, 32, 64)}


def set_all(b, head, parts, rows):
    b.set_split(parts)
    b.set_row_split(rows)
    b.set_head_split(head)


def head_launches(nit, gap, path):
    """[gap] avg, dual, fold, loss, [plan], xrows, x per iteration"""
    return nit * (6 + (1 if gap else 0) + (1 if path == 2 else 0))


@pytest.mark.parametrize("name", list(HEAD))
def test_head_split_is_bitwise_the_single_launch(name):
    cname, head, parts, rows = HEAD[name]
    case = CASE[cname]
    nit = rows_t.ROWS[cname][2]
    seed = shapes.seed_of(case)
    want = rows_t.case_single_launch(cname)
    b = shapes.new_batch(case, nit, case[7])
    set_all(b, head, parts, rows)
    assert b.head_split_parts == [head]
    assert b.split_parts == ([parts] if parts > 1 else None) and b.row_split_parts == ([rows] if rows > 1 else None)
    path = 2 if rows > 1 else 1
    # entry ranges of X: the column parts on path 1, slices x row parts on path 2
    ranges = parts if path == 1 else _lib.BatchSolver.split_slices(case[9][1], parts)[1] * rows
    for n in calls_of(nit):
        b.iterate(n, None, [seed])
        assert b.split_call()["path"] == path
        assert b.head_call() == {"on": True, "launches": head_launches(n, False, path), "widest": max(head, ranges)}
    assert b.iterations_done(0) == nit
    got = fields(b, 0)
    bd = b.head_ranges(0, head)
    K, C = b.sizes[0]["K"], b.sizes[0]["C"]
    b.close()
    info = got[_lib.F_EXPM_INFO]
    print("[batch-head] %-16s K %4d D %3d head %2d parts %2d rows %2d  plan (%d, %d)  ranges %s" % (name, K, case[9][1], head, parts, rows, int(info[2]), int(info[1]), bd[:8]))
    assert_same(got, want, name)
    assert bd[0] == 0 and bd[-1] == K and len(bd) == head + 1
    if cname in ("tiny", "d_gt_k"):
        assert any(a == b_ for a, b_ in zip(bd, bd[1:]))  # K < head parts: a row range is empty
    if cname == "odd_d":
        assert K % head != 0
    if cname == "ng1_group2":
        assert K > shapes.NT and C > 2 * shapes.NT  # the folds' thread maps wrap
    if cname == "fallback":
        assert int(info[2]) == shapes.NSUB_MAX and int(info[1]) == 1


# ---- a dense row, and states without association pairs
def test_a_dense_row_leaves_head_parts_empty():
    Z, nit, eta, seed, head = 4, 4, 0.3, [77], 16
    one = _lib.BatchSolver([Z], [rows_t.star_state()], nit, eta)
    one.set_expm(16, 1e-13)
    indptr = one.read_i32(0, _lib.I_L_INDPTR)
    assert one.sizes[0]["E_asso"] == 0
    one.iterate(nit, None, seed)
    want = fields(one, 0)
    one.close()
    for rows in (1, 16):  # both paths
        b = _lib.BatchSolver([Z], [rows_t.star_state()], nit, eta)
        b.set_expm(16, 1e-13)
        bd = b.head_ranges(0, head)
        assert bd == _lib.BatchSolver.row_bounds(indptr, head)
        assert bd[:7] == [0, 1, 1, 1, 1, 1, 5]  # the hub alone, then four empty parts
        b.set_row_split(rows)
        b.set_head_split(head)
        for n in calls_of(nit):
            b.iterate(n, None, seed)
        assert b.head_call()["on"] and b.split_call()["path"] == (2 if rows > 1 else 1)
        assert_same(fields(b, 0), want, ("star", rows))
        b.close()


def test_a_state_whose_q_is_empty_at_k_3():
    """Hand-made: S dense 3 x 3, Q empty, so E_asso = 0 and no part owns a pair.  mmw_batch_create accepts the state."""
    rng = np.random.default_rng(11)
    S = scipy.sparse.csr_matrix(rng.uniform(0.1, 3.7, (3, 3)))
    st = (S, scipy.sparse.csr_matrix((3, 3)), np.ones(3))
    Z, nit, seed = 2, 5, [31]
    one = _lib.BatchSolver([Z], [st], nit, 0.2)
    assert one.sizes[0]["K"] == 3 and one.sizes[0]["E_asso"] == 0
    one.iterate(nit, None, seed)
    want = fields(one, 0)
    one.close()
    for head, rows in ((2, 1), (4, 1), (3, 2)):
        b = _lib.BatchSolver([Z], [st], nit, 0.2)
        b.set_row_split(rows)
        b.set_head_split(head)
        for n in calls_of(nit):
            b.iterate(n, None, seed)
        assert b.head_call()["on"]
        assert_same(fields(b, 0), want, ("empty Q", head, rows))
        b.close()


# ---- the mixed batch
# head parts of rows_t.MIXED's instances, in order (ng8 keeps its head on one workgroup)
MIXED_HEAD = {"tiny": 3, "d_gt_k": 7, "odd_d": 4, "ng8": 1, "ng3_substeps": 5, "ng1_group2": 11, "substeps_order": 2, "fallback": 2, "limits": 64}


def new_mixed(insts, rows_on):
    big = _lib.BatchSolver([x[1] for x in insts], [shapes.state(x[0]) for x in insts], [x[5] for x in insts], 0.04, rank_radio=1)
    big.set_eta([x[2] for x in insts])
    big.set_expm(16, 1e-13)
    set_all(big, [MIXED_HEAD[m[0]] for m in rows_t.MIXED], [x[4] for x in insts], [x[3] for x in insts] if rows_on else None)
    return big


@pytest.mark.parametrize("mode", ["philox", "randv", "gap", "gap_alone"])
def test_mixed_batch_every_instance_is_bitwise_its_single_launch_solo_run(mode):
    """philox: the row split's path, then an instance taken out by set_slots.  randv: uploaded sketches on the column split's path.
    gap: the gap on, the row split's path.  gap_alone: the gap on and the head split alone."""
    insts = rows_t.mixed_instances()
    heads = [MIXED_HEAD[m[0]] for m in rows_t.MIXED]
    assert 1 in heads and max(heads) == _lib.BATCH_MAX_HEAD_PARTS
    assert {0.04, 5.0} <= {x[2] for x in insts if x[0] == "er300" and x[1] == 24}
    seeds = np.array([x[6] for x in insts], dtype=np.uint64)
    rows_on = mode in ("philox", "gap")
    big = new_mixed(insts, rows_on)
    if mode == "gap_alone":
        big.set_split(None)
    gap = mode.startswith("gap")
    if gap:
        big.set_gap(True)
    path = 2 if rows_on else 1
    done = [0] * len(insts)
    for call, n in enumerate((1, 3, 1)):
        if mode == "randv":
            blocks = []
            for i, x in enumerate(insts):
                nb = max(0, min(n, x[5] - done[i]))
                blocks.append(np.stack([big.sketch(i, x[6], done[i] + k) for k in range(nb)]) if nb else None)
                done[i] += nb
            big.iterate(n, blocks)
        else:
            big.iterate(n, None, seeds)
        hc = big.head_call()
        assert big.split_call()["path"] == path and hc["on"] and hc["launches"] == head_launches(n, gap, path)
        if call == 0:  # every instance runs
            widest_all = hc["widest"]
            assert widest_all >= sum(heads)
    for i, (st, D, eta, rows, parts, nit, seed) in enumerate(insts):
        assert big.iterations_done(i) == nit
        want, wgap = rows_t.solo_single_launch(st, D, eta, nit, seed, gap)
        assert_same(fields(big, i), want, (mode, i, st, D, heads[i]))
        if gap:
            rows_g, steps_g = big.gap_log(i)
            assert np.all(np.isfinite(rows_g)) and np.array_equal(rows_g, wgap[0]) and np.array_equal(steps_g, wgap[1]), (i, st)
    if mode == "philox":
        # the largest instance is taken out (Z <= 0, nrun = 0), the others restart with one count for all: the settings hold
        nit2 = 3
        big.set_slots([x[1] if i + 1 < len(insts) else 0 for i, x in enumerate(insts)], nit2)
        assert big.head_split_parts == heads and big.row_split_parts == [x[3] for x in insts] and big.split_parts == [x[4] for x in insts]
        big.iterate(2, None, seeds)
        big.iterate(1, None, seeds)
        assert big.split_call()["path"] == 2 and big.head_call()["on"]
        assert big.head_call()["widest"] < widest_all  # the instance that sits out has no workgroup
        for i, (st, D, eta, rows, parts, nit, seed) in enumerate(insts[:-1]):
            assert big.iterations_done(i) == nit2
            assert_same(fields(big, i), rows_t.solo_single_launch(st, D, eta, nit2, seed, False)[0], ("after set_slots", i, st))
        assert big.iterations_done(len(insts) - 1) == 0
    big.close()


# ---- the setting's lifecycle
def test_refusals_and_what_the_setting_survives():
    case = CASE["ng8"]
    nit, seed = 3, [shapes.seed_of(case)]
    one = shapes.new_batch(case, nit, 1e-13)
    one.iterate(nit, None, seed)
    want = fields(one, 0)
    off_call = {"on": False, "launches": 0, "widest": 0}
    assert one.head_call() == off_call and one.split_call() == {"path": 0, "launches": 1, "idle": 0, "widest": 1}
    b = shapes.new_batch(case, nit, 1e-13)
    assert b.head_call() == off_call
    b.set_head_split(3)
    for bad in (0, -1, _lib.BATCH_MAX_HEAD_PARTS + 1):
        with pytest.raises(_lib.MMWError, match=r"mmw_batch_set_head_split: instance 0: parts = -?\d+ is outside \[1, 64\]"):
            b.set_head_split(bad)
        assert b.head_split_parts == [3]
    b.iterate(nit, None, seed)
    # the refused values left the setting; alone it is the column split's path with one slice and one entry range
    assert b.head_call() == {"on": True, "launches": 6 * nit, "widest": 3}
    assert b.split_call() == {"path": 1, "launches": 7 * nit, "idle": 0, "widest": 3}
    assert_same(fields(b, 0), want, "after the refusals")
    # all ones or None: every launch is what it is without the head split, and the record says off
    for off in ([1], None):
        b.reset(nit)
        b.set_head_split(off)
        assert b.head_split_parts is None
        b.iterate(nit, None, seed)
        assert b.head_call() == off_call and b.split_call() == {"path": 0, "launches": 1, "idle": 0, "widest": 1}
        assert_same(fields(b, 0), want, "off")
    b.reset(nit)
    b.set_split(3)
    b.iterate(nit, None, seed)
    assert b.head_call() == off_call and b.split_call() == {"path": 1, "launches": 3 * nit, "idle": 0, "widest": 3}
    # the setting survives reset and set_slots to another D
    b.set_head_split(5)
    b.reset(nit)
    assert b.head_split_parts == [5]
    b.iterate(nit, None, seed)
    assert b.head_call() == {"on": True, "launches": 6 * nit, "widest": 5} and b.split_call()["path"] == 1
    assert_same(fields(b, 0), want, "head 5 x parts 3 after reset")
    b.set_row_split(2)
    Z2 = 20
    b.set_slots([Z2], nit)
    one.set_slots([Z2], nit)
    assert b.head_split_parts == [5] and b.split_parts == [3] and b.row_split_parts == [2] and b.sizes[0]["D"] == 40
    b.iterate(nit, None, seed)
    one.iterate(nit, None, seed)
    assert b.split_call()["path"] == 2 and b.head_call() == {"on": True, "launches": 7 * nit, "widest": 6}
    assert_same(fields(b, 0), fields(one, 0), "after set_slots")
    b.close()
    one.close()


def test_auto_is_taken_again_after_set_slots():
    """Two instances of K = 243 and 675, then the second one alone: "auto" follows the instances that run."""
    states = [journal_graph(9, 75e-4, 0), journal_graph(15, 75e-4, 0)]
    nit, seeds = 2, [5, 6]
    b = _lib.BatchSolver([8, 8], states, nit, 0.04)
    b.set_head_split("auto", cus=16)
    first = b.head_split_parts
    assert first == b.suggest_head_split(16) and max(first) > 1
    b.set_slots([0, 4], nit)
    second = b.head_split_parts
    assert second == b.suggest_head_split(16) and second != first and second[0] == 1
    one = _lib.BatchSolver([8, 4], states, nit, 0.04)
    one.set_slots([0, 4], nit)
    one.iterate(nit, None, seeds)
    b.iterate(nit, None, seeds)
    assert b.head_call()["on"] and b.head_call()["widest"] == second[1]
    assert_same(fields(b, 1), fields(one, 1), "auto")
    # a value by hand ends "auto"
    b.set_head_split([2, 2])
    b.set_slots([8, 8], nit)
    assert b.head_split_parts == [2, 2]
    b.close()
    one.close()


# ---- end to end
@functools.lru_cache(maxsize=None)
def sweep_states():
    return tuple([journal_graph(c, 75e-4, 0) for c in (5, 6, 7)] + [journal_graph(7, 75e-4, 1)])


SEARCH_KW = dict(nit=20, eta=0.04, seed=7, epilogue="batch")


@functools.lru_cache(maxsize=None)
def search_without():
    return batch.search_many(list(sweep_states()), **SEARCH_KW)


@pytest.mark.parametrize("beside", [dict(), dict(split=2, row_split=2)])
def test_search_many_under_the_head_split(beside):
    got = batch.search_many(list(sweep_states()), head_split=2, **beside, **SEARCH_KW)
    for i, (g, w) in enumerate(zip(got, search_without())):
        assert g["probes"] == w["probes"] and g["Z"] == w["Z"] and g["remainder"] == w["remainder"], i
        assert np.array_equal(g["z_vec"], w["z_vec"]), i


def test_single_under_the_head_split():
    st = sweep_states()[2]
    w = search_without()[2]
    one = batch.single(st, index=2, split=2, row_split=2, head_split=2, **SEARCH_KW)
    bs = binary_search_relaxation()
    bs.verbose = False
    bs.feasibility_check_alg = one
    z_vec, Z, rem = bs.run(st)
    assert one._b.head_call()["on"] and one._b.split_call()["path"] == 2
    assert list(one.probes) == w["probes"] and Z == w["Z"] and rem == w["remainder"] and np.array_equal(z_vec, w["z_vec"])
    one.close()
