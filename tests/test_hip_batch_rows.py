"""The row split of the batched solver (`BatchSolver.set_row_split`, csrc/kernels_batch_rows.h): an iteration as head, plan, one
launch per Taylor term with one workgroup per (instance, column slice, row part), and x must give, bit for bit, what the single-launch
kernel `k_mmw_batch` gives.

The cases, their states, slot counts, step sizes and exponential settings are those of the same names in
tests/test_hip_batch_shapes.py (imported from there); (rows, column parts) and what a case reaches under the row split:

  case                  K, D       rows, parts  what it reaches
  tiny                  2, 4       3, 1         a row range is empty
  d_gt_k                5, 80      7, 16        more parts than rows, ten slices
  odd_d                 75, 3      4, 1         D < 8, rows not dividing K
  ng8                   243, 64    3, 3         slices x row parts
  ng3_substeps (eta 5)  300, 170   5, 7         narrow last slice, at least 2 substeps
  ng1_group2            675, 257   11, 16       odd D
  substeps_order        300, 24    4, 2         64 substeps of order 2
  fallback              300, 24    2, 1         4 096 substeps of order 1, one iteration only
  limits                4096, 512  64, 32       the K, D and row-part limits, one iteration

A dense row: L's pattern is symmetric with a full diagonal, so a row of n entries faces n - 1 rows of at least two and no row holds
more than half of nnzL; the densest a row gets is the hub of a star graph, built here at K = 65 (65 of 193 entries).  At 16 row
parts the hub's part stands alone and the four parts that would start inside the hub's row are empty.

The mixed batch has one rank_radio and one (max_order, tol) for all its instances, as every batch has: there the cases run with
rank_radio 1 and Z = D at max_order 16, tol 1e-13 (as in tests/test_hip_batch_split.py), so substeps_order and fallback are there the
(300, 24) shape at eta 0.04 and eta 5: schedules of different length share the launches.

Mutations of csrc/kernels_batch_rows.h and csrc/batch_rows.h, tried by hand once; each turned tests of this file red (the case
tests, the star graph and the mixed batch were run against each):
  * no fold over the row parts (a term folds `prev_t` / `prev_f` of its own part only): ng3_substeps, the star, the mixed batch;
  * c_on not carried from term to term (`on = 1` instead of the stored state): ng3_substeps, the star, the mixed batch;
  * T0 / T1 not alternated at a substep boundary (the start of a substep writes W1 whatever the term count, so after a substep
    with an odd number of terms the first term reads the stale buffer): fallback, ng3_substeps, the star, the mixed batch;
  * row range boundaries off by one (a part's first row taken one row late in the work table): every case.
"""
import functools

import numpy as np
import pytest
import scipy.sparse

import test_hip_batch_shapes as shapes
from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.graphs import journal_graph

pytestmark = pytest.mark.gpu

FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_SKETCH,
          _lib.F_EXPM_INFO)
# name: (rows, column parts, iterations)
ROWS = {"tiny": (3, 1, 5), "d_gt_k": (7, 16, 5), "odd_d": (4, 1, 5), "ng8": (3, 3, 5), "ng3_substeps": (5, 7, 4),
        "ng1_group2": (11, 16, 4), "substeps_order": (4, 2, 3), "fallback": (2, 1, 1), "limits": (64, 32, 1)}
CASE = {c[0]: c for c in shapes.CASES}
NAMES = list(ROWS)


def fields(b, i):
    return {f: b.read(i, f) for f in FIELDS}


def assert_same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, "field", f)


def calls_of(nit):
    """nit iterations as calls of uneven length"""
    return [1, nit - 2, 1] if nit >= 4 else ([1, nit - 1] if nit >= 2 else [1])


def set_both(b, rows, parts):
    b.set_split(parts)
    b.set_row_split(rows)


@functools.lru_cache(maxsize=None)
def case_single_launch(name):
    case = CASE[name]
    nit = ROWS[name][2]
    one = shapes.new_batch(case, nit, case[7])
    one.iterate(nit, None, [shapes.seed_of(case)])
    out = fields(one, 0)
    one.close()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_row_split_is_bitwise_the_single_launch(name):
    case = CASE[name]
    rows, parts, nit = ROWS[name]
    seed = shapes.seed_of(case)
    want = case_single_launch(name)
    b = shapes.new_batch(case, nit, case[7])
    set_both(b, rows, parts)
    assert b.row_split_parts == [rows] and b.split_parts == ([parts] if parts > 1 else None)
    for n in calls_of(nit):
        b.iterate(n, None, [seed])
        assert b.split_call()["path"] == 2
    assert b.iterations_done(0) == nit
    got = fields(b, 0)
    bd = b.row_ranges(0, rows)
    K = b.sizes[0]["K"]
    b.close()
    info = got[_lib.F_EXPM_INFO]
    print("[batch-rows] %-16s K %4d D %3d rows %2d parts %2d  plan (%d, %d)  ranges %s" % (name, K, case[9][1], rows, parts, int(info[2]), int(info[1]), bd[:8]))
    assert_same(got, want, name)
    assert bd[0] == 0 and bd[-1] == K and len(bd) == rows + 1
    if name in ("tiny", "d_gt_k"):
        assert any(a == b_ for a, b_ in zip(bd, bd[1:]))  # K < rows: a row range is empty
    if name == "odd_d":
        assert K % rows != 0
    if name == "ng3_substeps":
        assert info[2] >= 2
    if name == "substeps_order":
        assert int(info[2]) == 64 and int(info[1]) == 2
    if name == "fallback":
        assert int(info[2]) == shapes.NSUB_MAX and int(info[1]) == 1


# ---- a dense row
@functools.lru_cache(maxsize=None)
def star_state(K=65):
    """Hub 0 and K - 1 leaves: S has the hub's row and column (directed gains) and the diagonal, Q is empty."""
    rng = np.random.default_rng(5)
    leaves = np.arange(1, K)
    r = np.concatenate([np.zeros(K - 1, dtype=np.int64), leaves, np.arange(K)])
    c = np.concatenate([leaves, np.zeros(K - 1, dtype=np.int64), np.arange(K)])
    v = np.concatenate([rng.uniform(0.1, 3.7, 2 * (K - 1)), np.full(K, 3.7)])
    S = scipy.sparse.csr_matrix((v, (r, c)), shape=(K, K))
    S.sort_indices()
    return S, scipy.sparse.csr_matrix((K, K)), np.ones(K)


def test_a_dense_row_leaves_row_parts_empty():
    Z, nit, eta, seed, rows = 4, 4, 0.3, [77], 16
    one = _lib.BatchSolver([Z], [star_state()], nit, eta)
    one.set_expm(16, 1e-13)
    indptr = one.read_i32(0, _lib.I_L_INDPTR)
    lens = np.diff(indptr)
    assert lens.max() == 65 and lens.argmax() == 0 and indptr[-1] == 193
    one.iterate(nit, None, seed)
    want = fields(one, 0)
    b = _lib.BatchSolver([Z], [star_state()], nit, eta)
    b.set_expm(16, 1e-13)
    bd = b.row_ranges(0, rows)
    assert bd == _lib.BatchSolver.row_bounds(indptr, rows)
    assert bd[:6] == [0, 1, 1, 1, 1, 1]  # the hub alone, then four empty parts
    nnz = int(indptr[-1])
    for p in range(rows):
        assert indptr[bd[p + 1]] - indptr[bd[p]] <= -(-nnz // rows) + int(lens.max())
    b.set_row_split(rows)
    for n in calls_of(nit):
        b.iterate(n, None, seed)
    assert_same(fields(b, 0), want, "star")
    b.close()
    one.close()


# ---- the mixed batch
# (case whose shape it is, eta, rows, column parts, iterations)
MIXED = [("tiny", 0.04, 3, 1, 5), ("d_gt_k", 0.04, 7, 16, 3), ("odd_d", 0.04, 4, 1, 5), ("ng8", 0.04, 3, 3, 4), ("ng3_substeps", 5.0, 5, 7, 3),
         ("ng1_group2", 0.04, 11, 16, 3), ("substeps_order", 0.04, 4, 2, 5), ("fallback", 5.0, 1, 2, 4), ("limits", 0.4, 64, 32, 1)]


def mixed_instances():
    """(state name, D, eta, rows, parts, nit, seed)"""
    return [(CASE[n][1], CASE[n][9][1], eta, rows, parts, nit, 900 + i) for i, (n, eta, rows, parts, nit) in enumerate(MIXED)]


@functools.lru_cache(maxsize=None)
def solo_single_launch(st, D, eta, nit, seed, gap):
    one = _lib.BatchSolver([D], [shapes.state(st)], nit, eta, rank_radio=1)
    one.set_expm(16, 1e-13)
    if gap:
        one.set_gap(True)
    one.iterate(nit, None, [seed])
    out = fields(one, 0), (one.gap_log(0) if gap else None)
    one.close()
    return out


def new_mixed(insts):
    big = _lib.BatchSolver([x[1] for x in insts], [shapes.state(x[0]) for x in insts], [x[5] for x in insts], 0.04, rank_radio=1)
    big.set_eta([x[2] for x in insts])
    big.set_expm(16, 1e-13)
    set_both(big, [x[3] for x in insts], [x[4] for x in insts])
    return big


@pytest.mark.parametrize("mode", ["philox", "randv", "gap"])
def test_mixed_batch_every_instance_is_bitwise_its_single_launch_solo_run(mode):
    insts = mixed_instances()
    assert any(x[3] == 1 and x[4] > 1 for x in insts) and any(x[3] > 1 and x[4] == 1 for x in insts)
    assert {0.04, 5.0} <= {x[2] for x in insts if x[0] == "er300" and x[1] == 24}
    seeds = np.array([x[6] for x in insts], dtype=np.uint64)
    big = new_mixed(insts)
    gap = mode == "gap"
    if gap:
        big.set_gap(True)
    done = [0] * len(insts)
    for n in (1, 3, 1):
        if mode == "randv":
            blocks = []
            for i, x in enumerate(insts):
                nb = max(0, min(n, x[5] - done[i]))
                blocks.append(np.stack([big.sketch(i, x[6], done[i] + k) for k in range(nb)]) if nb else None)
                done[i] += nb
            big.iterate(n, blocks)
        else:
            big.iterate(n, None, seeds)
        assert big.split_call()["path"] == 2
    for i, (st, D, eta, rows, parts, nit, seed) in enumerate(insts):
        assert big.iterations_done(i) == nit
        want, wgap = solo_single_launch(st, D, eta, nit, seed, gap)
        assert_same(fields(big, i), want, (mode, i, st, D, rows, parts))
        if gap:
            rows_g, steps_g = big.gap_log(i)
            assert np.all(np.isfinite(rows_g)) and np.array_equal(rows_g, wgap[0]) and np.array_equal(steps_g, wgap[1]), (i, st)
    if mode == "philox":
        # the largest instance is taken out (Z <= 0), the others restart with one count for all: the settings hold
        nit2 = 3
        big.set_slots([x[1] if i + 1 < len(insts) else 0 for i, x in enumerate(insts)], nit2)
        assert big.row_split_parts == [x[3] for x in insts] and big.split_parts == [x[4] for x in insts]
        big.iterate(2, None, seeds)
        big.iterate(1, None, seeds)
        assert big.split_call()["path"] == 2
        for i, (st, D, eta, rows, parts, nit, seed) in enumerate(insts[:-1]):
            assert big.iterations_done(i) == nit2
            assert_same(fields(big, i), solo_single_launch(st, D, eta, nit2, seed, False)[0], ("after set_slots", i, st))
        assert big.iterations_done(len(insts) - 1) == 0
    big.close()


# ---- the setting's lifecycle
def test_refusals_and_what_the_setting_survives():
    case = CASE["ng8"]
    nit, seed = 3, [shapes.seed_of(case)]
    one = shapes.new_batch(case, nit, 1e-13)
    one.iterate(nit, None, seed)
    want = fields(one, 0)
    assert one.split_call() == {"path": 0, "launches": 1, "idle": 0, "widest": 1}
    b = shapes.new_batch(case, nit, 1e-13)
    b.set_row_split(3)
    for bad in (0, -1, _lib.BATCH_MAX_ROW_PARTS + 1):
        with pytest.raises(_lib.MMWError, match="instance 0"):
            b.set_row_split(bad)
        assert b.row_split_parts == [3]
    b.iterate(nit, None, seed)
    assert b.split_call()["path"] == 2  # the refused values left the setting
    assert_same(fields(b, 0), want, "after the refusals")
    # all ones or None: what runs without the row split
    for off in ([1], None):
        b.reset(nit)
        b.set_row_split(off)
        assert b.row_split_parts is None
        b.iterate(nit, None, seed)
        assert b.split_call()["path"] == 0
        assert_same(fields(b, 0), want, "off")
    b.reset(nit)
    b.set_split(3)
    b.iterate(nit, None, seed)
    assert b.split_call() == {"path": 1, "launches": 3 * nit, "idle": 0, "widest": 3}
    # the setting survives reset and set_slots to another D (and the slices follow it: 16 + 16 + 8 of 40 columns)
    b.set_row_split(5)
    b.reset(nit)
    assert b.row_split_parts == [5]
    b.iterate(nit, None, seed)
    assert b.split_call()["path"] == 2 and b.split_call()["widest"] == 15
    assert_same(fields(b, 0), want, "rows 5 x parts 3 after reset")
    Z2 = 20
    b.set_slots([Z2], nit)
    one.set_slots([Z2], nit)
    assert b.row_split_parts == [5] and b.split_parts == [3] and b.sizes[0]["D"] == 40
    b.iterate(nit, None, seed)
    one.iterate(nit, None, seed)
    assert b.split_call()["path"] == 2
    assert_same(fields(b, 0), fields(one, 0), "after set_slots")
    b.close()
    one.close()


def test_auto_is_taken_again_after_set_slots():
    """Two instances of K = 243 and 675: "auto" follows the slot counts, and with them the weights w_i = nnzL_i D_i."""
    states = [journal_graph(9, 75e-4, 0), journal_graph(15, 75e-4, 0)]
    nit, seeds = 2, [5, 6]
    b = _lib.BatchSolver([8, 8], states, nit, 0.04)
    b.set_row_split("auto", cus=16)
    first = b.row_split_parts
    assert first == b.suggest_row_split(16) and max(first) > 1
    b.set_slots([64, 4], nit)
    second = b.row_split_parts
    assert second == b.suggest_row_split(16) and second != first
    one = _lib.BatchSolver([64, 4], states, nit, 0.04)
    one.iterate(nit, None, seeds)
    b.iterate(nit, None, seeds)
    assert b.split_call()["path"] == 2
    for i in range(2):
        assert_same(fields(b, i), fields(one, i), ("auto", i))
    # a value by hand ends "auto"
    b.set_row_split([2, 2])
    b.set_slots([8, 8], nit)
    assert b.row_split_parts == [2, 2]
    b.close()
    one.close()


# ---- end to end
def test_search_many_under_the_row_split():
    states = [journal_graph(c, 75e-4, 0) for c in (5, 6, 7)] + [journal_graph(7, 75e-4, 1)]
    kw = dict(nit=20, eta=0.04, seed=7, epilogue="batch")
    want = batch.search_many(states, **kw)
    got = batch.search_many(states, row_split=2, **kw)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["probes"] == w["probes"] and g["Z"] == w["Z"] and g["remainder"] == w["remainder"], i
        assert np.array_equal(g["z_vec"], w["z_vec"]), i


# ---- MMW_F_SPLIT_CALL
def test_split_call_counts_the_launches_of_the_longest_schedule():
    """Two instances of the (300, 24) shape at eta 0.04 and eta 5: per iteration head, plan, the launches of the longer schedule
    nsub (1 + mo) and x.  nsub is read back; mo, the plan's a-priori order, is replayed from the rho read back."""
    st = shapes.state("er300")
    etas, seeds, nit, tol, order = [0.04, 5.0], [11, 12], 4, 1e-13, 16

    def new():
        b = _lib.BatchSolver([24, 24], [st, st], nit, 0.04, rank_radio=1)
        b.set_eta(etas)
        b.set_expm(order, tol)
        set_both(b, [4, 2], [2, 1])
        return b
    a = new()
    per_it = []
    for it in range(nit):
        a.iterate(1, None, seeds)
        sched = []
        for i in range(2):
            info = a.read(i, _lib.F_EXPM_INFO)
            nsub, mo = shapes.plan(info[0], tol, order)
            assert nsub == int(info[2]) and 1 <= int(info[1]) <= mo
            sched.append(nsub * (1 + mo))
        per_it.append(2 + max(sched) + 1)
        call = a.split_call()
        print("[batch-rows] iteration %d schedules %s call %s" % (it, sched, call))
        assert call["path"] == 2 and call["launches"] == per_it[-1] and call["widest"] == 2 * 4 + 1 * 2
        assert 0 <= call["idle"] < max(sched)
    a.close()
    b = new()
    b.iterate(nit, None, seeds)
    assert b.split_call()["launches"] == sum(per_it)
    b.close()
