"""The split mode of the batched solver (`BatchSolver.set_split`, csrc/kernels_batch_split.h): an iteration as three launches with
several workgroups per instance must give, bit for bit, what the single-launch kernel `k_mmw_batch` gives.

The cases, their states, slot counts, step sizes and exponential settings are those of the same names in
tests/test_hip_batch_shapes.py (imported from there); `parts` and what a case reaches under the split:

  case                  K, D      parts  what it reaches
  tiny                  2, 4      4      one slice; entry parts beyond nnzL are empty
  odd_d                 75, 3     2      D < 8
  d_gt_k                5, 80     16     ten slices of 8; D > K
  ng8                   243, 64   3      24 + 24 + 16
  ng3_substeps (eta 5)  300, 170  7      six slices of 32, the last with 10 columns; at least 2 substeps
  ng1_group2            675, 257  16     odd D, eleven slices, sketch group 2
  substeps_order        300, 24   2      64 substeps of order 2; 16 + 8
  fallback              300, 24   2      4 096 substeps of order 1; 16 + 8

The mixed batch has one rank_radio and one (max_order, tol) for all its instances, as every batch has: there the cases run with
rank_radio 1 and Z = D (the shapes are the cases', as in test_all_case_shapes_in_one_launch_are_bitwise_alone) at max_order 16,
tol 1e-13, so substeps_order and fallback are there two instances of the (300, 24) shape under different seeds; their own degree
caps are covered case by case.
"""
import functools

import numpy as np
import pytest

import test_hip_batch_shapes as shapes
from conftest import relerr
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib, batch
from sig_sdp_mmw_amd.graphs import journal_graph

pytestmark = pytest.mark.gpu

FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_SKETCH,
          _lib.F_EXPM_INFO)
# name: (parts, iterations, (W, G) of the column slices)
SPLIT = {"tiny": (4, 5, (8, 1)), "odd_d": (2, 5, (8, 1)), "d_gt_k": (16, 5, (8, 10)), "ng8": (3, 5, (24, 3)),
         "ng3_substeps": (7, 4, (32, 6)), "ng1_group2": (16, 4, (24, 11)), "substeps_order": (2, 3, (16, 2)), "fallback": (2, 3, (16, 2))}
CASE = {c[0]: c for c in shapes.CASES}
NAMES = list(SPLIT)


def fields(b, i):
    return {f: b.read(i, f) for f in FIELDS}


def assert_same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, "field", f)


def calls_of(nit):
    """nit iterations as calls of uneven length"""
    return [1, nit - 2, 1] if nit >= 4 else [1, nit - 1]


@pytest.mark.parametrize("name", NAMES)
def test_split_is_bitwise_the_single_launch(name):
    case = CASE[name]
    parts, nit, slices = SPLIT[name]
    tol, seed = case[7], shapes.seed_of(case)
    assert _lib.BatchSolver.split_slices(case[9][1], parts) == slices
    one = shapes.new_batch(case, nit, tol)
    one.iterate(nit, None, [seed])
    want = fields(one, 0)
    one.close()
    b = shapes.new_batch(case, nit, tol)
    b.set_split(parts)
    assert b.split_parts == [parts]
    for n in calls_of(nit):
        b.iterate(n, None, [seed])
    assert b.iterations_done(0) == nit
    got = fields(b, 0)
    nnz = b.sizes[0]["nnzL"]
    b.close()
    assert_same(got, want, name)
    info = got[_lib.F_EXPM_INFO]
    print("[batch-split] %-16s K %3d D %3d parts %2d slices %s  plan (%d, %d)" % (name, case[9][0], case[9][1], parts, slices, int(info[2]), int(info[1])))
    if name == "tiny":
        assert nnz < 2 * parts  # entry ranges of one entry or none
    if name == "ng3_substeps":
        assert info[2] >= 2
    if name == "substeps_order":  # (64 substeps at the third iteration, as in test_hip_batch_shapes.py; rho grows with every iteration)
        assert int(info[2]) == 64 and int(info[1]) == 2
    if name == "fallback":
        assert int(info[2]) == shapes.NSUB_MAX and int(info[1]) == 1


def test_empty_entry_ranges():
    """tiny at parts 8: nnzL = 4 entries in 8 ranges, every second one empty, range 0 (which owns EXPM_INFO) among them."""
    case, parts, nit = CASE["tiny"], 8, 4
    seed = [shapes.seed_of(case)]
    one = shapes.new_batch(case, nit, case[7])
    assert one.sizes[0]["nnzL"] * 0 // parts == one.sizes[0]["nnzL"] * 1 // parts
    one.iterate(nit, None, seed)
    b = shapes.new_batch(case, nit, case[7])
    b.set_split(parts)
    b.iterate(1, None, seed)
    b.iterate(nit - 1, None, seed)
    assert_same(fields(b, 0), fields(one, 0), "tiny, parts 8")
    b.close()
    one.close()


# ---- the mixed batch
def mixed_instances():
    """(state name, D, eta, parts, nit, seed): the eight cases with their parts, then ng8 and d_gt_k again unsplit."""
    out = []
    for i, name in enumerate(NAMES + ["ng8", "d_gt_k"]):
        c = CASE[name]
        out.append((c[1], c[9][1], c[4], SPLIT[name][0] if i < len(NAMES) else 1, 3 if i % 2 else 6, 700 + i))
    return out


@functools.lru_cache(maxsize=None)
def solo_unsplit(st, D, eta, nit, seed):
    one = _lib.BatchSolver([D], [shapes.state(st)], nit, eta, rank_radio=1)
    one.set_expm(16, 1e-13)
    one.iterate(nit, None, [seed])
    out = fields(one, 0)
    one.close()
    return out


def test_mixed_batch_every_instance_is_bitwise_its_unsplit_solo_run():
    insts = mixed_instances()
    seeds = np.array([s for *_, s in insts], dtype=np.uint64)
    big = _lib.BatchSolver([D for _, D, *_ in insts], [shapes.state(n) for n, *_ in insts], [nit for *_, nit, _ in insts], 0.04, rank_radio=1)
    big.set_eta([eta for _, _, eta, *_ in insts])
    big.set_expm(16, 1e-13)
    big.set_split([p for _, _, _, p, _, _ in insts])
    big.iterate(2, None, seeds)
    big.iterate(4, None, seeds)
    for i, (st, D, eta, parts, nit, seed) in enumerate(insts):
        assert big.iterations_done(i) == nit
        assert_same(fields(big, i), solo_unsplit(st, D, eta, nit, seed), (i, st, D, parts))
    big.close()


def test_uploaded_sketches_under_the_split():
    """Parity mode in a batch of two (d_gt_k at 16 parts and 6 iterations, then ng8 at 3 parts and 3 iterations, so the second
    instance's blocks start past the first's and the two run different counts per call): the split copies each slice's columns of
    the uploaded blocks; with the device's own blocks uploaded every instance is bitwise its device-sketch solo run."""
    mixed = mixed_instances()
    insts = [[x for x in mixed if x[1] == 80][0], [x for x in mixed if x[1] == 64][0]]
    assert [x[3] for x in insts] == [16, 3] and [x[4] for x in insts] == [6, 3]
    b = _lib.BatchSolver([x[1] for x in insts], [shapes.state(x[0]) for x in insts], [x[4] for x in insts], 0.04, rank_radio=1)
    b.set_eta([x[2] for x in insts])
    b.set_expm(16, 1e-13)
    b.set_split([x[3] for x in insts])
    sk = [np.stack([b.sketch(i, x[5], it) for it in range(x[4])]) for i, x in enumerate(insts)]
    b.iterate(2, [sk[0][:2], sk[1][:2]])
    b.iterate(4, [sk[0][2:], sk[1][2:]])
    for i, (st, D, eta, parts, nit, seed) in enumerate(insts):
        assert b.iterations_done(i) == nit
        assert_same(fields(b, i), solo_unsplit(st, D, eta, nit, seed), ("randv", i))
    b.close()


# ---- the gap
@pytest.mark.parametrize("name,st,Z,rr,eta,parts", [("ng8", "j9", 32, 2, 0.04, 3), ("er300", "er300", 12, 2, 0.04, 2)])
def test_gap_under_the_split(name, st, Z, rr, eta, parts):
    nit, seed = 10, [41]

    def run(split, gap):
        b = _lib.BatchSolver([Z], [shapes.state(st)], nit, eta, rank_radio=rr)
        if gap:
            b.set_gap(True)
        if split:
            b.set_split(parts)
            b.iterate(3, None, seed)
            b.iterate(nit - 3, None, seed)
        else:
            b.iterate(nit, None, seed)
        out = fields(b, 0), (b.gap_log(0) if gap else None)
        b.close()
        return out
    f_split_gap, (rows_s, steps_s) = run(True, True)
    f_one_gap, (rows_1, steps_1) = run(False, True)
    f_split, _ = run(True, False)
    assert np.all(np.isfinite(rows_s)) and np.all(steps_s != 0)
    assert np.array_equal(rows_s, rows_1) and np.array_equal(steps_s, steps_1), name
    assert_same(f_split_gap, f_split, name + ": gap on / off under the split")
    assert_same(f_split_gap, f_one_gap, name + ": split on / off with the gap")


# ---- the oracle
def test_split_instance_follows_the_oracle():
    st = journal_graph(9, 75e-4, 0)
    Z, nit, eta, seed = 16, 30, 0.04, 12
    b = _lib.BatchSolver([Z], [st], nit, eta)
    b.set_expm(16, 1e-13)
    b.set_split(4)
    o = orc.MMWOracle(nit=nit, eta=eta)
    o.run(Z, st, lambda it, K, D: b.sketch(0, seed, it), keep_trace=[nit - 1], factor=False)
    for n in (7, 23):
        b.iterate(n, None, [seed])
    end = {k: b.read(0, w) for k, w in (("e_this", _lib.F_E_THIS), ("e_accu", _lib.F_E_ACCU), ("Y", _lib.F_Y), ("lval", _lib.F_LVAL),
                                         ("xval", _lib.F_XVAL), ("X_half", _lib.F_XHALF))}
    end["xsum"] = b.read(0, _lib.F_XAVG) + end["xval"]
    end["ysum"] = b.read(0, _lib.F_YAVG) + end["Y"]
    b.close()
    for k in ("e_this", "e_accu", "Y", "lval", "xval", "X_half", "xsum", "ysum"):
        e = relerr(end[k], o.trace[k][0])
        print("[batch-split] oracle %-7s %.2e" % (k, e))
        assert e < 1e-9, (k, e)


# ---- end to end
def search_states():
    return [journal_graph(c, 75e-4, 0) for c in (5, 6, 7, 8, 9)] + [journal_graph(9, 75e-4, 1)]


SEARCH_KW = dict(nit=30, eta=0.04, seed=7)


@functools.lru_cache(maxsize=None)
def search_unsplit(epilogue):
    return batch.search_many(search_states(), epilogue=epilogue, **SEARCH_KW)


@pytest.mark.parametrize("epilogue,split", [("handle", "auto"), ("batch", "auto"), ("batch", 4)])
def test_search_many_under_the_split(epilogue, split):
    """"auto" is the shipped rule, whatever it gives these sizes; 4 splits every instance of every round."""
    want = search_unsplit(epilogue)
    got = batch.search_many(search_states(), epilogue=epilogue, split=split, **SEARCH_KW)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["probes"] == w["probes"] and g["Z"] == w["Z"] and g["remainder"] == w["remainder"], i
        assert np.array_equal(g["z_vec"], w["z_vec"]), i


# ---- refusals
def test_refusals_and_what_the_setting_survives():
    case = CASE["ng8"]
    nit, seed = 3, [shapes.seed_of(case)]
    one = shapes.new_batch(case, nit, 1e-13)
    one.iterate(nit, None, seed)
    want = fields(one, 0)
    b = shapes.new_batch(case, nit, 1e-13)
    b.set_split(3)
    for bad in (0, _lib.BATCH_MAX_PARTS + 1):
        with pytest.raises(_lib.MMWError, match="instance 0"):
            b.set_split(bad)
        assert b.split_parts == [3]
    b.iterate(nit, None, seed)
    assert_same(fields(b, 0), want, "after the refusals")
    # all ones: the single-launch kernel
    b.reset(nit)
    b.set_split([1])
    assert b.split_parts is None
    b.iterate(nit, None, seed)
    assert_same(fields(b, 0), want, "all ones")
    # the setting survives set_slots (and the slices follow the new D: 16 + 16 + 8 of 40 columns)
    b.set_split(3)
    Z2 = 20
    b.set_slots([Z2], nit)
    one.set_slots([Z2], nit)
    assert b.split_parts == [3] and b.sizes[0]["D"] == 40
    b.iterate(nit, None, seed)
    one.iterate(nit, None, seed)
    assert_same(fields(b, 0), fields(one, 0), "after set_slots")
    b.close()
    one.close()
