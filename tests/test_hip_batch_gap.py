"""GPU checks of the duality-gap phase of the batched solver (`k_mmw_batch<true>`, csrc/kernels_batch.h): the LOG_GAP branch of the
reference (mmw.py:79-117) logged inside the batch launch, one row {e_max, K lambda_min(L(Ybar)), their difference, Lanczos steps} per
iteration, against the reference's golden vectors, the CPU oracle and the per-handle `mmw_gap`.

Bars (the ones tests/test_hip_epilogue.py holds the handle's gap to): column 0 `1e-8 |ref| + 1e-12`, column 1 `1e-6 |ref| + 1e-9`,
column 2 `1e-6 (|ref0| + |ref1|) + 1e-9`.
"""
import functools

import numpy as np
import pytest
import scipy.sparse

from conftest import load_golden, state_from
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

pytestmark = pytest.mark.gpu

FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_SKETCH,
          _lib.F_EXPM_INFO)


def fields(b, i):
    return [b.read(i, f) for f in FIELDS]


def deviations(rows, ref):
    """Per column: |got - ref| and the bar, both [n, 3]."""
    rows, ref = np.asarray(rows), np.asarray(ref)
    bar = np.stack([1e-8 * np.abs(ref[:, 0]) + 1e-12, 1e-6 * np.abs(ref[:, 1]) + 1e-9,
                    1e-6 * (np.abs(ref[:, 0]) + np.abs(ref[:, 1])) + 1e-9], axis=1)
    return np.abs(rows - ref), bar


def assert_rows(rows, ref, what):
    assert np.shape(rows) == np.shape(ref), (what, np.shape(rows), np.shape(ref))
    dev, bar = deviations(rows, ref)
    print("[batch-gap] %-28s rows %4d  worst deviation per column %s (worst bar ratio %s)"
          % (what, len(ref), np.array2string(dev.max(axis=0), precision=2), np.array2string((dev / bar).max(axis=0), precision=2)))
    bad = np.argwhere(~(dev <= bar))
    assert bad.size == 0, (what, bad[:5].tolist(), [(rows[i][j], ref[i][j]) for i, j in bad[:5]])


def oracle_gap(b, i, state, Z, seed, nit, eta, rank_radio=2):
    """The oracle's LOG_GAP rows on the sketches the batch's device generator draws for instance i."""
    o = orc.MMWOracle(nit=nit, eta=eta, rank_radio=rank_radio, log_gap=True)
    o.run(Z, state, lambda it, K, D: b.sketch(i, seed, it), factor=False)
    return np.array(o.trace["gap"])


# ---- 1
def test_reference_goldens_as_one_batch():
    names = ("env75", "env192", "dense60")
    gs = [load_golden("run_" + n) for n in names]
    nits = [int(g["nit"]) for g in gs]
    b = _lib.BatchSolver([int(g["Z"]) for g in gs], [state_from(g) for g in gs], nits, 0.1)
    b.set_eta([float(g["eta"]) for g in gs])
    b.set_expm(16, 1e-13)
    b.set_gap(True)
    b.iterate(max(nits), [g["randv"][:n] for g, n in zip(gs, nits)])
    for i, (name, g) in enumerate(zip(names, gs)):
        rows, steps = b.gap_log(i)
        assert_rows(rows, g["gap"][:nits[i]], "golden " + name)
        assert steps.shape == (nits[i],) and np.all(steps > 0), (name, steps)
    b.close()


# ---- 2
SWEEP = [("cell5", lambda: journal_graph(5, 75e-4, 0), 27), ("cell10", lambda: journal_graph(10, 75e-4, 0), 36),
         ("cell15", lambda: journal_graph(15, 75e-4, 0), 45), ("cell10-125", lambda: journal_graph(10, 125e-4, 0), 63),
         ("er240", lambda: er_contention_graph(240, 0.04, 3), 14)]
SWEEP_CALLS = (1, 36, 13, 50, 20)  # 120 iterations in calls of uneven length


@functools.lru_cache(maxsize=None)
def sweep_oracle():
    """The oracle's rows for the five sweep instances over 120 iterations (eta 0.04), on the device generator's sketches."""
    states = [mk() for _, mk, _ in SWEEP]
    Zs = [Z for _, _, Z in SWEEP]
    seeds = np.array([41, 42, 43, 44, 45], dtype=np.uint64)
    nit, eta = sum(SWEEP_CALLS), 0.04
    b = _lib.BatchSolver(Zs, states, nit, eta)
    refs = [oracle_gap(b, i, states[i], Zs[i], int(seeds[i]), nit, eta) for i in range(len(states))]
    b.close()
    return states, Zs, seeds, nit, eta, refs


def run_sweep(tol):
    states, Zs, seeds, nit, eta, refs = sweep_oracle()
    b = _lib.BatchSolver(Zs, states, nit, eta)
    if tol is not None:
        b.set_expm(16, tol)
    b.set_gap(True)
    for n in SWEEP_CALLS:
        b.iterate(n, None, seeds)
    logs = [b.gap_log(i) for i in range(len(states))]
    b.close()
    return logs, refs


@pytest.mark.timeout(600)
def test_oracle_on_device_sketches_at_sweep_sizes():
    logs, refs = run_sweep(1e-12)
    for (name, _, _), (rows, steps), ref in zip(SWEEP, logs, refs):
        print("[batch-gap] %-10s Lanczos steps min %d mean %.1f max %d" % (name, steps.min(), steps.mean(), steps.max()))
        # the condition: every row converged, under the default cap
        assert np.all(steps > 0) and np.all(steps <= 600), (name, steps.min(), steps.max())
        assert_rows(rows, ref, "sweep " + name)


@pytest.mark.timeout(600)
def test_sweep_at_the_default_expm_tolerance_converges_every_row():
    """Default expm tolerance (1e-9; the iterate then follows the oracle to ~1e-5): only the condition on `steps` is asserted, the
    deviation from the oracle is printed (DESIGN §12 quotes it)."""
    logs, refs = run_sweep(None)
    for (name, _, _), (rows, steps), ref in zip(SWEEP, logs, refs):
        dev = np.abs(rows - ref)
        print("[batch-gap] default tol %-10s worst deviation per column %s, relative %s; steps mean %.1f max %d"
              % (name, np.array2string(dev.max(axis=0), precision=2),
                 np.array2string((dev / np.maximum(np.abs(ref), 1e-300)).max(axis=0), precision=2), steps.mean(), steps.max()))
        assert np.all(steps > 0) and np.all(steps <= 600), (name, steps.min(), steps.max())
        assert np.all(np.isfinite(rows)), name


# ---- 3
def small_mix():
    states = [journal_graph(5, 75e-4, 0), journal_graph(10, 75e-4, 0), er_contention_graph(200, 0.05, 1), journal_graph(7, 75e-4, 2)]
    return states, [12, 36, 10, 14], np.array([61, 62, 63, 64], dtype=np.uint64)


def test_the_gap_phase_only_reads_the_iterate():
    states, Zs, seeds = small_mix()
    nit, eta = 50, 0.04
    on = _lib.BatchSolver(Zs, states, nit, eta)
    off = _lib.BatchSolver(Zs, states, nit, eta)
    on.set_gap(True)
    done = 0
    for upto in (1, 13, 50):
        on.iterate(upto - done, None, seeds)
        off.iterate(upto - done, None, seeds)
        done = upto
        for i in range(len(states)):
            for f, a, r in zip(FIELDS, fields(on, i), fields(off, i)):
                assert np.array_equal(a, r), (upto, i, f)
    for i in range(len(states)):
        rows, steps = on.gap_log(i)
        assert rows.shape == (nit, 3) and np.all(np.isfinite(rows)) and np.all(steps > 0), i
    with pytest.raises(_lib.MMWError):
        off.gap_log(0)  # never enabled
    on.close()
    off.close()


# ---- 4
def full_log(b, i):
    rows, steps = b.gap_log(i)
    return np.column_stack([rows, steps.astype(np.float64)])


def test_gap_rows_are_bitwise_independent_of_neighbours_and_call_splits():
    pool = [journal_graph(c, 75e-4, s) for c in (5, 7, 9, 11, 13, 15) for s in (0, 1)] + [er_contention_graph(200, 0.05, s) for s in range(2)]
    rng = np.random.default_rng(9)
    states = [pool[k] for k in rng.integers(0, len(pool), 64)]
    Zs = [int(z) for z in rng.integers(6, 24, 64)]
    seeds = np.arange(2000, 2064, dtype=np.uint64)
    nit, eta, probe = 30, 0.04, 11
    big = _lib.BatchSolver(Zs, states, nit, eta)
    big.set_gap(True)
    big.iterate(nit, None, seeds)
    logs = []
    for calls in ((1,) * 30, (7, 23), (30,)):
        one = _lib.BatchSolver([Zs[probe]], [states[probe]], nit, eta)
        one.set_gap(True)
        for n in calls:
            one.iterate(n, None, seeds[probe:probe + 1])
        logs.append(full_log(one, 0))
        if calls == (30,):
            for f, a, r in zip(FIELDS, fields(one, 0), fields(big, probe)):
                assert np.array_equal(a, r), f
        one.close()
    ref = full_log(big, probe)
    assert ref.shape == (nit, 4) and np.all(np.isfinite(ref))
    for lg in logs:
        assert np.array_equal(lg, ref)
    big.close()


# ---- 5
def test_row_against_the_handles_gap_on_an_exported_iterate():
    """The set-up of test_export_before_the_last_iteration_continues_like_the_handle: after 12 of 30 iterations the exported handle's
    sums hold 13 terms, which is what the batch's row 12 is made from when its iteration 12 starts."""
    gs = load_golden("run_env192")
    state = state_from(gs)
    Z, eta, nit, cut = 12, 0.05, 30, 12
    K = state[0].shape[0]
    rng = np.random.default_rng(8)
    sk = np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * Z))) for _ in range(nit)])
    b = _lib.BatchSolver([Z], [state], nit, eta)
    b.set_expm(16, 1e-13)
    b.set_gap(True)
    b.iterate(cut, [sk[:cut]])
    h = _lib.Solver(Z, state, nit, eta, dtype=_lib.F64)
    h.set_expm(_lib.EXPM_TAYLOR, 16, 1e-13)
    b.export(0, h)
    gh = np.asarray(h.gap())
    b.iterate(1, [sk[cut:cut + 1]])
    rows, steps = b.gap_log(0)
    assert rows.shape == (cut + 1, 3) and steps[cut] > 0
    assert np.allclose(rows[cut], gh, rtol=1e-8, atol=1e-10), (rows[cut], gh)
    b.close()
    h.close()


# ---- 6
@functools.lru_cache(maxsize=None)
def state(name):
    """The graphs of tests/test_hip_batch_shapes.py's cases, restated."""
    if name == "er2":
        return er_contention_graph(2, 1.0, 1)
    if name == "er5":
        return er_contention_graph(5, 0.5, 1)
    if name == "degen":  # the empty association relation, user 5 with only its diagonal entry
        S, _, h = er_contention_graph(30, 0.2, seed=3)
        S = S.tolil()
        S[5, :] = 0
        S[:, 5] = 0
        S[5, 5] = 3.7
        S = S.tocsr()
        S.eliminate_zeros()
        return S, scipy.sparse.csr_matrix((30, 30)), h
    if name == "j9":
        return journal_graph(9, 75e-4, 0)
    if name == "er1000":
        return er_contention_graph(1000, 0.01, 4)
    if name == "er4096":
        return er_contention_graph(4096, 0.002, 2)
    raise KeyError(name)


# (graph, Z = D with the batch's one rank_radio 1, eta, iterations): the (K, D) shapes of that file's cases tiny, d_gt_k,
# degenerate_z2, ng8, odd_group3 and limits
SHAPES = [("er2", 2, 0.04, 2), ("er5", 80, 0.04, 2), ("degen", 4, 0.1, 2), ("j9", 64, 0.04, 2), ("er1000", 511, 0.4, 2),
          ("er4096", 512, 0.4, 1)]


@pytest.mark.timeout(600)
def test_shapes_in_one_launch_against_the_oracle():
    states = [state(n) for n, _, _, _ in SHAPES]
    Zs = [Z for _, Z, _, _ in SHAPES]
    nits = [n for _, _, _, n in SHAPES]
    seeds = np.arange(700, 700 + len(SHAPES), dtype=np.uint64)
    b = _lib.BatchSolver(Zs, states, nits, 0.04, rank_radio=1)
    assert [(b.sizes[i]["K"], b.sizes[i]["D"]) for i in range(len(SHAPES))] == [(2, 2), (5, 80), (30, 4), (243, 64), (1000, 511), (4096, 512)]
    assert b.sizes[2]["E_asso"] == 0
    b.set_eta([e for _, _, e, _ in SHAPES])
    b.set_expm(16, 1e-13)
    b.set_gap(True)
    b.iterate(2, None, seeds)  # one launch
    for i, (name, Z, eta, nit) in enumerate(SHAPES):
        assert b.iterations_done(i) == nit
        rows, steps = b.gap_log(i)
        K = b.sizes[i]["K"]
        print("[batch-gap] shape %-7s K %4d steps %s rows %s" % (name, K, steps.tolist(), np.array2string(rows, precision=6)))
        assert np.all(steps > 0) and np.all(steps <= min(K, 600)), (name, steps)  # an exhausted Krylov space is convergence
        assert_rows(rows, oracle_gap(b, i, states[i], Z, int(seeds[i]), nit, eta, rank_radio=1), "shape " + name)
    b.close()


# ---- 7
def test_cap_flags_nan_rows_and_reset():
    st, Z, seed, eta, nit = journal_graph(10, 75e-4, 0), 36, np.array([77], dtype=np.uint64), 0.04, 20
    b = _lib.BatchSolver([Z], [st], nit, eta)
    b.set_expm(16, 1e-12)
    off = _lib.BatchSolver([Z], [st], nit, eta)
    off.set_expm(16, 1e-12)
    assert b.sizes[0]["K"] == 300
    b.iterate(3, None, seed)  # before set_gap: these rows stay NaN
    b.set_gap(True, m_cap=5)
    b.iterate(nit - 3, None, seed)
    off.iterate(nit, None, seed)
    rows, steps = b.gap_log(0)
    assert rows.shape == (nit, 3)
    assert np.all(np.isnan(rows[:3])) and np.all(steps[:3] == 0)
    assert np.all(steps[3:] == -5), steps
    ref = oracle_gap(b, 0, st, Z, int(seed[0]), nit, eta)
    # a Ritz value is an upper bound of lambda_min (eigsh is within 1e-14 of the dense value on these inputs; 1e-12 leaves it room)
    assert np.all(rows[3:, 1] >= ref[3:, 1] - 1e-12 * np.abs(ref[3:, 1])), (rows[3:, 1], ref[3:, 1])
    assert np.all(np.abs(rows[3:, 0] - ref[3:, 0]) <= 1e-8 * np.abs(ref[3:, 0]) + 1e-12)  # e_max does not depend on the cap
    assert np.allclose(rows[3:, 2], rows[3:, 0] - rows[3:, 1], rtol=0, atol=1e-12)
    for f, a, r in zip(FIELDS, fields(b, 0), fields(off, 0)):
        assert np.array_equal(a, r), f
    # reset: an empty log, the setting kept
    b.reset(4)
    rows, steps = b.gap_log(0)
    assert rows.shape == (0, 3) and steps.shape == (0,)
    b.iterate(2, None, seed)
    rows, steps = b.gap_log(0)
    assert rows.shape == (2, 3) and np.all(steps == -5) and np.all(np.isfinite(rows))
    # the default cap again; set_slots clears the log too
    b.set_gap(True)
    b.set_slots([30], 3)
    assert b.gap_log(0)[0].shape == (0, 3)
    b.iterate(3, None, seed)
    rows, steps = b.gap_log(0)
    assert rows.shape == (3, 3) and np.all(steps > 0)
    # off again: rows of the iterations that follow are NaN
    b.reset(4)
    b.iterate(1, None, seed)
    b.set_gap(False)
    b.iterate(1, None, seed)
    rows, steps = b.gap_log(0)
    assert np.all(np.isfinite(rows[0])) and np.all(np.isnan(rows[1])) and steps[1] == 0
    with pytest.raises(_lib.MMWError):
        b.set_gap(True, m_cap=5000)
    b.close()
    off.close()


# ---- 8
def test_convergence_many_with_per_instance_nit_and_eta():
    from sig_sdp_mmw_amd import batch
    states = [journal_graph(5, 75e-4, 1), journal_graph(8, 75e-4, 1), er_contention_graph(150, 0.05, 2)]
    Zs, nits, etas = [10, 20, 9], (100, 40, 60), (0.1, 0.04, 0.05)
    seeds = np.array([5, 6, 7], dtype=np.uint64)
    out = batch.convergence_many(Zs, states, nits, etas, seeds=seeds)
    assert len(out) == 3
    b = _lib.BatchSolver(Zs, states, list(nits), etas[0])
    b.set_eta(etas)
    b.set_gap(True)
    for n in (30, 70):
        b.iterate(n, None, seeds)
    for i in range(3):
        rows, steps = b.gap_log(i)
        assert out[i]["gap"].shape == (nits[i], 3) and out[i]["lanczos_steps"].shape == (nits[i],)
        assert np.array_equal(out[i]["gap"], rows) and np.array_equal(out[i]["lanczos_steps"], steps), i
        assert np.all(steps > 0)
    b.close()
    # scalars for all instances
    out2 = batch.convergence_many(Zs[:2], states[:2], 5, 0.04)
    assert [o["gap"].shape for o in out2] == [(5, 3), (5, 3)]
