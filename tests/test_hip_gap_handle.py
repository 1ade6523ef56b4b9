"""GPU checks of the duality gap logged inside the loop of a solver handle (mmw_set_gap / mmw_read_gap, csrc/kernels_gap.h,
csrc/solver_gap.h): one row {e_max, K lambda_min(L(Ybar)), their difference, Lanczos steps} per iteration (mmw.py:79-117) at any K and
on either dtype, without leaving the chunked `iterate(n)`, against the reference's golden vectors, the CPU oracle, a float64
recomputation from the sums read back, the per-call `mmw_gap` and the batch's row.

Bars (those of tests/test_hip_epilogue.py::test_gap_matches_reference): column 0 `1e-8 |ref| + 1e-12`, column 1 `1e-6 |ref| + 1e-9`,
column 2 `1e-6 (|ref0| + |ref1|) + 1e-9`.
"""
import functools

import numpy as np
import pytest

from conftest import load_golden, state_from
from helpers import gap_cases as gc
from helpers import mfma_graphs as mg
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.convergence import convergence
from sig_sdp_mmw_amd.graphs import journal_graph_device
from sig_sdp_mmw_amd.mmw import mmw

pytestmark = pytest.mark.gpu

FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF, _lib.F_SKETCH,
          _lib.F_EXPM_INFO, _lib.F_DUAL_INFO)


def deviations(rows, ref):
    rows, ref = np.asarray(rows), np.asarray(ref)
    bar = np.stack([1e-8 * np.abs(ref[:, 0]) + 1e-12, 1e-6 * np.abs(ref[:, 1]) + 1e-9,
                    1e-6 * (np.abs(ref[:, 0]) + np.abs(ref[:, 1])) + 1e-9], axis=1)
    return np.abs(rows - ref), bar


def assert_rows(rows, ref, what, steps=None, info=None):
    assert np.shape(rows) == np.shape(ref), (what, np.shape(rows), np.shape(ref))
    dev, bar = deviations(rows, ref)
    extra = ""
    if steps is not None:
        extra += "  steps min %d mean %.1f max %d" % (np.min(steps), np.mean(steps), np.max(steps))
    if info is not None:
        extra += "  launches per row %.1f, continued %d" % (info["launches"] / max(info["rows"], 1), info["continued"])
    print("[handle-gap] %-30s rows %4d  worst deviation per column %s (worst bar ratio %s)%s"
          % (what, len(ref), np.array2string(dev.max(axis=0), precision=2), np.array2string((dev / bar).max(axis=0), precision=2), extra))
    bad = np.argwhere(~(dev <= bar))
    assert bad.size == 0, (what, bad[:5].tolist(), [(rows[i][j], ref[i][j]) for i, j in bad[:5]])


# ---- 1
@pytest.mark.parametrize("name", ["env75", "env192", "dense60"])
def test_reference_goldens_in_one_iterate(name):
    g = load_golden("run_" + name)
    Z, nit, eta = int(g["Z"]), int(g["nit"]), float(g["eta"])
    s = _lib.Solver(Z, state_from(g), nit, eta)
    s.set_expm(_lib.EXPM_LANCZOS, 16, 1e-13)
    s.set_gap()
    s.iterate(nit, g["randv"][:nit])
    rows, steps = s.gap_log()
    assert_rows(rows, g["gap"][:nit], "golden " + name, steps, s.gap_info())
    assert steps.shape == (nit,) and np.all(steps > 0), steps
    s.close()


# ---- 2
K300_Z, K300_NIT, K300_ETA, K300_SEED, K300_CALLS = 36, 40, 0.04, 77, (1, 17, 9, 13)


def k300_handle(nit=K300_NIT, tol=1e-12):
    s = _lib.Solver(K300_Z, gc.k300(), nit, K300_ETA)
    s.set_expm(_lib.EXPM_LANCZOS, 12, tol)
    return s


@functools.lru_cache(maxsize=None)
def k300_oracle():
    """The oracle's LOG_GAP rows of the K = 300 run on the device generator's sketches."""
    s = k300_handle()
    o = orc.MMWOracle(nit=K300_NIT, eta=K300_ETA, log_gap=True)
    o.run(K300_Z, gc.k300(), lambda it, K, D: s.sketch(K300_SEED, it), factor=False)
    s.close()
    ref = np.array(o.trace["gap"])
    ref.setflags(write=False)
    return ref


def test_chunked_path_against_the_oracle():
    s = k300_handle()
    s.set_gap()
    for n in K300_CALLS:
        s.iterate(n, None, seed=K300_SEED)
    rows, steps = s.gap_log()
    assert_rows(rows, k300_oracle(), "oracle K 300 chunked", steps, s.gap_info())
    assert np.all(steps > 0) and np.all(steps <= 600), steps
    s.close()


# ---- 3 and 4
TWIN_CALLS = (1, 7, 12)
TWIN_NIT = 30


@functools.lru_cache(maxsize=None)
def twins(kind):
    """Twin handles of `kind`, the gap on and off, through the same calls: per call boundary the fields of both and the off twin's
    sums; the on twin's log; on fp64 the off twin's per-call gap() at every boundary."""
    on, off = gc.make(kind, TWIN_NIT), gc.make(kind, TWIN_NIT)
    if gc.KINDS[kind][6]:
        assert on.read(_lib.F_SPMM_KIND)[0] == 3.0, "this kind is expected on the matrix-core kernels"
    on.set_gap()
    snaps, sums, percall = [], [], []
    done = 0
    for n in (0,) + TWIN_CALLS:
        if n:
            on.iterate(n, None, seed=5)
            off.iterate(n, None, seed=5)
            done += n
        if n:  # (the sketch can be read only after an iteration)
            snaps.append(([on.read(f) for f in FIELDS], [off.read(f) for f in FIELDS]))
        sums.append((done, off.read(_lib.F_XAVG), off.read(_lib.F_YAVG)))
        if gc.KINDS[kind][3] == _lib.F64:
            percall.append(off.gap())
    # one more iteration so that the row of the last boundary exists
    on.iterate(1, None, seed=5)
    rows, steps = on.gap_log()
    info, dual = on.gap_info(), on.read(_lib.F_DUAL_INFO)
    on.close()
    off.close()
    return snaps, sums, percall, rows, steps, info, dual


KIND_IDS = list(gc.KINDS)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_phase_only_reads(kind):
    snaps, _, _, rows, steps, info, dual = twins(kind)
    for k, (a, b) in enumerate(snaps):
        for f, x, y in zip(FIELDS, a, b):
            assert x.tobytes() == y.tobytes(), (kind, "boundary", k, "field", f)
    if gc.KINDS[kind][6]:
        assert dual[0] > 0, ("no iteration took its row sums from the matrix-core SDDMM", dual)
    print("[handle-gap] %-30s bitwise over %d boundaries x %d fields; dual info %s; rows %d launches %d"
          % ("only reads " + kind, len(snaps), len(FIELDS), dual, info["rows"], info["launches"]))
    assert np.all(np.isfinite(rows)) and np.all(steps != 0)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_rows_against_a_float64_recomputation(kind):
    _, sums, percall, rows, steps, info, _ = twins(kind)
    p = gc.pattern(kind)
    idx = [d for d, _, _ in sums]
    ref = np.array([gc.recompute(p, x, y, d + 1) for d, x, y in sums])
    assert_rows(rows[idx], ref, "recomputed " + kind, steps[idx], info)
    if percall:
        assert_rows(rows[idx], np.array(percall), "per-call gap() " + kind)


# ---- 5
def test_against_the_batch_row():
    state = gc.k300()
    b = _lib.BatchSolver([K300_Z], [state], K300_NIT, K300_ETA)
    b.set_expm(16, 1e-12)
    b.set_gap(True)
    seeds = np.array([K300_SEED], dtype=np.uint64)
    b.iterate(9, None, seeds)
    s = k300_handle()
    b.export(0, s)
    b.iterate(1, None, seeds)
    brow, bsteps = b.gap_log(0)
    b.close()
    s.set_gap()
    s.iterate(1, None, seed=K300_SEED)
    rows, steps = s.gap_log()
    assert rows.shape == (10, 3) and np.all(np.isnan(rows[:9])) and np.all(steps[:9] == 0)
    assert_rows(rows[9:], brow[9:10], "batch row 9", steps[9:], s.gap_info())
    checks = _lib.gap_checks(300)
    i = checks.index(int(bsteps[9]))
    print("[handle-gap] steps handle %d batch %d" % (steps[9], bsteps[9]))
    assert int(steps[9]) in checks[max(0, i - 1):i + 2], (steps[9], bsteps[9])
    s.close()


# ---- 6
def test_rows_do_not_depend_on_the_enqueue_guess():
    logs, infos = [], []
    for first in (10, 0):
        s = k300_handle(nit=20)
        s.set_gap(first_steps=first)
        s.iterate(20, None, seed=K300_SEED)
        logs.append(s.gap_log())
        infos.append(s.gap_info())
        s.close()
    print("[handle-gap] first_steps 10: %s\n[handle-gap] first_steps 0:  %s" % (infos[0], infos[1]))
    assert logs[0][0].tobytes() == logs[1][0].tobytes() and np.array_equal(logs[0][1], logs[1][1])
    assert infos[0]["continued"] > 0 and infos[0]["capped"] == 0
    # first_steps = 0: the rows of the first chunk go through the cap and none of those is continued (a later chunk's rows follow the
    # steps read back, and may be)
    assert infos[1]["capped"] > 0 and infos[1]["continued"] <= infos[1]["rows"] - infos[1]["capped"]
    assert infos[0]["rows"] == infos[1]["rows"] == 20
    assert_rows(logs[0][0], k300_oracle()[:20], "oracle K 300 first_steps 10", logs[0][1], infos[0])


# ---- 7
def test_a_discarded_chunk_rewrites_its_rows(monkeypatch):
    kind = "f32-er240"
    monkeypatch.setenv("MMW_NO_LAGGED_PLAN", "1")
    monkeypatch.setenv("MMW_DUAL_GAP", "-1")
    nit = 24
    on, off = gc.make(kind, nit + 1), gc.make(kind, nit + 1)
    on.set_gap()
    ref, idx = [], []
    p = gc.pattern(kind)
    done = 0
    for n in (12, 12):
        idx.append(done)
        ref.append(gc.recompute(p, off.read(_lib.F_XAVG), off.read(_lib.F_YAVG), done + 1))
        on.iterate(n, None, seed=3)
        off.iterate(n, None, seed=3)
        done += n
    idx.append(done)
    ref.append(gc.recompute(p, off.read(_lib.F_XAVG), off.read(_lib.F_YAVG), done + 1))
    on.iterate(1, None, seed=3)
    assert on.read(_lib.F_BLOCKING)[3] > 0, "no chunk was discarded"
    rows, steps = on.gap_log()
    assert not np.any(np.isnan(rows)) and np.all(steps != 0)
    assert_rows(rows[idx], np.array(ref), "replayed chunks", steps, on.gap_info())
    on.close()
    off.close()


# ---- 8
@pytest.mark.parametrize("K", [6, 11])
def test_tiny_instances_check_once_at_k(K):
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    state = er_contention_graph(K, 0.5, 1)
    nit = 4
    on, off = _lib.Solver(3, state, nit + 1, 0.05), _lib.Solver(3, state, nit + 1, 0.05)
    on.set_gap()
    p = orc.Pattern(3, state)
    ref = []
    for i in range(nit):
        ref.append(gc.recompute(p, off.read(_lib.F_XAVG), off.read(_lib.F_YAVG), i + 1))
        on.iterate(1, None, seed=2)
        off.iterate(1, None, seed=2)
    rows, steps = on.gap_log()
    assert_rows(rows, np.array(ref), "K %d" % K, steps)
    assert np.all(steps == K), steps
    on.close()
    off.close()


def edge_run(state, Z, rr, dtype, nit, m_cap=0, tol=1e-12):
    on, off = _lib.Solver(Z, state, nit + 1, 0.04, rank_radio=rr, dtype=dtype), _lib.Solver(Z, state, nit + 1, 0.04, rank_radio=rr, dtype=dtype)
    for s in (on, off):
        s.set_expm(_lib.EXPM_LANCZOS, 12, tol)
    on.set_gap(m_cap=m_cap)
    p = orc.Pattern(Z, state)
    ref, idx, done = [], [], 0
    for n in (1, nit - 1):
        idx.append(done)
        ref.append(gc.recompute(p, off.read(_lib.F_XAVG), off.read(_lib.F_YAVG), done + 1))
        on.iterate(n, None, seed=4)
        off.iterate(n, None, seed=4)
        done += n
    idx.append(done)
    ref.append(gc.recompute(p, off.read(_lib.F_XAVG), off.read(_lib.F_YAVG), done + 1))
    on.iterate(1, None, seed=4)
    rows, steps = on.gap_log()
    on.close()
    off.close()
    return rows, steps, idx, np.array(ref)


def test_one_dense_block():
    rows, steps, idx, ref = edge_run(mg.state("one64"), 8, 2, _lib.F64, 6)
    assert_rows(rows[idx], ref, "band_state(64, 31)", steps)
    assert np.all(steps > 0) and np.all(steps <= 64)


def test_hub_row_and_diagonal_only_rows():
    rows, steps, idx, ref = edge_run(mg.state("hub"), 16, 2, _lib.F64, 6)
    assert_rows(rows[idx], ref, "hub", steps)
    assert np.all(steps > 0)


def test_a_cap_that_cuts_the_krylov_space_short():
    g = load_golden("run_env192")
    rows, steps, idx, ref = edge_run(state_from(g), int(g["Z"]), 2, _lib.F64, 6, m_cap=10)
    print("[handle-gap] m_cap 10 at K 192: steps %s, K theta %s against K lambda_min %s" % (steps, rows[idx, 1], ref[:, 1]))
    assert np.all(steps == -10), steps
    bar = 1e-6 * np.abs(ref[:, 1]) + 1e-9
    assert np.all(rows[idx, 1] >= ref[:, 1] - bar)  # a Ritz value bounds lambda_min from above
    assert np.all(np.abs(rows[:, 2] - (rows[:, 0] - rows[:, 1])) <= 1e-12)
    dev, b0 = deviations(rows[idx], ref)
    assert np.all(dev[:, 0] <= b0[:, 0])


def test_log_over_a_handles_life():
    s = k300_handle(nit=12, tol=1e-9)
    with pytest.raises(_lib.MMWError):
        s.gap_log()  # never enabled
    s.set_gap()
    s.iterate(3, None, seed=1)
    s.set_gap(False)
    s.iterate(4, None, seed=1)
    s.set_gap(True)
    s.iterate(5, None, seed=1)
    rows, steps = s.gap_log()
    off = np.arange(12)[3:7]
    assert np.all(np.isnan(rows[off])) and np.all(steps[off] == 0)
    on = np.r_[0:3, 7:12]
    assert np.all(np.isfinite(rows[on])) and np.all(steps[on] > 0)
    out = np.empty(4 * 12 + 4)
    assert _lib.lib().mmw_read_gap(s._h, _lib._pd(out), int(out.size)) == -1  # a wrong length
    with pytest.raises(_lib.MMWError):
        s.set_gap(m_cap=1025)
    s.reset(6)
    rows, steps = s.gap_log()
    assert rows.shape == (0, 3)
    s.iterate(2, None, seed=1)
    rows, steps = s.gap_log()
    assert rows.shape == (2, 3) and np.all(np.isfinite(rows)) and np.all(steps > 0)  # the setting survived the reset
    s.set_slots(30, 5)
    assert s.gap_log()[0].shape == (0, 3)
    s.iterate(5, None, seed=1)
    rows, steps = s.gap_log()
    assert rows.shape == (5, 3) and np.all(np.isfinite(rows)) and np.all(steps > 0)
    s.close()


# ---- 9
def test_class_logs_the_same_table_in_the_loop():
    tables = {}
    for how in ("call", "loop"):
        alg = mmw(nit=K300_NIT, eta=K300_ETA, log_gap=True, gap_log=how, rng="device", dtype="f64", expm_tol=1e-13, device=0, seed=3)
        alg.run_with_state(0, K300_Z, gc.k300())
        tables[how] = alg.LOGGED_NP_DATA["gap"]
        alg.close()
    assert tables["loop"].shape == tables["call"].shape == (K300_NIT, 6)
    assert np.array_equal(tables["loop"][:, 1], tables["call"][:, 1])
    assert_rows(tables["loop"][:, 3:6], tables["call"][:, 3:6], "class loop against call")


@pytest.mark.parametrize("where", ["host", "env"])
def test_convergence_module(where):
    if where == "host":
        out = convergence(K300_Z, gc.k300(), K300_NIT, K300_ETA, seed=K300_SEED, expm_tol=1e-12)
    else:
        _, env = journal_graph_device(10, 75e-4, 0)
        out = convergence(K300_Z, env.device_state(), K300_NIT, K300_ETA, seed=K300_SEED, expm_tol=1e-12)
        env.close()
    assert out["gap"].shape == (K300_NIT, 3) and out["lanczos_steps"].shape == (K300_NIT,)
    assert_rows(out["gap"], k300_oracle(), "convergence() " + where, out["lanczos_steps"])
    assert np.all(out["lanczos_steps"] > 0)
