"""Developer tool (GPU box): the reference's convergence sweep with LOG_GAP (sim_script/ton_major_rv/sim_convergence_rho.py: cell 10,
five densities x 20 seeds, eta 0.04, nit 625) through
  (a) the batched solver with the gap logged inside the launch (csrc/kernels_batch.h, k_mmw_batch<true>),
  (b) the batched solver without the gap,
  (c) the per-handle path as sig_sdp_mmw_amd/mmw.py runs LOG_GAP: fp64 handles, `gap()` + `iterate(1)` per iteration, 8 handles
      resident at a time (tools/batch_small.py's run_handles); its rate is per instance, so --handle-cap keeps it short.

    python tools/batch_gap.py [--seeds 20] [--nit 625] [--reps 3] [--handle-cap 8] [--skip-handles] [--only-batch-gap]

Z is the middle of each instance's bisection bounds (the reference takes it from its ADMM run).  One JSON line per measurement:
seconds, instances/s, time per instance-iteration, and for (a) the mean / max Lanczos steps per instance."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph  # noqa: E402

RHOS = (25e-4, 50e-4, 75e-4, 100e-4, 125e-4)


def workload(nseeds):
    bs = binary_search_relaxation()
    states, Zs = [], []
    for rho in RHOS:
        for seed in range(nseeds):
            st = journal_graph(10, rho, seed=seed)
            lb, ub = bs.set_bounds(st)
            states.append(st)
            Zs.append(max(2, (lb + ub) // 2))
    return states, Zs


def run_batch(states, Zs, nit, eta, gap):
    b = _lib.BatchSolver(Zs, states, nit, eta)
    if gap:
        b.set_gap(True)
    t0 = time.perf_counter()
    b.iterate(nit, None, np.arange(len(states), dtype=np.uint64) + 1)
    logs = [b.gap_log(i) for i in range(len(states))] if gap else None  # the one readback of the gap table is part of the run
    t = time.perf_counter() - t0
    b.close()
    return t, logs


def run_handles(states, Zs, nit, eta, resident=8):
    t_all = 0.0
    for g in range(0, len(states), resident):
        hs = [_lib.Solver(Z, st, nit, eta, dtype=_lib.F64) for Z, st in zip(Zs[g:g + resident], states[g:g + resident])]
        for h in hs:
            h.set_expm(_lib.EXPM_TAYLOR, 16, 1e-9)
        t0 = time.perf_counter()
        for _ in range(nit):
            for h in hs:
                h.gap()
                h.iterate(1, None, 1)
        for h in hs:
            h.sync()
        t_all += time.perf_counter() - t0
        for h in hs:
            h.close()
    return t_all


def report(path, B, nit, t, K, extra=None):
    row = {"workload": "convergence-rho-cell10", "path": path, "instances": B, "nit": nit, "K_range": [int(min(K)), int(max(K))],
           "seconds": round(t, 4), "instances_per_s": round(B / t, 3), "us_per_instance_iteration": round(t * 1e6 / (B * nit), 3)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--nit", type=int, default=625)
    ap.add_argument("--eta", type=float, default=0.04)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--handle-cap", type=int, default=8, help="instances the handle path runs (its rate is per instance)")
    ap.add_argument("--skip-handles", action="store_true")
    ap.add_argument("--only-batch-gap", action="store_true", help="one run of (a) alone, for a kernel trace")
    a = ap.parse_args()
    states, Zs = workload(a.seeds)
    K = [st[0].shape[0] for st in states]
    B = len(states)
    if a.only_batch_gap:
        t, logs = run_batch(states, Zs, a.nit, a.eta, True)
        report("batch-gap", B, a.nit, t, K)
        return
    run_batch(states[:2], Zs[:2], 2, a.eta, True)  # module load, first launches
    run_batch(states[:2], Zs[:2], 2, a.eta, False)
    for _ in range(a.reps):
        t, logs = run_batch(states, Zs, a.nit, a.eta, True)
        steps = np.array([np.abs(s).mean() for _, s in logs])
        capped = int(sum(int(np.any(s <= 0)) for _, s in logs))
        report("batch-gap", B, a.nit, t, K, {"lanczos_steps_mean": round(float(steps.mean()), 1),
                                             "lanczos_steps_max": int(max(np.abs(s).max() for _, s in logs)),
                                             "instances_with_a_capped_row": capped})
        t, _ = run_batch(states, Zs, a.nit, a.eta, False)
        report("batch-nogap", B, a.nit, t, K)
    if not a.skip_handles:
        # spread the capped handle instances over the five densities
        pick = [int(i) for i in np.linspace(0, B - 1, min(B, a.handle_cap)).round()]
        hs, hz = [states[i] for i in pick], [Zs[i] for i in pick]
        for _ in range(a.reps):
            report("handles-gap-8-resident", len(pick), a.nit, run_handles(hs, hz, a.nit, a.eta), [K[i] for i in pick])


if __name__ == "__main__":
    main()
