"""Developer tool (GPU box): throughput of the batched solver (one workgroup per instance, csrc/kernels_batch.h) against resident
handles on 8 streams (as tools/batch_throughput.py drives them), fp64, device sketches, default expm tolerance (1e-9).

    python tools/batch_small.py [--sizes 64,128,256] [--nit 150] [--er-nit 150] [--handle-cap 64] [--skip-er]

Workloads: sweep batches of journal_graph(cell, 75e-4, seed) for cells 5..15 (the reference's journal sweeps, K = 75 ... 675),
Z at the middle of each instance's bisection bounds; and the BASELINE configs[3] shape (8 x er_contention_graph(2000, 0.05), Z 32).
One JSON line per measurement: instances/s, aggregate iterations/s, and the batch launch's time per instance-iteration."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.binary_search import binary_search_relaxation  # noqa: E402
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph  # noqa: E402


def sweep(n):
    cells = list(range(5, 16))
    states, Zs = [], []
    bs = binary_search_relaxation()
    for i in range(n):
        st = journal_graph(cells[i % len(cells)], 75e-4, seed=1 + i // len(cells))
        lb, ub = bs.set_bounds(st)
        states.append(st)
        Zs.append(max(2, (lb + ub) // 2))
    return states, Zs


def run_batch(states, Zs, nit, eta=0.04):
    b = _lib.BatchSolver(Zs, states, nit, eta)
    t0 = time.perf_counter()
    b.iterate(nit, None, np.arange(len(states), dtype=np.uint64) + 1)
    t = time.perf_counter() - t0
    b.close()
    return t


def run_handles(states, Zs, nit, eta=0.04, streams=8, chunk=16):
    """Resident handles, `streams` at a time, iterations enqueued round-robin (each handle has its own HIP stream)."""
    t_all = 0.0
    for g in range(0, len(states), streams):
        hs = [_lib.Solver(Z, st, nit, eta, dtype=_lib.F64) for Z, st in zip(Zs[g:g + streams], states[g:g + streams])]
        t0 = time.perf_counter()
        for s in range(0, nit, chunk):
            for h in hs:
                h.iterate(min(chunk, nit - s), None, 1)
        for h in hs:
            h.sync()
        t_all += time.perf_counter() - t0
        for h in hs:
            h.close()
    return t_all


def report(name, B, nit, t, path, K):
    print(json.dumps({"workload": name, "path": path, "instances": B, "nit": nit, "K_range": [int(min(K)), int(max(K))],
                      "seconds": round(t, 4), "instances_per_s": round(B / t, 2), "iterations_per_s": round(B * nit / t, 1),
                      "us_per_instance_iteration": round(t * 1e6 / (B * nit), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--er-nit", type=int, default=150)
    ap.add_argument("--handle-cap", type=int, default=64, help="instances the handle path runs (its rate is per instance)")
    ap.add_argument("--skip-er", action="store_true")
    ap.add_argument("--skip-handles", action="store_true")
    a = ap.parse_args()
    s0, z0 = sweep(2)
    run_batch(s0, z0, 2)  # module load, first launch
    for B in [int(x) for x in a.sizes.split(",") if x]:
        states, Zs = sweep(B)
        K = [st[0].shape[0] for st in states]
        report("journal-sweep-75e-4", B, a.nit, run_batch(states, Zs, a.nit), "batch", K)
        if not a.skip_handles:
            n = min(B, a.handle_cap)
            report("journal-sweep-75e-4", n, a.nit, run_handles(states[:n], Zs[:n], a.nit), "handles-8-streams", K[:n])
    if not a.skip_er:
        states = [er_contention_graph(2000, 0.05, seed=100 + i) for i in range(8)]
        Zs = [32] * 8
        K = [2000] * 8
        report("er-5pct-2k-x8", 8, a.er_nit, run_batch(states, Zs, a.er_nit), "batch", K)
        if not a.skip_handles:
            report("er-5pct-2k-x8", 8, a.er_nit, run_handles(states, Zs, a.er_nit), "handles-8-streams", K)


if __name__ == "__main__":
    main()
