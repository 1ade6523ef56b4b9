"""Developer tool (GPU box): what building a batch on the device from CSR states that lie there costs against building it on the host.

    python tools/batch_from_csr.py [--workloads sweep-64,sweep-256,er-5pct-2k-x8] [--reps 5] [--out profiles/batch_from_csr.log]

Workloads: tools/batch_small.py's `sweep(n)` (journal_graph(cell, 75e-4, seed), cells 5..15, K = 75 ... 675) at 64 and 256 instances, Z at
the middle of each instance's bisection bounds; and 8 x er_contention_graph(2000, 0.05), Z 32.  Per workload two legs are timed:
  host    BatchSolver(Zs, states, ...)          mmw_batch_create: build_pattern per instance on the host, both arenas uploaded whole
  device  BatchSolver.from_csr(csrs, Zs, ...)   mmw_batch_create_from_csr: one workgroup per instance from the arrays already there
and, listed apart because it is paid once per state and not per batch, `upload`: DeviceCSR.upload of all the states.  The host leg
includes the wrapper's look at the scipy matrices (`_lib._state_arrays`), as any caller of BatchSolver pays it; the device leg starts
from the DeviceCSRs.  One throwaway of each leg first, then the two legs alternate, `--reps` repetitions, reported as median
(min - max), one JSON line per workload.  The comparator is the same build's mmw_batch_create.  Every workload runs in a child process
of its own under `timeout -k 10`; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = {"sweep-64": 120, "sweep-256": 300, "er-5pct-2k-x8": 240}  # name -> the child's time limit in seconds


def make(name):
    from batch_small import sweep
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    if name.startswith("sweep-"):
        return sweep(int(name.split("-")[1]))
    return [er_contention_graph(2000, 0.05, seed=100 + i) for i in range(8)], [32] * 8


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2)}


def one(name, reps, nit):
    from sig_sdp_mmw_amd import _lib
    states, Zs = make(name)

    def timed(fn):
        t0 = time.perf_counter()
        h = fn()
        t = time.perf_counter() - t0
        if isinstance(h, list):
            return t, h
        h.close()
        return t, None

    def host():
        return _lib.BatchSolver(Zs, states, nit, 0.04)

    def upload():
        return [_lib.DeviceCSR.upload(s) for s in states]
    _, csrs = timed(upload)
    timed(host)
    timed(lambda: _lib.BatchSolver.from_csr(csrs, Zs, nit, 0.04))
    for c in csrs:
        c.close()
    t_up, t_host, t_dev = [], [], []
    for _ in range(reps):
        t, csrs = timed(upload)
        t_up.append(t)
        t_host.append(timed(host)[0])
        t_dev.append(timed(lambda: _lib.BatchSolver.from_csr(csrs, Zs, nit, 0.04))[0])
        for c in csrs:
            c.close()
    b = host()
    rec = {"workload": name, "B": len(states), "K_sum": sum(s["K"] for s in b.sizes), "K_max": max(s["K"] for s in b.sizes),
           "nnzL_sum": sum(s["nnzL"] for s in b.sizes), "reps": reps, "host": stats(t_host), "device": stats(t_dev), "upload": stats(t_up),
           "device_over_host": round(statistics.median(t_dev) / statistics.median(t_host), 3)}
    b.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this workload in this process")
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.reps, args.nit)
    for name in args.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(WORKLOADS[name]), sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(args.reps), "--nit", str(args.nit)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit("%s ended with status %d: nothing more is started" % (name, r.returncode))
        if args.out:
            with open(args.out, "a") as f:
                f.write(r.stdout)


if __name__ == "__main__":
    main()
