#!/usr/bin/env python
"""The convergence sweep (LOG_GAP over nit = ceil(1 / eta^2) iterations, mmw.py:79-117) on a solver handle at journal-1pct
(N = 10 003, Z = 186, eta = 0.04), fp32 and fp64: the rows logged inside the loop (`Solver.set_gap`, one `iterate(nit)`) against one
`Solver.gap()` call per row in front of a one-iteration `iterate` (what `mmw(log_gap=True)` does by default), `--reps` sweeps each
in one session.  Prints one JSON line per sweep (wall time, the launches and continuations of `gap_info()`, the steps' minimum, mean
and maximum), one per dtype with the spread, and for three rows the deviation of the logged row from `scipy.sparse.linalg.eigsh` on
the sums read back at that iteration.

    python tools/gap_handle_sweep.py > profiles/gap_handle.log
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import scipy.sparse.linalg  # noqa: E402

from oracle import mmw_oracle as orc  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph  # noqa: E402


def sweep_loop(s, nit, seed):
    s.reset(nit)
    s.set_gap(True)
    before = s.gap_info()
    t0 = time.perf_counter()
    s.iterate(nit, None, seed=seed)
    rows, steps = s.gap_log()
    dt = time.perf_counter() - t0
    after = s.gap_info()
    s.set_gap(False)
    return dt, rows, steps, {k: after[k] - before[k] for k in ("rows", "continued", "capped", "launches")}


def sweep_call(s, nit, seed):
    s.reset(nit)
    s.set_gap(False)
    rows = np.empty((nit, 3))
    t0 = time.perf_counter()
    for i in range(nit):
        rows[i] = s.gap()
        s.iterate(1, None, seed=seed)
    s.sync()
    return time.perf_counter() - t0, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=28)
    ap.add_argument("--rho", type=float, default=0.0319)
    ap.add_argument("--Z", type=int, default=186)
    ap.add_argument("--eta", type=float, default=0.04)
    ap.add_argument("--nit", type=int, default=0, help="0: ceil(1 / eta^2)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--no-call", action="store_true", help="skip the per-call sweeps")
    ap.add_argument("--eigsh-rows", type=int, nargs="*", default=None)
    a = ap.parse_args()
    nit = a.nit or int(math.ceil(1.0 / a.eta ** 2))
    state = journal_graph(cell_size=a.cell, sta_density_per_1m2=a.rho, seed=0)
    K = state[0].shape[0]
    print(json.dumps({"workload": "journal cell %d rho %g" % (a.cell, a.rho), "K": K, "Z": a.Z, "eta": a.eta, "nit": nit, "reps": a.reps}), flush=True)
    logged = {}
    for name, dtype in (("f32", _lib.F32), ("f64", _lib.F64)):
        s = _lib.Solver(a.Z, state, nit, a.eta, dtype=dtype)
        s.iterate(min(nit, 40), None, seed=a.seed)  # warm-up: the handle's lazy tables, the chunk policy's first plans
        s.sync()
        times = {"loop": [], "call": []}
        for r in range(a.reps):
            dt, rows, steps, info = sweep_loop(s, nit, a.seed)
            times["loop"].append(dt)
            logged[name] = rows
            print(json.dumps({"dtype": name, "path": "loop", "rep": r, "seconds": round(dt, 4), **info, "launches_per_row": round(info["launches"] / nit, 1),
                              "steps_min": int(np.abs(steps).min()), "steps_mean": round(float(np.abs(steps).mean()), 1), "steps_max": int(np.abs(steps).max()),
                              "rows_capped_short": int((steps < 0).sum()), "bytes": s.gap_info()["bytes"]}), flush=True)
        for r in range(0 if a.no_call else a.reps):
            dt, rows_c = sweep_call(s, nit, a.seed)
            times["call"].append(dt)
            d = np.abs(rows_c - logged[name])
            print(json.dumps({"dtype": name, "path": "call", "rep": r, "seconds": round(dt, 4),
                              "worst_abs_difference_to_loop_rows": [float("%.3g" % x) for x in d.max(axis=0)]}), flush=True)
        out = {"dtype": name}
        for k, v in times.items():
            if v:
                out[k] = {"min_s": round(min(v), 4), "median_s": round(float(np.median(v)), 4), "max_s": round(max(v), 4)}
        if times["call"]:
            out["call_min_over_loop_max"] = round(min(times["call"]) / max(times["loop"]), 2)
        print(json.dumps(out), flush=True)
        if name == "f64":
            p = orc.Pattern(a.Z, state)
            at = sorted(set(a.eigsh_rows if a.eigsh_rows is not None else [0, nit // 5, nit - 1]))
            s.reset(nit)
            done = 0
            for i in at:
                if i > done:
                    s.iterate(i - done, None, seed=a.seed)
                    done = i
                xs, ys = s.read(_lib.F_XAVG), s.read(_lib.F_YAVG)
                e_max = float(np.max(orc.violations(p, xs / (i + 1))))
                lam, _ = scipy.sparse.linalg.eigsh(p.csr(orc.loss_values(p, ys / (i + 1))), k=1, which="SA", tol=1e-12)
                ref = np.array([e_max, lam[0] * K, e_max - lam[0] * K])
                print(json.dumps({"dtype": name, "eigsh_row": i, "logged": [float(x) for x in logged[name][i]], "eigsh": [float(x) for x in ref],
                                  "abs_deviation": [float("%.3g" % x) for x in np.abs(logged[name][i] - ref)]}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
