"""Developer tool (GPU box): does a re-solve at every time point of the online sweep pay on ONE instance of any K, on the solver
handle, and does carrying the iterate across the moved states (`Solver.carry_from`, csrc/kernels_carry.h) buy what a third of the
iterations loses?  The handle's tools/batch_online_resolve.py.

    python tools/online_resolve_handle.py [--cell 28] [--rho 0.0319] [--points 11] [--step-us 1e6] [--speeds 1,3] [--nit 150] [--runs 3]
                                          [--skip LEG[,LEG]] [--only LEG]

Workload: `mobile_drop(28, 0.0319, r)`, the benchmark instance (N = 10 003, fp32); run r walks the drop of seed r and keys the solver
by seed r, so the runs are samples and not one repeated.  Legs, alternating inside every run on copies of the same drop:
  reround    `online.online_sweep`: one solve at Z_fin, that factor re-rounded at every point (the reference's scripts)
  cold       `online.online_resolve_sweep(carry=False)`: a cold re-solve with `nit` iterations per point
  cold3      the same with ceil(nit / 3) iterations
  carried    `online.online_resolve_sweep(carry=True)`: ceil(nit / 3) iterations from the previous point's iterate
One JSON line per (speed, run, leg): mean BLER over points and users, the share of points with users left over, seconds per point
split as `timings` splits them (medians over the points after point 0) -- or the error that ended the leg's sweep; then per
(speed, leg) the median of the runs that finished.  Last, the
carry by itself on the first drop moved one step: `carry_from` + `sync` on a fresh destination, against `DeviceEnv.move`.
--only runs one leg once at the first speed (for a kernel trace of its own)."""
import argparse
import copy
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib, online  # noqa: E402
from sig_sdp_mmw_amd.graphs import mobile_drop  # noqa: E402

LEGS = ("reround", "cold", "cold3", "carried")
PARTS = ("create_s", "carry_s", "iterate_s", "epilogue_s", "evaluate_s", "step_s")


def run_leg(leg, drop, a, speed, seed):
    kw = dict(n_points=a.points, step_us=a.step_us, mob_spd_meter_s=speed, nit=a.nit, eta=0.04, seed=seed, nattempt=10)
    n3 = int(math.ceil(a.nit / 3.0))
    tm = []
    np.random.seed(seed)  # (the search's roundings draw from the global stream)
    t0 = time.perf_counter()
    if leg == "reround":
        res = online.online_sweep(drop, timings=tm, **kw)
        split = {"device_s": float(np.median([t["device_s"] for t in tm[1:] or tm])), "step_s": float(np.median([t["step_s"] for t in tm]))}
    else:
        res = online.online_resolve_sweep(drop, carry=leg == "carried", resolve_nit=a.nit if leg == "cold" else n3, timings=tm, **kw)
        split = {k: float(np.median([t[k] for t in tm[1:] or tm])) for k in PARTS}
    total = time.perf_counter() - t0
    per_point = float(np.median([sum(v for k, v in t.items() if k != "step_s") for t in tm[1:] or tm]))
    later = res["bler"][1:] if a.points > 1 else res["bler"]
    return {"leg": leg, "speed": speed, "seed": seed, "K": drop.K, "Z": res["Z"], "points": a.points, "iters_per_point": a.nit if leg in ("reround", "cold") else n3,
            "mean_bler": float(res["bler"].mean()), "mean_bler_after_point_0": float(later.mean()), "share_points_with_remainder": float(np.mean(res["remainder"] > 0)),
            "seconds_per_point": round(per_point, 4), "split": {k: round(v, 5) for k, v in split.items()}, "total_seconds": round(total, 2)}


def carry_alone(a, speed, reps=7):
    """`carry_from` + `sync` on fresh destinations, and `DeviceEnv.move`, in milliseconds (medians)."""
    drop = mobile_drop(a.cell, a.rho, 0)
    env = online._env(drop, 0)
    Z, n = 40, 8
    src = _lib.Solver.from_env(env, Z, n, 0.04, dtype=_lib.F32)
    src.iterate(n, None, seed=1)
    src.sync()
    here = drop.sta_locs.copy()
    drop.step_time(a.step_us, speed, 1e5)
    t_move, t_carry = [], []
    for _ in range(reps):
        env.move(here)
        t0 = time.perf_counter()
        env.move(drop.sta_locs)
        t_move.append(time.perf_counter() - t0)
        dst = _lib.Solver.from_env(env, Z, n, 0.04, dtype=_lib.F32)
        dst.sync()
        t0 = time.perf_counter()
        dst.carry_from(src)
        dst.sync()
        t_carry.append(time.perf_counter() - t0)
        dst.close()
    out = {"carry_alone": "carry_from + sync on a fresh destination", "K": drop.K, "nnzL": src.nnzL, "speed": speed, "carry_ms": round(float(np.median(t_carry)) * 1e3, 3),
           "carry_ms_min": round(float(np.min(t_carry)) * 1e3, 3), "move_ms": round(float(np.median(t_move)) * 1e3, 3)}
    src.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=28)
    ap.add_argument("--rho", type=float, default=0.0319)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--step-us", type=float, default=1e6)
    ap.add_argument("--speeds", default="1,3")
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip", default="", help="legs to leave out, comma separated")
    ap.add_argument("--only", default="", help="one leg, one run, the first speed (for a kernel trace)")
    a = ap.parse_args()
    speeds = [float(s) for s in a.speeds.split(",")]
    legs = [leg for leg in LEGS if leg not in a.skip.split(",")]
    if a.only:
        legs, speeds, a.runs = [a.only], speeds[:1], 1
    for leg in legs:
        if leg not in LEGS:
            raise SystemExit("unknown leg %r (legs: %s)" % (leg, ", ".join(LEGS)))
    online.online_resolve_sweep(mobile_drop(5, 75e-4, 0), n_points=2, nit=8, carry=True)  # module load, first launches
    rows = []
    for speed in speeds:
        for r in range(a.runs):
            base = mobile_drop(a.cell, a.rho, r)
            for leg in legs:
                try:
                    row = run_leg(leg, copy.deepcopy(base), a, speed, r)
                except _lib.MMWError as e:  # (a factor that did not converge ends the leg's sweep: recorded, not hidden)
                    row = {"leg": leg, "speed": speed, "seed": r, "error": str(e)}
                row["run"] = r
                rows.append(row)
                print(json.dumps(row), flush=True)
    for speed in speeds:
        for leg in legs:
            mine = [x for x in rows if x["speed"] == speed and x["leg"] == leg and "error" not in x]
            if not mine:
                continue
            print(json.dumps({"summary": "median of %d runs" % len(mine), "speed": speed, "leg": leg,
                              "mean_bler": float(np.median([x["mean_bler"] for x in mine])),
                              "mean_bler_after_point_0": float(np.median([x["mean_bler_after_point_0"] for x in mine])),
                              "share_points_with_remainder": float(np.median([x["share_points_with_remainder"] for x in mine])),
                              "seconds_per_point": float(np.median([x["seconds_per_point"] for x in mine])),
                              **{k: float(np.median([x["split"].get(k, 0.0) for x in mine])) for k in PARTS[:5]}}), flush=True)
    if not a.only:
        print(json.dumps(carry_alone(a, speeds[-1])), flush=True)


if __name__ == "__main__":
    main()
