"""Developer tool (GPU box): does a re-solve at every time point of the online sweeps pay, and does carrying the iterate across
the moved states (`BatchSolver.carry_from`, csrc/kernels_batch_carry.h) buy what a third of the iterations loses?

    python tools/batch_online_resolve.py [--instances 64] [--points 11] [--step-us 1e6] [--speeds 0.1,1,3] [--nit 150] [--runs 3]
                                         [--skip LEG[,LEG]] [--only LEG] [--handover host,device] [--factor-split auto]

Workload: `mobile_drop(cell, 75e-4, seed)` over the sweep's mix, cells 5..15 (K = 75 ... 675) as tools/batch_small.py's `sweep(n)`
deals them; run r of a speed walks the drops of seeds 1 + r * 100 + i // 11 and keys the solver by seed r, so the three runs are
three samples and not one repeated.  Legs, alternating inside every run on copies of the same drops:
  reround    `batch.online_many`: one solve at Z_fin, that factor re-rounded at every point (the reference's scripts)
  cold       `batch.online_resolve_many(carry=False)`: a cold re-solve with `nit` iterations per point
  cold3      the same with ceil(nit / 3) iterations
  carried    `batch.online_resolve_many(carry=True)`: ceil(nit / 3) iterations from the previous point's iterate
One JSON line per (speed, run, leg): mean BLER over points and instances, the share of points with remainder > 0, seconds per point
split as `timings` splits them (medians over the points after point 0); then per (speed, leg) the median of the runs.  --only runs
one leg once at the first speed (for a kernel trace of its own).  --handover: how the re-solving legs hand a point's states to its
batch (`online_resolve_many(handover=...)`); with both values every such leg runs once per value, alternating inside the run, and
the rows carry "handover".  --factor-split goes to every leg as `factor_split`."""
import argparse
import copy
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import mobile_drop  # noqa: E402

LEGS = ("reround", "cold", "cold3", "carried")
PARTS = ("create_s", "carry_s", "iterate_s", "epilogue_s", "evaluate_s", "step_s")


def drops_of(n, run):
    cells = list(range(5, 16))
    return [mobile_drop(cells[i % len(cells)], 75e-4, 1 + run * 100 + i // len(cells)) for i in range(n)]


def run_leg(leg, drops, a, speed, seed, handover="host"):
    kw = dict(n_points=a.points, step_us=a.step_us, mob_spd_meter_s=speed, nit=a.nit, eta=0.04, seed=seed, nattempt=10,
              factor_split=a.factor_split or None)
    n3 = int(math.ceil(a.nit / 3.0))
    tm = []
    t0 = time.perf_counter()
    if leg == "reround":
        res = batch.online_many(drops, timings=tm, **kw)
        split = {"device_s": float(np.median([t["device_s"] for t in tm[1:] or tm])), "step_s": float(np.median([t["step_s"] for t in tm]))}
    else:
        res = batch.online_resolve_many(drops, carry=leg == "carried", resolve_nit=a.nit if leg == "cold" else n3, timings=tm, handover=handover, **kw)
        split = {k: float(np.median([t[k] for t in tm[1:] or tm])) for k in PARTS}
    total = time.perf_counter() - t0
    per_point = float(np.median([sum(v for k, v in t.items() if k != "step_s") for t in tm[1:] or tm]))
    bler = np.concatenate([r["bler"].ravel() for r in res])
    rem = np.concatenate([r["remainder"] for r in res])
    later = np.concatenate([r["bler"][1:].ravel() for r in res]) if a.points > 1 else bler
    return {"leg": leg, "handover": handover if leg != "reround" else "-", "speed": speed, "seed": seed, "instances": len(drops), "points": a.points, "iters_per_point": a.nit if leg in ("reround", "cold") else n3,
            "mean_bler": float(bler.mean()), "mean_bler_after_point_0": float(later.mean()), "share_points_with_remainder": float(np.mean(rem > 0)),
            "seconds_per_point": round(per_point, 4), "split": {k: round(v, 4) for k, v in split.items()}, "total_seconds": round(total, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--step-us", type=float, default=1e6)
    ap.add_argument("--speeds", default="0.1,1,3")
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip", default="", help="legs to leave out, comma separated")
    ap.add_argument("--only", default="", help="one leg, one run, the first speed (for a kernel trace)")
    ap.add_argument("--handover", default="host", help="host, device or both comma separated: the re-solving legs run once per value")
    ap.add_argument("--factor-split", default="", help="factor_split of every leg (e.g. auto)")
    a = ap.parse_args()
    hands = a.handover.split(",")
    for h in hands:
        if h not in ("host", "device"):
            raise SystemExit("unknown handover %r (host, device)" % h)
    speeds = [float(s) for s in a.speeds.split(",")]
    legs = [leg for leg in LEGS if leg not in a.skip.split(",")]
    if a.only:
        legs, speeds, a.runs = [a.only], speeds[:1], 1
    for leg in legs:
        if leg not in LEGS:
            raise SystemExit("unknown leg %r (legs: %s)" % (leg, ", ".join(LEGS)))
    batch.online_resolve_many([mobile_drop(5, 75e-4, s) for s in range(2)], n_points=2, nit=4)  # module load, first launches
    rows = []
    for speed in speeds:
        for r in range(a.runs):
            base = drops_of(a.instances, r)
            for leg in legs:
                for h in hands if leg != "reround" else ["host"]:
                    row = run_leg(leg, copy.deepcopy(base), a, speed, r, h)
                    row["run"] = r
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    for speed in speeds:
        for leg, h in [(leg, h) for leg in legs for h in (hands if leg != "reround" else ["-"])]:
            mine = [x for x in rows if x["speed"] == speed and x["leg"] == leg and x["handover"] == h]
            print(json.dumps({"summary": "median of %d runs" % len(mine), "speed": speed, "leg": leg, "handover": h,
                              "mean_bler": float(np.median([x["mean_bler"] for x in mine])),
                              "mean_bler_after_point_0": float(np.median([x["mean_bler_after_point_0"] for x in mine])),
                              "share_points_with_remainder": float(np.median([x["share_points_with_remainder"] for x in mine])),
                              "seconds_per_point": float(np.median([x["seconds_per_point"] for x in mine])),
                              "create_s": float(np.median([x["split"].get("create_s", 0.0) for x in mine])),
                              "carry_s": float(np.median([x["split"].get("carry_s", 0.0) for x in mine])),
                              "iterate_s": float(np.median([x["split"].get("iterate_s", 0.0) for x in mine])),
                              "epilogue_s": float(np.median([x["split"].get("epilogue_s", 0.0) for x in mine]))}), flush=True)


if __name__ == "__main__":
    main()
