"""Developer tool (GPU box): wall time per time point of the reference's online sweeps (sim_script/journal_version/sim_mmw_online.py:
re-round Z_fin's factor on the moved stations, score, move on), batched against per-instance.

    python tools/batch_online.py [--instances 64] [--points 11] [--step-us 1e6] [--speed 0.1] [--nit 150]

Workload: `mobile_drop(10, 75e-4, seed)` for seed = 0 .. instances-1 (K = 300, the sweeps' cell size).
  batch      `batch.online_many`'s loop: BatchEnv.move + BatchSolver.round_env + BatchEnv.evaluate, all instances per call
  instances  the only path without the batched environment, in the same process on the same factors and positions: per instance a
             fresh `_lib.DeviceEnv`, a `_lib.Solver` built from its moved state only to serve `round`, nattempt x Z x rank NumPy
             normals drawn and uploaded, `Solver.round`, `DeviceEnv.evaluate`
One JSON line per path: seconds per point (every point, and the median) and per instance-point."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from sig_sdp_mmw_amd.graphs import min_sinr_dec, mobile_drop  # noqa: E402


def report(path, B, per_point, extra=None):
    med = float(np.median(per_point))
    row = {"workload": "online-cell10-75e-4", "path": path, "instances": B, "points": len(per_point),
           "seconds_per_point": [round(t, 5) for t in per_point], "median_seconds_per_point": round(med, 5),
           "us_per_instance_point": round(med * 1e6 / B, 1)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)
    return med


def per_instance(drops, Zs, gX, n_points, step_us, speed, nattempt, eta, seed):
    msinr = min_sinr_dec()
    per_point = []
    for p in range(n_points):
        t0 = time.perf_counter()
        for i, d in enumerate(drops):
            env = _lib.DeviceEnv(d.sta_locs, d.ap_locs, min_sinr=msinr)
            h = _lib.Solver(Zs[i], env.state(), 1, eta, dtype=_lib.F64)
            z_vec, _, _ = batch._round(h, Zs[i], gX[i], None, batch.probe_seed(seed, i, 0x80000 | p), nattempt)
            env.evaluate(z_vec, Zs[i])
            h.close()
            env.close()
        per_point.append(time.perf_counter() - t0)
        for d in drops:
            d.step_time(step_us, speed)
    return per_point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--step-us", type=float, default=1e6)
    ap.add_argument("--speed", type=float, default=0.1)
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--skip-instances", action="store_true", help="the batch alone (for a kernel trace)")
    a = ap.parse_args()
    B, eta, seed, nattempt = a.instances, 0.04, 0, 10
    batch.online_many([mobile_drop(5, 75e-4, s) for s in range(2)], n_points=1, nit=4)  # module load, first launches
    drops = [mobile_drop(10, 75e-4, s) for s in range(B)]
    states = [d.state() for d in drops]
    timings = []
    t0 = time.perf_counter()
    res = batch.online_many(drops, n_points=a.points, step_us=a.step_us, mob_spd_meter_s=a.speed, nit=a.nit, eta=eta, seed=seed, nattempt=nattempt,
                            timings=timings)
    total = time.perf_counter() - t0
    Zs = [r["Z"] for r in res]
    tb = report("batch", B, [t["device_s"] for t in timings],
                {"online_many_seconds": round(total, 3), "host_walk_seconds_per_point": round(float(np.median([t["step_s"] for t in timings])), 5),
                 "Z_range": [min(Zs), max(Zs)], "mean_remainder": round(float(np.mean([r["remainder"].mean() for r in res])), 3),
                 "mean_bler": float(np.mean([r["bler"].mean() for r in res]))})
    if a.skip_instances:
        return
    # the same factors for the per-instance path: the solve at Z_fin that online_many runs
    b = _lib.BatchSolver(Zs, states, a.nit, eta)
    b.iterate(a.nit, None, np.array([batch.probe_seed(seed, i, len(res[i]["probes"])) for i in range(B)], dtype=np.uint64))
    b.factor()
    gX = [b.read_factor(i) for i in range(B)]
    b.close()
    ti = report("instances", B, per_instance([mobile_drop(10, 75e-4, s) for s in range(B)], Zs, gX, a.points, a.step_us, a.speed, nattempt, eta, seed))
    print(json.dumps({"workload": "online-cell10-75e-4", "instances_over_batch": round(ti / tb, 2)}), flush=True)


if __name__ == "__main__":
    main()
