"""Developer tool (GPU box): wall time per time point of the online sweep on the solver handle (`online.online_sweep`:
DeviceEnv.move + Solver.round_env + DeviceEnv.evaluate) against the only route without them, in the same process, alternating
point by point on the same positions, factor and draws.

    python tools/online_handle.py [--cell 28] [--rho 0.0319] [--seed 0] [--points 11] [--step-us 1e6] [--speed 0.1] [--nit 150]

Workload: `mobile_drop(28, 0.0319, seed)`, the benchmark instance (N = 10 003), Z from the cold search as `online_sweep` runs it.
  handle   env.move(positions), `online.round_point` (round_env of the resident factor, first feasible of `nattempt`), env.evaluate
  rebuild  a fresh `DeviceEnv` at the positions, `Solver.from_env` on it, the factor uploaded with every `round`, evaluate
Point 0 is thrown away (first launches of every kernel).  After the timed part of a point the handle route is taken apart once
more: move / first round_env (lists + round) / second round_env on the cached lists (round alone) / evaluate.
One JSON line per point, then one with the medians and min-max of points 1..

    python tools/online_handle.py --draws [the same options]

The same instance and points, three legs per point instead: "host" (`online.round_point`: the sequential attempts, directions drawn
by NumPy), "device" (`online.round_point_device`: one `round_env_attempts` call, pick="first") and "fewest" (the same call with
pick="fewest"), each as move + round + evaluate, the order of the legs rotating point by point.  The colourings differ between
"host" and the other two because the directions do; per leg the line gives the users left over and the mean BLER.  After the timed
part the device leg is taken apart: move / first call (lists + attempts) / second call on the cached lists / evaluate."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.graphs import mobile_drop  # noqa: E402


def stats(v):
    return {"median": round(float(np.median(v)) * 1e3, 3), "min": round(float(np.min(v)) * 1e3, 3), "max": round(float(np.max(v)) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=28)
    ap.add_argument("--rho", type=float, default=0.0319)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--step-us", type=float, default=1e6)
    ap.add_argument("--speed", type=float, default=0.1)
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--nattempt", type=int, default=10)
    ap.add_argument("--draws", action="store_true", help="the host / device / fewest legs instead of handle / rebuild")
    a = ap.parse_args()
    if a.draws:
        return draws_legs(a)
    eta, dtype = 0.04, _lib.F32
    np.random.seed(a.seed)
    online.online_sweep(mobile_drop(5, 75e-4, 0), n_points=2, nit=8)  # module load
    drop = mobile_drop(a.cell, a.rho, a.seed)
    t0 = time.perf_counter()
    env, alg, solver, Z, gX = online._setup(drop, a.nit, eta, a.seed, 2, 0, dtype)
    print(json.dumps({"workload": "online-handle", "K": drop.K, "Z": Z, "rank": int(gX.shape[1]), "setup_seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    g_host = np.array(np.asarray(gX))  # the rebuild route hands the factor in from the host (the resident one stays resident)
    rows = []
    for p in range(a.points):
        seed = probe_seed(a.seed, 0, 0x80000 | p)
        order = ("handle", "rebuild") if p % 2 == 0 else ("rebuild", "handle")
        t, res = {}, {}
        for route in order:
            rng = np.random.default_rng(seed)
            t0 = time.perf_counter()
            if route == "handle":
                env.move(drop.sta_locs)
                z_vec, rem = online.round_point(solver, env, Z, gX, a.nattempt, rng)
                _, bler = env.evaluate(z_vec, Z)
            else:
                e2 = online._env(drop, 0)
                s2 = _lib.Solver.from_env(e2, Z, 1, eta, dtype=dtype)
                z = None
                for _ in range(a.nattempt):
                    rv = rng.standard_normal((Z, g_host.shape[1]))
                    rv /= np.linalg.norm(rv, axis=1, keepdims=True)
                    zb, rb = s2.round(Z, g_host, rv[None])
                    z = zb[0]
                    if rb[0] == 0:
                        break
                un = z < 0
                z_vec = z.astype(np.float64)
                if un.any():
                    z_vec[un] = rng.integers(0, Z, int(un.sum()))
                rem = int(un.sum())
                _, bler = e2.evaluate(z_vec, Z)
                s2.close()
                e2.close()
            t[route] = time.perf_counter() - t0
            res[route] = (z_vec, rem, bler)
        same = bool(np.array_equal(res["handle"][0], res["rebuild"][0]) and res["handle"][2].tobytes() == res["rebuild"][2].tobytes())
        # the handle route taken apart (not part of the figures above)
        rv = np.random.default_rng(seed).standard_normal((Z, g_host.shape[1]))
        rv /= np.linalg.norm(rv, axis=1, keepdims=True)
        c0 = time.perf_counter()
        env.move(drop.sta_locs)
        c1 = time.perf_counter()
        solver.round_env(env, Z, gX, rv[None])
        c2 = time.perf_counter()
        solver.round_env(env, Z, gX, rv[None])
        c3 = time.perf_counter()
        env.evaluate(res["handle"][0], Z)
        c4 = time.perf_counter()
        row = {"point": p, "first": order[0], "handle_s": t["handle"], "rebuild_s": t["rebuild"], "same_result": same, "remainder": res["handle"][1],
               "move_s": c1 - c0, "lists_s": (c2 - c1) - (c3 - c2), "round_s": c3 - c2, "evaluate_s": c4 - c3, "mean_bler": float(res["handle"][2].mean())}
        rows.append(row)
        print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        drop.step_time(a.step_us, a.speed, 1e5)
    alg.close()
    env.close()
    keep = rows[1:]
    out = {"workload": "online-handle", "K": drop.K, "Z": Z, "points_kept": len(keep), "unit": "ms", "all_same_result": all(r["same_result"] for r in rows)}
    for k in ("handle_s", "rebuild_s", "move_s", "lists_s", "round_s", "evaluate_s"):
        out[k[:-2]] = stats([r[k] for r in keep])
    out["rebuild_over_handle"] = round(out["rebuild"]["median"] / out["handle"]["median"], 2)
    print(json.dumps(out), flush=True)


def draws_legs(a):
    eta, dtype = 0.04, _lib.F32
    np.random.seed(a.seed)
    online.online_sweep(mobile_drop(5, 75e-4, 0), n_points=2, nit=8, draws="device")  # module load, first launches of the new kernels
    drop = mobile_drop(a.cell, a.rho, a.seed)
    t0 = time.perf_counter()
    env, alg, solver, Z, gX = online._setup(drop, a.nit, eta, a.seed, 2, 0, dtype)
    print(json.dumps({"workload": "online-handle-draws", "K": drop.K, "Z": Z, "rank": int(gX.shape[1]), "nattempt": a.nattempt,
                      "setup_seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    legs = ("host", "device", "fewest")
    rows = []
    for p in range(a.points):
        key = probe_seed(a.seed, 0, 0x80000 | p)
        order = legs[p % 3:] + legs[:p % 3]
        row = {"point": p, "first": order[0]}
        for leg in order:
            t0 = time.perf_counter()
            env.move(drop.sta_locs)
            if leg == "host":
                z_vec, rem = online.round_point(solver, env, Z, gX, a.nattempt, np.random.default_rng(key))
            else:
                z_vec, rem = online.round_point_device(solver, env, Z, gX, a.nattempt, key, pick="first" if leg == "device" else "fewest")
            _, bler = env.evaluate(z_vec, Z)
            row[leg + "_s"] = time.perf_counter() - t0
            row[leg + "_remainder"], row[leg + "_mean_bler"] = rem, float(bler.mean())
        # the device leg taken apart (not part of the figures above)
        c0 = time.perf_counter()
        env.move(drop.sta_locs)
        c1 = time.perf_counter()
        z, rem_all, pick = solver.round_env_attempts(env, Z, gX, a.nattempt, key)
        c2 = time.perf_counter()
        solver.round_env_attempts(env, Z, gX, a.nattempt, key)
        c3 = time.perf_counter()
        env.evaluate(np.where(z < 0, 0, z).astype(np.float64), Z)
        c4 = time.perf_counter()
        row.update({"move_s": c1 - c0, "lists_s": (c2 - c1) - (c3 - c2), "attempts_s": c3 - c2, "evaluate_s": c4 - c3, "pick": pick,
                    "attempts_left_over": [int(r) for r in rem_all]})
        rows.append(row)
        print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        drop.step_time(a.step_us, a.speed, 1e5)
    alg.close()
    env.close()
    keep = rows[1:]
    out = {"workload": "online-handle-draws", "K": drop.K, "Z": Z, "nattempt": a.nattempt, "points_kept": len(keep), "unit": "ms"}
    for k in ("host_s", "device_s", "fewest_s", "move_s", "lists_s", "attempts_s", "evaluate_s"):
        out[k[:-2]] = stats([r[k] for r in keep])
    for leg in legs:
        out[leg + "_share_left_over"] = round(float(np.mean([r[leg + "_remainder"] > 0 for r in keep])), 3)
        out[leg + "_mean_left_over"] = round(float(np.mean([r[leg + "_remainder"] for r in keep])), 3)
        out[leg + "_mean_bler"] = round(float(np.mean([r[leg + "_mean_bler"] for r in keep])), 6)
    out["host_over_device"] = round(out["host"]["median"] / out["device"]["median"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
