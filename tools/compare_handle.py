"""Developer tool (GPU box): the five-method comparison on the solver handle (`online.compare`) and its random-embedding arm by both
routes, on the benchmark instance.

    python tools/compare_handle.py [--cell 28] [--rho 0.0319] [--seed 0] [--reps 5] [--nit 150] [--nattempt 10] [--out profiles/compare_handle.log]

Workload: `mobile_drop(28, 0.0319, seed)` (N = 10 003), fp32 handle, Z from the cold search as `online.compare` runs it.

The `rand` arm, `reps` times, the two legs alternating in one session on ONE handle (the search's):
  host    today's default route: `rand_sdp_solver().run_with_state` draws K x 2Z normals with NumPy and normalises them (draw_s);
          `rounding` scales them (`index_ordered`) and every attempt draws its directions on the host and uploads the block again
          (round_s).  transfer_s: one attempt's `Solver.round` with the block handed in from the host minus the same call on a
          resident block of the same shape -- the upload an attempt pays.
  device  `rand_sdp_solver(draws="device")`: `Solver.factor_random(2Z, key, resident, index-ordered)` to the end of the device's work
          (draw_s), nothing to transfer, then ONE `Solver.round_attempts` call (round_s).
The colourings differ between the legs because the draws do; each line gives the users left over.

The whole `online.compare` with all five methods, `reps` times: search_s, every arm's seconds, evaluate_s.

One JSON line per repetition and leg, then the medians with min - max.  Figures are measurements, written down and asserted nowhere."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib, batch, online  # noqa: E402
from sig_sdp_mmw_amd.graphs import mobile_drop  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver  # noqa: E402


def stats(v):
    return {"median": round(float(np.median(v)) * 1e3, 3), "min": round(float(np.min(v)) * 1e3, 3), "max": round(float(np.max(v)) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=28)
    ap.add_argument("--rho", type=float, default=0.0319)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--nattempt", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    eta, dtype, rr = 0.04, _lib.F32, 2
    np.random.seed(a.seed)
    online.compare(mobile_drop(5, 75e-4, 0), nit=8, methods=batch.METHODS + batch.OPT_IN_METHODS)  # module load, first launches
    drop = mobile_drop(a.cell, a.rho, a.seed)

    # ---- the rand arm by both routes, on the search's handle
    env = online._env(drop, 0)
    state = env.device_state()
    t0 = time.perf_counter()
    alg, _, Z, _, probes = online._search(state, a.nit, eta, a.seed, rr, 0, dtype)
    solver = alg._device_solver(Z, state)
    say({"workload": "compare-handle", "K": drop.K, "Z": Z, "cols": rr * Z, "probes": probes, "nattempt": a.nattempt, "search_seconds": round(time.perf_counter() - t0, 3)})
    legs = {"host": rand_sdp_solver(a.nit, rr), "device": rand_sdp_solver(a.nit, rr, draws="device", seed=a.seed)}
    legs["device"].round_draws = "device"
    for leg in legs.values():
        leg._dev = (None, state, solver)  # the handle the search made, for both legs (closed once, below)
    rows = {"host": [], "device": []}
    transfer = []
    for r in range(a.reps + 1):  # repetition 0 is thrown away (first launches, first allocations)
        for name in (("host", "device") if r % 2 == 0 else ("device", "host")):
            leg = legs[name]
            solver.sync()
            t0 = time.perf_counter()
            _, gX = leg.run_with_state(0, Z, state)
            if name == "device":
                solver.sync()
            t1 = time.perf_counter()
            z_vec, _, rem = leg.rounding(Z, gX, state, nattempt=a.nattempt)
            t2 = time.perf_counter()
            _, bler = env.evaluate(z_vec, Z)
            rec = {"rep": r, "leg": name, "draw_s": round(t1 - t0, 6), "round_s": round(t2 - t1, 6), "remainder": int(rem), "mean_bler": round(float(np.mean(bler)), 6)}
            if name == "host":  # what one attempt pays for handing the block in
                g = rand_sdp_solver.index_ordered(gX)
                rv = solver.round_randv(Z, rr * Z, 1, 0)[None]
                ta = time.perf_counter()
                solver.round(Z, g, rv)
                tb = time.perf_counter()
                df = solver.factor_random(rr * Z, 1, resident=True, index_order=True)
                solver.sync()
                tc = time.perf_counter()
                solver.round(Z, df, rv)
                td = time.perf_counter()
                del df  # (a held resident block would be copied out by the next factor call, inside that leg's draw_s)
                rec["transfer_s"] = round((tb - ta) - (td - tc), 6)
            say(rec)
            if r > 0:
                rows[name].append(rec)
                if name == "host":
                    transfer.append(rec["transfer_s"])
    legs["host"]._dev = legs["device"]._dev = None
    alg.close()
    env.close()
    summary = {"workload": "compare-handle", "part": "rand arm", "K": drop.K, "Z": Z, "reps_kept": a.reps, "unit": "ms"}
    for name in rows:
        summary[name] = {"draw": stats([x["draw_s"] for x in rows[name]]), "round": stats([x["round_s"] for x in rows[name]]),
                         "total": stats([x["draw_s"] + x["round_s"] for x in rows[name]]),
                         "mean_left_over": round(float(np.mean([x["remainder"] for x in rows[name]])), 2)}
    summary["host"]["transfer_per_attempt"] = stats(transfer)
    say(summary)

    # ---- the whole comparison
    names = batch.METHODS + batch.OPT_IN_METHODS
    runs = []
    for r in range(a.reps + 1):
        t = {}
        np.random.seed(a.seed)
        t0 = time.perf_counter()
        res = online.compare(drop, nit=a.nit, eta=eta, seed=a.seed, nattempt=a.nattempt, rank_radio=rr, dtype=dtype, methods=names, timings=t)
        rec = {"rep": r, "leg": "compare", "Z": res["Z"], "total_s": round(time.perf_counter() - t0, 6), "search_s": round(t["search_s"], 6),
               "baselines_s": round(t["baselines_s"], 6), "evaluate_s": round(t["evaluate_s"], 6), "arm_s": {k: round(v, 6) for k, v in t["arm_s"].items()},
               "remainder": res["remainder"], "mean_bler": {k: round(float(np.mean(v)), 6) for k, v in res["bler"].items()}}
        say(rec)
        if r > 0:
            runs.append(rec)
    summary = {"workload": "compare-handle", "part": "whole compare", "K": drop.K, "Z": runs[0]["Z"], "reps_kept": a.reps, "unit": "ms",
               "total": stats([x["total_s"] for x in runs]), "search": stats([x["search_s"] for x in runs]), "evaluate": stats([x["evaluate_s"] for x in runs])}
    for m in names:
        summary[m] = stats([x["arm_s"][m] for x in runs])
    say(summary)


if __name__ == "__main__":
    main()
