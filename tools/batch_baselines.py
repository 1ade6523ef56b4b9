"""Developer tool (GPU box): wall time of the sweeps' baselines (sim_script/journal_version/sim_all_bler.py:42-72: rand_sdp_solver,
MAX_GAIN and MAX_ASSO at each instance's Z), batched against per-instance.

    python tools/batch_baselines.py [--seeds 3] [--reps 7] [--skip-instances]

Workload: the sweep's own instance mix, `journal_geometry(cell, 75e-4, seed)` for cell = 5 .. 15 and seed = 0 .. seeds-1 (K = 75 ..
675); Z per instance: the MAX_GAIN slot count of the state (a bound every method can fill) -- the timing does not depend on the search.
  instances  the paths without the batched calls, per instance: `gm.MAX_GAIN.run(Z, state, order="stable")` and
             `gm.MAX_ASSO.run(Z, state, order="stable")` (a GreedyHandle, a scipy key, one single-wave launch each), and for rand the
             host draw K x 2Z, one `_lib.Solver` of the state and `batch._round` (nattempt x Z x 2Z NumPy normals, `Solver.round`)
  batch      one `BatchSolver.gm` per greedy method, `factor_random` + `round` for rand, for all instances per call
Every repetition is timed with a host clock around calls that end in a device synchronise (every entry copies its results back);
one warm-up repetition of each path first.  One JSON line per (path, method) with the median and the spread over the repetitions, and
one line with the quotients."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib, batch, gm  # noqa: E402
from sig_sdp_mmw_amd.graphs import _state_at, journal_geometry  # noqa: E402

METHODS = ("rand", "mgain", "masso")


def per_instance(states, Zs, seed, nattempt):
    t = {}
    t0 = time.perf_counter()
    for i, st in enumerate(states):
        K, Z = st[0].shape[0], Zs[i]
        gX = np.random.randn(K, 2 * Z)
        gX = gX / np.linalg.norm(gX, axis=1, keepdims=True)
        h = _lib.Solver(Z, st, 1, 0.04, dtype=_lib.F64)
        batch._round(h, Z, gX, st, batch.probe_seed(seed, i, 0x40000), nattempt)
        h.close()
    t["rand"] = time.perf_counter() - t0
    for name, cls in (("mgain", gm.MAX_GAIN), ("masso", gm.MAX_ASSO)):
        t0 = time.perf_counter()
        for i, st in enumerate(states):
            cls.run(Zs[i], st, order="stable")
        t[name] = time.perf_counter() - t0
    return t


def batched(b, Zs, seed, nattempt):
    t = {}
    for m, name in enumerate(METHODS):
        t0 = time.perf_counter()
        batch.baselines_many(b, Zs, methods=(name,), seed=seed, nattempt_round=nattempt)
        t[name] = time.perf_counter() - t0
    return t


def report(path, B, reps):
    out = {}
    for name in METHODS + ("all",):
        v = np.array([sum(r.values()) if name == "all" else r[name] for r in reps])
        out[name] = float(np.median(v))
        print(json.dumps({"workload": "baselines-cells5-15-75e-4", "path": path, "method": name, "instances": B, "repetitions": len(v),
                          "median_seconds": round(out[name], 5), "min_seconds": round(float(v.min()), 5), "max_seconds": round(float(v.max()), 5),
                          "us_per_instance": round(out[name] * 1e6 / B, 1)}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-instances", action="store_true", help="the batch alone (for a kernel trace)")
    a = ap.parse_args()
    seed, nattempt = 0, 10
    states = [_state_at(*journal_geometry(c, 75e-4, s))[0] for c in range(5, 16) for s in range(a.seeds)]
    B = len(states)
    b = _lib.BatchSolver([2] * B, states, 1, 0.04)
    _, ZZ, _ = b.gm(0, 0)
    Zs = [max(2, int(z)) for z in ZZ]
    b.set_slots(Zs, 1)
    # the alternation of section 5: a repetition of one path, then one of the other
    tb, ti = [], []
    for r in range(a.reps + 1):
        x = batched(b, Zs, seed, nattempt)
        y = None if a.skip_instances else per_instance(states, Zs, seed, nattempt)
        if r:  # (the first repetition warms up every shape)
            tb.append(x)
            ti.append(y)
    base = batch.baselines_many(b, Zs, seed=seed, nattempt_round=nattempt)
    b.close()
    mb = report("batch", B, tb)
    print(json.dumps({"workload": "baselines-cells5-15-75e-4", "K_range": [min(s[0].shape[0] for s in states), max(s[0].shape[0] for s in states)],
                      "Z_range": [min(Zs), max(Zs)], "mean_remainder": {m: round(float(np.mean([x[m][2] for x in base])), 3) for m in METHODS}}), flush=True)
    if a.skip_instances:
        return
    mi = report("instances", B, ti)
    q = {m: [round(y[m] / x[m], 2) for x, y in zip(tb, ti)] for m in METHODS}
    q["all"] = [round(sum(y.values()) / sum(x.values()), 2) for x, y in zip(tb, ti)]
    print(json.dumps({"workload": "baselines-cells5-15-75e-4", "instances_over_batch_median": {m: round(mi[m] / mb[m], 2) for m in mb},
                      "instances_over_batch_per_repetition": q}), flush=True)


if __name__ == "__main__":
    main()
