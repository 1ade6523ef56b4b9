"""Developer tool (GPU box): wall time of gm.MAX_RAND with its draws on the host against its draws on the device, and of the batched
form against the per-instance path.

    python tools/gm_rand.py [--reps 7] [--seeds 3] [--skip-large] [--device 0]

  large      journal_graph(28, 0.0319) (K = 10 003) at Z = 186: `gm.MAX_RAND.run(Z, state)` with draws="host" -- the path as it was:
             randn(Z, K) and randn(K) from NumPy, K argsorts of Z values, a K x Z int32 upload, mmw_gm_assign -- and with
             draws="device" (mmw_gm_rand: nothing drawn or sorted on the host, nothing uploaded); the same handle serves both, built
             before the clock starts.  The host path's parts (draw, sorts, assign) are timed apart once.
  batch      the sweep's instance mix, `journal_geometry(cell, 75e-4, seed)` for cell = 5 .. 15 (K = 75 .. 675), Z per instance the
             MAX_GAIN slot count of the state: one `BatchSolver.gm_rand` for all against one `GreedyHandle.rand` per instance (handles
             built before the clock starts) and against `gm.MAX_RAND.run(draws="host")` per instance (its handle cache holds one
             state, so every call rebuilds the handle: the cost a sweep pays today).
Every repetition is timed with a host clock around calls that end in a device synchronise (every entry copies its results back), the
paths alternating within a repetition; one warm-up repetition first.  One JSON line per measurement."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib, gm  # noqa: E402
from sig_sdp_mmw_amd.graphs import _state_at, journal_geometry, journal_graph  # noqa: E402


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):  # (MAX_RAND prints the fill of users left over, as the reference does)
        return fn()


def line(what, path, ts, **more):
    v = np.array(ts)
    rec = {"workload": what, "path": path, "repetitions": len(v), "median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(float(v.min()) * 1e3, 3),
           "max_ms": round(float(v.max()) * 1e3, 3)}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return float(np.median(v))


def large(reps):
    st = journal_graph(28, 0.0319, seed=1)
    K, Z = st[0].shape[0], 186
    np.random.seed(0)
    th, td = [], []
    rem = {}
    for r in range(reps + 1):
        for path, ts in (("host", th), ("device", td)):
            t0 = time.perf_counter()
            out = quiet(lambda: gm.MAX_RAND.run(Z, st, draws=path))
            if r:
                ts.append(time.perf_counter() - t0)
            rem[path] = int(out[2])
    mh = line("max_rand-journal-1pct-Z186", "draws=host", th, K=K, Z=Z, remainder=rem["host"])
    md = line("max_rand-journal-1pct-Z186", "draws=device", td, K=K, Z=Z, remainder=rem["device"])
    g = gm._handle(st)
    t0 = time.perf_counter()
    inprod = np.random.randn(Z, K)
    key = np.random.randn(K)
    t1 = time.perf_counter()
    pref = np.ascontiguousarray(np.argsort(-inprod, axis=0).T)
    rank = np.argsort(key)
    t2 = time.perf_counter()
    g.assign(rank, pref)
    t3 = time.perf_counter()
    print(json.dumps({"workload": "max_rand-journal-1pct-Z186", "host_path_parts_ms": {"randn": round((t1 - t0) * 1e3, 3), "argsort": round((t2 - t1) * 1e3, 3),
                                                                                      "assign_with_upload": round((t3 - t2) * 1e3, 3)},
                      "host_over_device": round(mh / md, 2)}), flush=True)


def small(reps, seeds, device):
    states = [_state_at(*journal_geometry(c, 75e-4, s))[0] for c in range(5, 16) for s in range(seeds)]
    B = len(states)
    b = _lib.BatchSolver([2] * B, states, 1, 0.04, device=device)
    _, ZZ, _ = b.gm(0, 0)
    Zs = [max(2, int(z)) for z in ZZ]
    keys = np.arange(1, B + 1, dtype=np.uint64)
    handles = [_lib.GreedyHandle(st, device=device) for st in states]
    tb, th, tr = [], [], []
    np.random.seed(0)
    for r in range(reps + 1):
        t0 = time.perf_counter()
        z, rem, _ = b.gm_rand(Zs, keys, 1)
        t1 = time.perf_counter()
        one = [h.rand(Zs[i], 1, int(keys[i])) for i, h in enumerate(handles)]
        t2 = time.perf_counter()
        quiet(lambda: [gm.MAX_RAND.run(Zs[i], st) for i, st in enumerate(states)])
        t3 = time.perf_counter()
        assert all(np.array_equal(z[i][0], one[i][0]) for i in range(B))
        if r:
            tb.append(t1 - t0)
            th.append(t2 - t1)
            tr.append(t3 - t2)
    what = "max_rand-cells5-15-75e-4"
    more = dict(instances=B, K_range=[min(s[0].shape[0] for s in states), max(s[0].shape[0] for s in states)], Z_range=[min(Zs), max(Zs)])
    mb = line(what, "batch gm_rand, one launch", tb, **more)
    mh = line(what, "GreedyHandle.rand per instance, handles kept", th, **more)
    mr = line(what, "gm.MAX_RAND.run(draws=host) per instance", tr, **more)
    print(json.dumps({"workload": what, "handles_over_batch": round(mh / mb, 2), "host_path_over_batch": round(mr / mb, 2),
                      "us_per_instance": {"batch": round(mb * 1e6 / B, 1), "handles": round(mh * 1e6 / B, 1), "host_path": round(mr * 1e6 / B, 1)}}), flush=True)
    for h in handles:
        h.close()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--device", type=int, default=0, help="-1: the host forms (a dry run)")
    a = ap.parse_args()
    gm.DEVICE = a.device
    if not a.skip_large:
        large(a.reps)
    small(a.reps, a.seeds, a.device)


if __name__ == "__main__":
    main()
