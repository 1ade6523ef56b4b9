"""Developer tool (GPU box): what building the solver handle on the device from a CSR state costs against building it on the host.

    python tools/create_from_csr.py [--workloads er-5pct-2k,er-1pct,er-50k,journal-1pct] [--reps 5] [--out profiles/create_from_csr.log]

Per workload (bench.py's states, each at its bench Z and dtype), three things are timed:
  host    Solver(Z, state, ...)                 mmw_create: the single-threaded pattern build on the host, uploads, blocking
  device  Solver.from_csr(csr, Z, ...)          mmw_create_from_csr: the pattern by kernels from the arrays already on the device
  upload  DeviceCSR.upload(state)               the seven arrays to the device, once per state (not part of `device`)
The host leg includes the wrapper's look at the scipy matrices (`_lib._state_arrays`: no copy for canonical int32 / float64 CSR), as any
caller of Solver pays it; the device leg starts from the DeviceCSR.
The process is warmed by one throwaway handle first (the first launch loads the code object, which mmw_create hides under its host
build); then the two legs alternate, `--reps` repetitions, and the median and the spread (min .. max) are reported, one JSON line per
workload.  The locality blocking is built on the host in BOTH legs: with MMW_VERBOSE=1 the library's `[create]` line (stderr) gives
its share.  Every handle is closed before the next is made."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    h = fn()
    t = time.perf_counter() - t0
    h.close()
    return t


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="er-5pct-2k,er-1pct,er-50k,journal-1pct")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    warmed = False
    for name in args.workloads.split(","):
        _, factory, Z, dtype = bench.WORKLOADS[name]
        state = bench.make_state(*factory(0))
        if Z is None:
            Z = bench.first_midpoint(state)
        dt = _lib.F32 if dtype == "f32" else _lib.F64
        K, arrs = _lib._state_arrays(state)
        if not warmed:
            _lib.Solver(Z, state, args.nit, 0.04, dtype=dt).close()
            warmed = True
        t_up, t_host, t_dev = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            csr = _lib.DeviceCSR.upload_arrays(K, arrs)
            t_up.append(time.perf_counter() - t0)
            t_host.append(timed(lambda: _lib.Solver(Z, state, args.nit, 0.04, dtype=dt)))
            t_dev.append(timed(lambda: _lib.Solver.from_csr(csr, Z, args.nit, 0.04, dtype=dt)))
            csr.close()
        h = _lib.Solver(Z, state, args.nit, 0.04, dtype=dt)
        say({"workload": name, "K": K, "Z": int(Z), "dtype": dtype, "nnzS": int(arrs[1].size), "nnzL": h.nnzL, "reps": args.reps, "host": stats(t_host),
             "device": stats(t_dev), "upload": stats(t_up), "device_over_host": round(statistics.median(t_dev) / statistics.median(t_host), 3)})
        h.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
