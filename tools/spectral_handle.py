"""Developer tool (GPU box): what `spectral_solve` logs for the spectral baseline on the solver handle, beside the host path it replaces.

    python tools/spectral_handle.py [--workload journal-1pct] [--Z 8,20,40] [--out profiles/spectral_handle.log]

On the benchmark's instance (bench.py's state, N = 10 k) and for every Z and both dtypes, `spectral_sdp_solver(handle=True)` runs
`run_with_state` twice on one cached handle: the first call makes the handle (logged as `spectral_problem_setup`) and its solve fills the
Laplacian's values on the device; the second is the warm figure.  Beside them the same call with `handle=False`, which at this size is
SciPy's `eigsh(tol=1e-5)` on the host -- the path every K > 1024 took before the handle had the baseline.  One JSON line per
(Z, dtype) and per host call: the logged microseconds, and for the handle the call's record (`Solver.spectral_info`).  Figures are
measurements, written down and asserted nowhere."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import spectral_sdp_solver  # noqa: E402


def last_us(alg, key):
    return float(alg.LOGGED_NP_DATA[key][-1, 5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="journal-1pct")
    ap.add_argument("--Z", default="8,20,40")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    _, factory, _, _ = bench.WORKLOADS[args.workload]
    state = bench.make_state(*factory(0))
    K = state[0].shape[0]
    Zs = [int(z) for z in args.Z.split(",")]
    _lib.Solver(8, state, 1, 0.1, dtype=_lib.F32).close()  # the process's first launch loads the code object
    for Z in Zs:
        alg = spectral_sdp_solver(100, 2, 1., handle=False)
        ok, blk = alg.run_with_state(0, Z, state)
        say({"workload": args.workload, "K": K, "Z": Z, "path": "host eigsh(tol=1e-5)", "setup_us": round(last_us(alg, "spectral_problem_setup")),
             "solve_us": round(last_us(alg, "spectral_solve")), "finite": bool(np.all(np.isfinite(blk)))})
        for name, dt in (("f32", _lib.F32), ("f64", _lib.F64)):
            alg = spectral_sdp_solver(100, 2, 1., handle=True)
            alg._dtype_code = dt
            rec = {"workload": args.workload, "K": K, "Z": Z, "path": "handle", "dtype": name}
            for call in ("first", "warm"):
                blk = None  # (a resident block somebody still holds is copied out before the next call overwrites it)
                ok, blk = alg.run_with_state(0, Z, state)
                rec["setup_us_" + call] = round(last_us(alg, "spectral_problem_setup"))
                rec["solve_us_" + call] = round(last_us(alg, "spectral_solve"))
            s = alg._dev[2]
            rec["info"] = s.spectral_info()
            rec["spmm_kind"] = int(s.read(_lib.F_SPMM_KIND, 2)[0])
            rec["rows_below_1e-3"] = int(np.sum(s.factor_row_norms() < 1e-3))
            say(rec)
            alg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
