#!/usr/bin/env python3
"""Generate tests/golden/spectral.npz: the reference's spectral_sdp_solver.run_with_state (sim_src/alg/sdp_solver.py:165-185) on
journal states.

Runs only where the reference checkout is available; the fixture it writes is committed.  The reference is imported the way
make_golden_gm.py does it (empty stand-ins for cvxpy and line_profiler, which sim_src.alg.sdp_solver imports at its top and the
spectral class never uses); nothing of it is copied.

The states are `journal_graph(cell, 75e-4, seed)` of this repository for (cell, seed) = (3, 0), (5, 1), (8, 0): K = 27, 75, 192.  The
fixture does not carry them: the tests rebuild them and check K, the stored entries and the sum of S_gain's data against the record.
Recorded per case (state, Z): the K x Z block the reference returns and its measured distance to the dense restatement
(tests/helpers/spectral_oracle.py) -- the largest entry of N N^T - M M^T over the users whose un-normalised row has norm >= 1e-3, and
how many users those are.  eigsh's start vector is not pinned (ARPACK draws it), so that distance is a property of this file and
is asserted against the file, not against a fresh run.

Usage:  python tests/golden/make_golden_spectral.py   (from the repo root)
"""
import os
import sys
import types

import numpy as np
import scipy

REF = os.environ.get("MMW_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
sys.modules.setdefault("cvxpy", types.ModuleType("cvxpy"))
_lp = types.ModuleType("line_profiler")
_lp.LineProfiler = object
sys.modules.setdefault("line_profiler", _lp)

from sim_src.alg.sdp_solver import spectral_sdp_solver  # noqa: E402  (the reference)

import spectral_oracle as SO  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph  # noqa: E402

META = "reference zhouyou-gu/sig-sdp-mmw sdp_solver.py @ numpy %s / scipy %s" % (np.__version__, scipy.__version__)
STATES = [("c3s0", 3, 0, (3, 8, 20)), ("c5s1", 5, 1, (5, 12, 20)), ("c8s0", 8, 0, (5, 12, 20))]


def main():
    out = {"meta": np.array(META)}
    cases = []
    for name, cell, seed, Zs in STATES:
        state = journal_graph(cell, 75e-4, seed)
        S = state[0]
        out[name + "/K"] = np.array(S.shape[0])
        out[name + "/nnz"] = np.array(S.nnz)
        out[name + "/data_sum"] = np.array(float(S.data.sum()))
        dense = SO.Dense(S)
        for Z in Zs:
            alg = spectral_sdp_solver()
            ok, blk = alg.run_with_state(0, Z, state)
            assert ok and blk.shape == (S.shape[0], Z)
            assert sorted(alg.LOGGED_NP_DATA) == ["spectral_problem_setup", "spectral_solve"]
            V = dense.top(Z)[1]
            rows = SO.big_rows(V)
            dist = SO.gram_distance(np.asarray(blk), SO.normalise_rows(V), rows)
            cname = "%s/z%d" % (name, Z)
            out[cname + "/block"] = np.asarray(blk, dtype=np.float64)
            out[cname + "/gram_distance"] = np.array(dist)
            out[cname + "/rows_compared"] = np.array(int(rows.sum()))
            out[cname + "/relgap"] = np.array(dense.relgap(Z))
            cases.append(cname)
            print("%-10s K %3d Z %2d: %3d of %3d users compared, Gram distance to the dense restatement %.3e, relgap %.3e"
                  % (cname, S.shape[0], Z, int(rows.sum()), S.shape[0], dist, dense.relgap(Z)))
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "spectral.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
