#!/usr/bin/env python3
"""Wall-clock of the greedy baselines (sig_sdp_mmw_amd.gm: MAX_GAIN / MAX_ASSO, not_Z_bound) on journal states, both visiting
orders, beside the O(deg) CPU restatement of the tests (tests/helpers/gm_restate.py) on the same state.

Median of 5 calls after one warm-up call (the restatement: one call).  Prints one JSON line per (state, algorithm).

    python tools/gm_timing.py [--sizes 675,1875,10003] [--device 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "helpers")]

import gm_restate as R  # noqa: E402
from sig_sdp_mmw_amd import gm  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph  # noqa: E402

STATES = {675: (15, 75e-4), 1875: (25, 75e-4), 10003: (28, 0.0319)}  # K: (cell_size, station density); 10 003 = journal-1pct


def median_time(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="675,1875,10003")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    gm.DEVICE = a.device
    for K in [int(x) for x in a.sizes.split(",")]:
        cs, rho = STATES[K]
        st = journal_graph(cs, rho, seed=1)
        assert st[0].shape[0] == K, st[0].shape
        for name, cls, kf in (("MAX_GAIN", gm.MAX_GAIN, R.gain_key), ("MAX_ASSO", gm.MAX_ASSO, R.asso_key)):
            rec = {"K": K, "alg": name}
            for order in ("reference", "stable"):
                np.random.seed(0)
                _, ZZ, rem = cls.run(-1, st, not_Z_bound=True, order=order)
                rec[order + "_s"] = median_time(lambda: cls.run(-1, st, not_Z_bound=True, order=order))
                rec[order + "_ZZ"] = int(ZZ)
            if not a.no_restatement:
                t0 = time.perf_counter()
                _, ZZr, _, _ = R.slot_major(kf(st), -1, st, 1, True)
                rec["restatement_s"] = time.perf_counter() - t0
                rec["restatement_ZZ"] = int(ZZr)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
