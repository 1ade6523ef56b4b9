"""Developer tool (GPU box): a whole lockstep bisection (`batch.search_many`, nit 150) on sweep batches, end to end, with the probe
epilogue on handles (export + mmw_factor + mmw_round per instance) against the epilogue inside the batch (one mmw_batch_factor and
one mmw_batch_round per round of probes, csrc/kernels_batch_epilogue.h).

    python tools/batch_search.py [--sizes 64,256] [--nit 150] [--runs 3] [--epilogues handle,batch] [--factor-split auto|N]

Workload: tools/batch_small.py's `sweep(n)` (journal_graph(cell, 75e-4, seed), cells 5..15, K = 75 ... 675).  One JSON line per run:
wall seconds of the search and, per round of probes, the instances probing and the seconds in `iterate` and in the epilogue.
--factor-split adds runs of epilogue="batch" with that `factor_split` (csrc/kernels_batch_factor_split.h) after the others; every line
carries its `factor_split` and the `factor_call()` of its first round."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_small import sweep  # noqa: E402
from sig_sdp_mmw_amd import batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epilogues", default="handle,batch")
    ap.add_argument("--factor-split", default=None, help="auto or an int: further runs of epilogue=batch with this factor_split")
    a = ap.parse_args()
    legs = [(ep, None) for ep in a.epilogues.split(",") if ep]
    if a.factor_split is not None:
        legs.append(("batch", "auto" if a.factor_split == "auto" else int(a.factor_split)))
    s0, _ = sweep(2)
    for ep, fs in legs:
        batch.search_many(s0, nit=2, epilogue=ep, factor_split=fs)  # module load, first launches
    for B in [int(x) for x in a.sizes.split(",") if x]:
        states, _ = sweep(B)
        K = [st[0].shape[0] for st in states]
        for ep, fs in legs:
            for run in range(a.runs):
                rounds = []
                t0 = time.perf_counter()
                res = batch.search_many(states, nit=a.nit, eta=0.04, seed=run, epilogue=ep, timings=rounds, factor_split=fs)
                t = time.perf_counter() - t0
                print(json.dumps({"workload": "journal-sweep-75e-4", "epilogue": ep, "factor_split": fs, "factor_call": rounds[0]["factor_call"], "instances": B, "nit": a.nit, "run": run,
                                  "K_range": [int(min(K)), int(max(K))], "seconds": round(t, 4), "rounds": len(rounds),
                                  "iterate_s": round(sum(r["iterate_s"] for r in rounds), 4),
                                  "epilogue_s": round(sum(r["epilogue_s"] for r in rounds), 4),
                                  "Z_sum": int(sum(r["Z"] for r in res)),
                                  "per_round": [[r["probes"], round(r["iterate_s"], 4), round(r["epilogue_s"], 4)] for r in rounds]}),
                      flush=True)


if __name__ == "__main__":
    main()
