"""Developer tool (GPU box): a whole lockstep bisection (`batch.search_many`, nit 150) on sweep batches, end to end, with the probe
epilogue on handles (export + mmw_factor + mmw_round per instance) against the epilogue inside the batch (one mmw_batch_factor and
one mmw_batch_round per round of probes, csrc/kernels_batch_epilogue.h).

    python tools/batch_search.py [--sizes 64,256] [--nit 150] [--runs 3] [--epilogues handle,batch] [--factor-split auto|N] [--warm]
                                 [--root DIR --tag NAME]

Workload: tools/batch_small.py's `sweep(n)` (journal_graph(cell, 75e-4, seed), cells 5..15, K = 75 ... 675).  One JSON line per run:
wall seconds of the search and, per round of probes, the instances probing and the seconds in the slot change, in `iterate` and in
the epilogue.  --factor-split adds runs of epilogue="batch" with that `factor_split` (csrc/kernels_batch_factor_split.h) after the
others; every line carries its `factor_split` and the `factor_call()` of its first round.  --warm adds, per epilogue, a leg with
`warm_start=True` (opt-in, not the reference's search: later rounds continue from the previous probe and run a third of the
iterations); every line carries "warm" and the Z every instance ended at, so that two legs can be compared instance by instance.

`set_slots_s` is measured here, around `BatchSolver.set_slots`, so that it is there for every version of the package: --root DIR
imports `sig_sdp_mmw_amd` from another checkout of this project (with its library built), e.g. the commit before a change."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epilogues", default="handle,batch")
    ap.add_argument("--factor-split", default=None, help="auto or an int: further runs of epilogue=batch with this factor_split")
    ap.add_argument("--warm", action="store_true", help="a further leg per epilogue with warm_start=True")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout to import sig_sdp_mmw_amd from (default: this one)")
    ap.add_argument("--tag", default="", help="a name for the checkout measured, copied into every line")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.abspath(a.root))
    from sig_sdp_mmw_amd import _lib, batch  # before batch_small, which puts this checkout in front: the package is loaded by then
    from batch_small import sweep

    slot_s = []  # seconds of every set_slots call since the last clear
    inner = _lib.BatchSolver.set_slots

    def timed_set_slots(self, *args, **kw):
        t = time.perf_counter()
        try:
            return inner(self, *args, **kw)
        finally:
            slot_s.append(time.perf_counter() - t)
    _lib.BatchSolver.set_slots = timed_set_slots

    legs = [(ep, None, False) for ep in a.epilogues.split(",") if ep]
    if a.factor_split is not None:
        legs.append(("batch", "auto" if a.factor_split == "auto" else int(a.factor_split), False))
    if a.warm:
        legs += [(ep, None, True) for ep in a.epilogues.split(",") if ep]

    def search(states, ep, fs, warm, **kw):
        extra = {"warm_start": True} if warm else {}  # (a checkout from before the warm start takes no such argument)
        return batch.search_many(states, epilogue=ep, factor_split=fs, **extra, **kw)
    s0, _ = sweep(2)
    for ep, fs, warm in legs:
        search(s0, ep, fs, warm, nit=3)  # module load, first launches
    for B in [int(x) for x in a.sizes.split(",") if x]:
        states, _ = sweep(B)
        K = [st[0].shape[0] for st in states]
        for ep, fs, warm in legs:
            for run in range(a.runs):
                rounds = []
                del slot_s[:]
                t0 = time.perf_counter()
                res = search(states, ep, fs, warm, nit=a.nit, eta=0.04, seed=run, timings=rounds)
                t = time.perf_counter() - t0
                print(json.dumps({"workload": "journal-sweep-75e-4", "tag": a.tag,"epilogue": ep, "warm": warm, "factor_split": fs,
                                  "factor_call": rounds[0]["factor_call"], "instances": B, "nit": a.nit, "run": run,
                                  "K_range": [int(min(K)), int(max(K))], "seconds": round(t, 4), "rounds": len(rounds),
                                  "set_slots_s": round(sum(slot_s), 4),
                                  "iterate_s": round(sum(r["iterate_s"] for r in rounds), 4),
                                  "epilogue_s": round(sum(r["epilogue_s"] for r in rounds), 4),
                                  "Z_sum": int(sum(r["Z"] for r in res)),
                                  "per_round": [[r["probes"], round(r["iterate_s"], 4), round(r["epilogue_s"], 4), round(s, 4)] for r, s in zip(rounds, slot_s)],
                                  "Z": [int(r["Z"]) for r in res]}),
                      flush=True)


if __name__ == "__main__":
    main()
