"""Developer tool (GPU box): what the batch's split modes (BatchSolver.set_split, csrc/kernels_batch_split.h; BatchSolver.set_row_split,
csrc/kernels_batch_rows.h; BatchSolver.set_head_split, csrc/kernels_batch_head.h) buy, fp64, device sketches, default expm tolerance (1e-9).

    python tools/batch_split.py [--legs a,b,c,d,e] [--row-split] [--head-split] [--nit 150] [--er-nit 30] [--runs 3] [--limit 240] [--cus 256]

Legs, `--runs` rounds with the legs alternating inside a round, every run under its own time limit (the process ends if a run
overruns it), one JSON line per run (with MMW_F_SPLIT_CALL's launches and idle launches of the run's one iterate call):
  a  the 64-instance journal sweep (tools/batch_small.py's, K 75 ... 675), single-launch kernel
  b  the same sweep with set_split("auto")
  c  the same sweep on handles, 8 streams (tools/batch_small.py's leg)
  d  one K = 675 instance at parts 1, 4, 8, 16: ms per iteration
  e  er-5pct-2k x 8 (K 2 000, D 64) single launch and at the auto split (report only: D = 64 caps it at 8 slices)
--row-split adds
  r  the sweep with set_split("auto") and set_row_split("auto")
  s  the K = 675 instance at rows 1, 2, 4, 8 x parts "auto"
  f  er-5pct-2k x 8 at rows 8, 16, 32 x parts 8
  h  er-5pct-2k x 8 on handles, 8 streams: f's comparator
--head-split adds (with MMW_F_HEAD_CALL's record in every line), each beside the leg it extends:
  bh       the sweep with set_split("auto") and set_head_split("auto")                      beside b
  sh       the K = 675 instance at rows 8 x parts "auto" with set_head_split("auto")        beside s8
  fh8 ...  er-5pct-2k x 8 at rows 16 x parts 8 with set_head_split(8), (16), (32)           beside f16 and h
and summary lines: median(b) and median(r) against min(a) -- the bar -- and against median(c); median(f*) against min(h);
median(bh) against min(b), median(sh) against min(s8), median(fh*) against min(f16)."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batch_small import run_handles, sweep  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import er_contention_graph  # noqa: E402


def run(states, Zs, nit, split, cus, eta=0.04, rows=None, info=None, head=None):
    b = _lib.BatchSolver(Zs, states, nit, eta)
    if split is not None:
        b.set_split(split, cus) if split == "auto" else b.set_split(split)
    if rows is not None:
        b.set_row_split(rows, cus) if rows == "auto" else b.set_row_split(rows)
    if head is not None:
        b.set_head_split(head, cus) if head == "auto" else b.set_head_split(head)
    parts = b.split_parts
    t0 = time.perf_counter()
    b.iterate(nit, None, np.arange(len(states), dtype=np.uint64) + 1)
    t = time.perf_counter() - t0
    if info is not None:
        call = b.split_call()
        rp = b.row_split_parts
        info.update(launches_per_iteration=round(call["launches"] / nit, 2), idle_share=round(call["idle"] / max(1, call["launches"]), 4),
                    widest=call["widest"], max_rows=int(max(rp)) if rp else 1)
        if head is not None:
            hp = b.head_split_parts
            info.update(head_call=b.head_call(), max_head=int(max(hp)) if hp else 1)
    b.close()
    return t, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--nit", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--er-nit", type=int, default=30)
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--row-split", action="store_true", help="add the row-split legs r, s, f, h")
    ap.add_argument("--head-split", action="store_true", help="add the head-split legs bh, sh, fh8, fh16, fh32 and the legs they stand beside (b, s8, f16, h)")
    a = ap.parse_args()
    legs = [x for x in a.legs.split(",") if x] + (["r", "s", "f", "h"] if a.row_split else [])
    if a.head_split:
        legs += [x for x in ("b", "s8", "f16", "h", "bh", "sh", "fh") if x not in legs]
    s0, z0 = sweep(2)
    run(s0, z0, 2, None, a.cus)
    run(s0, z0, 2, 2, a.cus)  # module load, first launches
    states, Zs = sweep(a.instances)
    B = len(states)
    times = {}

    todo = []

    def leg(name, fn, **extra):
        todo.append((name, fn, extra))

    def batch_leg(split):
        def fn():
            t, parts = run(states, Zs, a.nit, split, a.cus)
            return t, {"instances": B, "nit": a.nit, "instances_per_s": round(B / t, 2),
                       "workgroups": int(sum(parts)) if parts else B, "max_parts": int(max(parts)) if parts else 1}
        return fn
    if "a" in legs:
        leg("a", batch_leg(None), path="batch")
    if "b" in legs:
        leg("b", batch_leg("auto"), path="batch-split-auto")
    if "c" in legs:
        leg("c", lambda: (run_handles(states, Zs, a.nit), {"instances": B, "nit": a.nit}), path="handles-8-streams")
    if "d" in legs:
        i675 = max(range(B), key=lambda i: states[i][0].shape[0])
        for parts in (1, 4, 8, 16):
            def fn(parts=parts):
                t, _ = run([states[i675]], [Zs[i675]], a.nit, parts, a.cus)
                return t, {"K": int(states[i675][0].shape[0]), "Z": int(Zs[i675]), "ms_per_iteration": round(t * 1e3 / a.nit, 4)}
            leg("d%d" % parts, fn, path="one-instance", parts=parts)
    if "e" in legs:
        er = [er_contention_graph(2000, 0.05, seed=100 + i) for i in range(8)]
        for split in (None, "auto"):
            def fn(split=split):
                t, parts = run(er, [32] * 8, a.er_nit, split, a.cus)
                return t, {"instances": 8, "nit": a.er_nit, "instances_per_s": round(8 / t, 2), "max_parts": int(max(parts)) if parts else 1}
            leg("e-" + ("auto" if split else "single"), fn, path="er-5pct-2k-x8")
    rows_of = {}
    if "r" in legs:
        def fn_r():
            more = {}
            t, parts = run(states, Zs, a.nit, "auto", a.cus, rows="auto", info=more)
            return t, {"instances": B, "nit": a.nit, "instances_per_s": round(B / t, 2), "max_parts": int(max(parts)) if parts else 1, **more}
        leg("r", fn_r, path="batch-split-auto-rows-auto")
    if "bh" in legs:
        def fn_bh():
            more = {}
            t, parts = run(states, Zs, a.nit, "auto", a.cus, info=more, head="auto")
            return t, {"instances": B, "nit": a.nit, "instances_per_s": round(B / t, 2), "max_parts": int(max(parts)) if parts else 1, **more}
        leg("bh", fn_bh, path="batch-split-auto-head-auto")
    if "s" in legs or "s8" in legs or "sh" in legs:
        i675 = max(range(B), key=lambda i: states[i][0].shape[0])
        for rows in (1, 2, 4, 8):
            if "s" not in legs and "s%d" % rows not in legs:
                continue

            def fn(rows=rows):
                more = {}
                t, parts = run([states[i675]], [Zs[i675]], a.nit, "auto", a.cus, rows=rows, info=more)
                return t, {"K": int(states[i675][0].shape[0]), "Z": int(Zs[i675]), "ms_per_iteration": round(t * 1e3 / a.nit, 4),
                           "parts": int(max(parts)) if parts else 1, **more}
            leg("s%d" % rows, fn, path="one-instance-rows", rows=rows)
        if "sh" in legs:
            def fn_sh():
                more = {}
                t, parts = run([states[i675]], [Zs[i675]], a.nit, "auto", a.cus, rows=8, info=more, head="auto")
                return t, {"K": int(states[i675][0].shape[0]), "Z": int(Zs[i675]), "ms_per_iteration": round(t * 1e3 / a.nit, 4),
                           "parts": int(max(parts)) if parts else 1, **more}
            leg("sh", fn_sh, path="one-instance-rows-head-auto", rows=8)
    if "f" in legs or "h" in legs or "fh" in legs or any(x[:1] == "f" and x.lstrip("fh").isdigit() for x in legs):
        er = [er_contention_graph(2000, 0.05, seed=100 + i) for i in range(8)]
        for rows in (8, 16, 32):
            if "f" not in legs and "f%d" % rows not in legs:
                continue

            def fn(rows=rows):
                more = {}
                t, _ = run(er, [32] * 8, a.er_nit, 8, a.cus, rows=rows, info=more)
                return t, {"instances": 8, "nit": a.er_nit, "instances_per_s": round(8 / t, 2), **more}
            leg("f%d" % rows, fn, path="er-5pct-2k-x8-rows", rows=rows, parts=8)
        for head in (8, 16, 32):
            if "fh" not in legs and "fh%d" % head not in legs:
                continue

            def fn(head=head):
                more = {}
                t, _ = run(er, [32] * 8, a.er_nit, 8, a.cus, rows=16, info=more, head=head)
                return t, {"instances": 8, "nit": a.er_nit, "instances_per_s": round(8 / t, 2), **more}
            leg("fh%d" % head, fn, path="er-5pct-2k-x8-rows-head", rows=16, parts=8, head=head)
        if "h" in legs:
            def fn_h():
                t = run_handles(er, [32] * 8, a.er_nit)
                return t, {"instances": 8, "nit": a.er_nit, "instances_per_s": round(8 / t, 2)}
            leg("h", fn_h, path="er-5pct-2k-x8-handles-8-streams")
    for r in range(a.runs):  # the legs alternate inside a round
        for name, fn, extra in todo:
            faulthandler.dump_traceback_later(a.limit, exit=True)
            t, more = fn()
            faulthandler.cancel_dump_traceback_later()
            times.setdefault(name, []).append(t)
            print(json.dumps({"leg": name, "run": r, "seconds": round(t, 4), **extra, **more}), flush=True)
    med = statistics.median
    for x in ("b", "r"):
        if "a" in times and x in times:
            out = {"summary": "median(%s) against min(a)" % x, "min_a_s": round(min(times["a"]), 4), "median_%s_s" % x: round(med(times[x]), 4),
                   "bar_met": med(times[x]) < min(times["a"])}
            if "c" in times:
                out["median_c_s"] = round(med(times["c"]), 4)
            print(json.dumps(out), flush=True)
    for x, base in [("bh", "b"), ("sh", "s8")] + [(y, "f16") for y in sorted(times) if y[:2] == "fh"]:
        if x in times and base in times:
            print(json.dumps({"summary": "median(%s) against min(%s)" % (x, base), "min_%s_s" % base: round(min(times[base]), 4),
                              "median_%s_s" % base: round(med(times[base]), 4), "median_%s_s" % x: round(med(times[x]), 4),
                              "min_%s_s" % x: round(min(times[x]), 4), "bar_met": med(times[x]) < min(times[base])}), flush=True)
    for x in sorted(times):
        if x[:1] == "f" and "h" in times:
            print(json.dumps({"summary": "median(%s) against min(h)" % x, "min_h_s": round(min(times["h"]), 4), "median_%s_s" % x: round(med(times[x]), 4),
                              "bar_met": med(times[x]) < min(times["h"])}), flush=True)


if __name__ == "__main__":
    main()
