"""Developer tool (GPU box): the parity instrument of the batch handle (csrc/batch_handle.h and its parts), as `bench.py --dump-outputs`
is of the solver handle.  One fixed, seeded scenario through every part of `BatchSolver` and `BatchEnv`; every result goes into one
.npz.  Two trees compute the same iff their dumps are bytewise equal:

    python tools/batch_dump.py --out a.npz
    python tools/batch_dump.py --compare a.npz b.npz

The scenario: six instances (journal_graph(c, 75e-4, 0) for c = 5 ... 9 and journal_graph(9, 75e-4, 1), nit 6) with the gap log on
and the split [1, 2, 1, 3, 1, 2]; iterate 4 + 2 (a resumed call); set_slots with instance 2 sitting out and a full run; the factor
under the factor split [1, 1, 2, 1, 4, 2] and its rounding; factor_random and its rounding; both greedy baselines; a BatchEnv of the
same users, moved once, with round_env and its own baselines."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph, min_sinr_dec, mobile_drop  # noqa: E402

RHO, ETA, NIT = 75e-4, 0.04, 6
CELLS = [(5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (9, 1)]
ZS = [6, 8, 10, 12, 14, 16]
ZS_RESTART = [8, 6, 0, 10, 12, 14]  # instance 2 sits out
SEEDS = [11, 12, 13, 14, 15, 16]
FIELDS = [("LVAL", _lib.F_LVAL), ("XVAL", _lib.F_XVAL), ("XAVG", _lib.F_XAVG), ("Y", _lib.F_Y), ("YAVG", _lib.F_YAVG),
          ("E_ACCU", _lib.F_E_ACCU), ("E_THIS", _lib.F_E_THIS), ("XHALF", _lib.F_XHALF), ("EXPM_INFO", _lib.F_EXPM_INFO)]


def scenario():
    out = {}
    B = len(CELLS)

    def iterate_fields(tag, b):
        for i in range(B):
            for name, which in FIELDS:
                out["%s/%d/%s" % (tag, i, name)] = b.read(i, which)
            out["%s/%d/gap_rows" % (tag, i)], out["%s/%d/gap_steps" % (tag, i)] = b.gap_log(i)

    def rounding(tag, b, res):
        z, rem, used = res
        out[tag + "/rem"], out[tag + "/used"] = rem, used
        for i in range(B):
            if z[i] is not None:
                out["%s/%d/z" % (tag, i)] = z[i]

    def factors(tag, b):
        out[tag + "/factor_call"] = np.array([b.factor_call()[k] for k in ("path", "launches", "sweeps", "widest")], dtype=np.int64)
        for i in range(B):
            if b.active[i]:
                out["%s/%d/factor" % (tag, i)] = b.read_factor(i)
                out["%s/%d/factor_info" % (tag, i)] = b.read(i, _lib.F_FACTOR_INFO, 5)

    def baselines(tag, gm, Zs):
        for kind in (0, 1):
            z, ZZ, rem, keys = gm(kind, Zs, 2, keys=True)
            out["%s/gm%d/ZZ" % (tag, kind)], out["%s/gm%d/rem" % (tag, kind)] = ZZ, rem
            for i in range(B):
                if z[i] is not None:
                    out["%s/gm%d/%d/z" % (tag, kind, i)], out["%s/gm%d/%d/key" % (tag, kind, i)] = z[i], keys[i]

    b = _lib.BatchSolver(ZS, [journal_graph(c, RHO, s) for c, s in CELLS], NIT, ETA)
    b.set_gap(True)
    b.set_split([1, 2, 1, 3, 1, 2])
    b.iterate(4, None, SEEDS)
    b.iterate(2, None, SEEDS)
    iterate_fields("run", b)

    b.set_slots(ZS_RESTART, NIT)
    b.iterate(NIT, None, SEEDS)
    iterate_fields("restart", b)

    b.set_factor_split([1, 1, 2, 1, 4, 2])
    b.factor()
    factors("factor", b)
    rounding("round", b, b.round(4, SEEDS, stop_at_first=False))
    b.factor_random(SEEDS)
    factors("factor_random", b)
    rounding("round_random", b, b.round(4, SEEDS))
    baselines("batch", b.gm, ZS_RESTART)

    drops = [mobile_drop(c, RHO, s) for c, s in CELLS]
    env = _lib.BatchEnv([d.ap_locs for d in drops], [d.K for d in drops], min_sinr=min_sinr_dec())
    for d in drops:
        d.step_time(3e6, 50.0)
    env.move([d.sta_locs for d in drops])
    b.factor()
    factors("factor_again", b)
    rounding("round_env", b, b.round_env(env, 4, SEEDS, stop_at_first=False))
    baselines("env", env.gm, ZS)
    env.close()
    b.close()
    return out


def compare(pa, pb):
    a, c = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(c.files))
    bad += [k for k in a.files if k in c.files and (a[k].dtype != c[k].dtype or a[k].shape != c[k].shape or a[k].tobytes() != c[k].tobytes())]
    print("[batch-dump] %s vs %s: %d arrays, %d differ%s" % (pa, pb, len(a.files), len(bad), "".join("\n  " + k for k in bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="batch_dump.npz")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    out = scenario()
    np.savez(a.out, **out)
    print("[batch-dump] %d arrays -> %s" % (len(out), a.out))


if __name__ == "__main__":
    main()
