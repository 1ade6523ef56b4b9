#!/usr/bin/env python3
"""Generate tests/golden/gm_env.npz: the reference's greedy baselines (sim_src/alg/gm.py) on journal env states.

Runs only where the reference checkout is available; the fixture it writes is committed.  The reference is imported the way
make_golden.py does it (empty stand-ins for cvxpy and line_profiler, which sim_src imports but gm never uses).

Recorded per case: the state, the call's arguments and seed, the outputs (z_vec, ZZ, remainder), every visiting order the reference
actually used (np.argsort is wrapped during the call: NumPy's default argsort breaks ties in a machine-dependent order, so the
orders are part of the fixture), the randint fill and the next draw of the global stream after the call.

Usage:  python tests/golden/make_golden_gm.py   (from the repo root)
"""
import os
import sys
import types

import numpy as np
import scipy
import scipy.sparse

REF = os.environ.get("MMW_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.modules.setdefault("cvxpy", types.ModuleType("cvxpy"))
_lp = types.ModuleType("line_profiler")
_lp.LineProfiler = object
sys.modules.setdefault("line_profiler", _lp)

from sim_src.alg import gm  # noqa: E402  (the reference)
from sim_src.env.env import env  # noqa: E402

META = "reference zhouyou-gu/sig-sdp-mmw gm.py @ numpy %s / scipy %s" % (np.__version__, scipy.__version__)


def csr_parts(m, prefix):
    m = scipy.sparse.csr_matrix(m)
    m.sort_indices()
    return {prefix + "_indptr": m.indptr.astype(np.int32), prefix + "_indices": m.indices.astype(np.int32),
            prefix + "_data": m.data.astype(np.float64), prefix + "_shape": np.array(m.shape, dtype=np.int64)}


def record(alg, args, kwargs, seed):
    """Call the reference with argsort / randint recorded; returns the case's arrays."""
    orders, fills = [], []
    argsort0, randint0 = np.argsort, np.random.randint

    def argsort(a, *x, **k):
        r = argsort0(a, *x, **k)
        orders.append(np.asarray(r))
        return r

    def randint(*x, **k):
        r = randint0(*x, **k)
        fills.append(np.asarray(r))
        return r

    np.random.seed(seed)
    np.argsort, np.random.randint = argsort, randint
    try:
        z_vec, ZZ, rem = alg.run(*args, **kwargs)
    finally:
        np.argsort, np.random.randint = argsort0, randint0
    nxt = np.random.random()
    out = {"z_vec": np.asarray(z_vec, dtype=np.float64), "ZZ": np.array(int(ZZ)), "rem": np.array(int(rem)), "seed": np.array(seed),
           "next": np.array(nxt), "fill": np.concatenate(fills).astype(np.int32) if fills else np.zeros(0, dtype=np.int32)}
    if alg is gm.MAX_RAND:
        # argsort(-inprod, axis=0) and argsort(randn(K)) (gm.py:149-150)
        out["pref"] = np.ascontiguousarray(orders[0].T).astype(np.int16)
        out["rank"] = orders[1].astype(np.int16)
    else:
        # one order per slot and attempt, of the unassigned users, already mapped through kindx (gm.py:31-32)
        out["order_len"] = np.array([o.size for o in orders], dtype=np.int32)
        out["order_pos"] = np.concatenate(orders).astype(np.int16) if orders else np.zeros(0, dtype=np.int16)
    return out


def main():
    out = {"meta": np.array(META)}
    states = [("c5s0", 5, 0), ("c5s1", 5, 1), ("c8s0", 8, 0), ("c8s3", 8, 3), ("c15s0", 15, 0), ("c15s2", 15, 2)]
    names, cases = [], []
    for sname, cs, seed in states:
        state = env(cell_size=cs, sta_density_per_1m2=75e-4, seed=seed).generate_S_Q_hmax()
        for k, v in csr_parts(state[0], "S").items():
            out[sname + "/" + k] = v
        for k, v in csr_parts(state[1], "Q").items():
            out[sname + "/" + k] = v
        out[sname + "/h_max"] = np.asarray(state[2], dtype=np.float64)
        names.append(sname)
        for aname, alg in (("gain", gm.MAX_GAIN), ("asso", gm.MAX_ASSO)):
            nb = record(alg, (-1, state), {"not_Z_bound": True}, 100 + seed)
            zz = int(nb["ZZ"])
            runs = [("nb", nb, -1, 1, 1),
                    ("feas", record(alg, (zz + 2, state), {}, 200 + seed), zz + 2, 1, 0),
                    ("infeas", record(alg, (max(1, zz // 2), state), {}, 300 + seed), max(1, zz // 2), 1, 0)]
            if cs == 8 and seed == 0:
                runs.append(("att3", record(alg, (zz, state), {"nattempt": 3}, 400 + seed), zz, 3, 0))
            for rname, rec, Z, natt, nzb in runs:
                cname = "%s/%s/%s" % (sname, aname, rname)
                rec["Z"], rec["nattempt"], rec["not_Z_bound"] = np.array(Z), np.array(natt), np.array(nzb)
                for k, v in rec.items():
                    out[cname + "/" + k] = v
                cases.append(cname)
        zr = max(2, int(out["%s/gain/nb/ZZ" % sname]))
        rec = record(gm.MAX_RAND, (zr, state), {}, 500 + seed)
        rec["Z"] = np.array(zr)
        cname = "%s/rand/z%d" % (sname, zr)
        for k, v in rec.items():
            out[cname + "/" + k] = v
        cases.append(cname)
    out["states"] = np.array(names)
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "gm_env.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
