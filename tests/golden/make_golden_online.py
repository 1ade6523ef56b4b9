#!/usr/bin/env python3
"""Generate tests/golden/online.npz from the REFERENCE's mobility environment (sim_src/env/mob_env.py on sim_src/env/env.py).

Same rules as make_golden.py: runs only where the reference is checked out, imports it with the same two stand-in modules
(cvxpy, line_profiler), never touches its files; the fixture is committed, the reference never travels.

Cases, all `mob_env(cell_size, sta_density_per_1m2=75e-4, seed)`; POINTS = 1 + 4: the drop, then after each of 4 `step_time` calls:
  c5s3   cell 5  seed 3   50 m/s,  3e6 us per call, resolution 1e5  (about 75 direction redraws per call)
  c5s0   cell 5  seed 0   1 m/s,   3e6 us per call, resolution 1e5  (a slow walk: the state changes entry by entry)
  c10s0  cell 10 seed 0   50 m/s,  3e6 us per call, resolution 1e5
  c10s1  cell 10 seed 1   0.1 m/s, 4.1e6 us per call, resolution 1e4 (the online sweeps' speed; 410 steps per call)
Every case: `sta_locs` / `sta_dirs` at every point.  The cell-5 cases also, at every point: `generate_S_Q_hmax()` as CSR, one
reference `rounding_one_attempt(Z, gX, moved state)` with its randn / randint draws recorded (make_golden.py's wrappers; gX is the
reference's own X_half of a short `mmw` run on the drop's state at Z = most users of one AP + 4, stored once), and
`evaluate_sinr` / `evaluate_bler` of that z_vec and of `arange(K) % 3`.

Usage:  python tests/golden/make_golden_online.py   (from the repo root)
"""
import os
import sys
import types

import numpy as np
import scipy
import scipy.sparse

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
sys.modules.setdefault("cvxpy", types.ModuleType("cvxpy"))
_lp = types.ModuleType("line_profiler")
_lp.LineProfiler = object
sys.modules.setdefault("line_profiler", _lp)

from sim_src.alg.mmw import mmw  # noqa: E402  (the reference)
from sim_src.env.mob_env import mob_env  # noqa: E402

from make_golden import META, state_parts  # noqa: E402

RHO = 75e-4
CALLS = 4
# name, cell, seed, speed m/s, t_us per call, resolution_us, full record
CASES = [
    ("c5s3", 5, 3, 50.0, 3e6, 1e5, True),
    ("c5s0", 5, 0, 1.0, 3e6, 1e5, True),
    ("c10s0", 10, 0, 50.0, 3e6, 1e5, False),
    ("c10s1", 10, 1, 0.1, 4.1e6, 1e4, False),
]


def one_attempt(alg, Z, gX, state, seed):
    """sdp_solver.rounding_one_attempt (sdp_solver.py:27-107) with its draws recorded."""
    cap = {}
    o_randn, o_randint = np.random.randn, np.random.randint

    def randn(*a):
        r = o_randn(*a)
        cap["randn"] = r.copy()
        return r

    def randint(*a, **k):
        r = o_randint(*a, **k)
        cap["randint"] = np.asarray(r).copy()
        return r

    np.random.seed(seed)
    np.random.randn, np.random.randint = randn, randint
    try:
        z_vec, _, rem = alg.rounding_one_attempt(Z, gX, state)
    finally:
        np.random.randn, np.random.randint = o_randn, o_randint
    pad = np.full(gX.shape[0], -1, dtype=np.int64)
    ri = cap.get("randint", np.zeros(0, dtype=np.int64))
    pad[:ri.size] = ri
    return cap["randn"], pad, z_vec.copy(), int(rem)


def main():
    out = {"meta": np.array(META), "names": np.array([c[0] for c in CASES]), "rho": np.array(RHO), "calls": np.array(CALLS)}
    for name, cell, seed, spd, t_us, res, full in CASES:
        e = mob_env(cell_size=cell, sta_density_per_1m2=RHO, seed=seed)
        K = e.n_sta
        out[name + "_cfg"] = np.array([cell, seed, spd, t_us, res], dtype=np.float64)
        locs, dirs = [], []
        if full:
            state0 = e.generate_S_Q_hmax()
            Z = int(np.diff(state0[1].indptr).max()) + 1 + 3
            alg = mmw(nit=8, eta=0.04)
            np.random.seed(500 + seed)
            _, gX = alg.run_with_state(0, Z, state0)
            out[name + "_Z"] = np.array(Z)
            out[name + "_gX"] = gX
            zb = (np.arange(K) % 3).astype(float)
            rec = {k: [] for k in ("randv", "randint", "z_vec", "rem", "sinr", "bler", "sinr_bad", "bler_bad")}
        redraws = []
        for p in range(CALLS + 1):
            if p > 0:
                before = e.sta_dirs.copy()
                e.step_time(t_us, spd, resolution_us=res)
                redraws.append(int(np.sum(np.any(before != e.sta_dirs, axis=1))))
            locs.append(e.sta_locs.copy())
            dirs.append(e.sta_dirs.copy())
            if not full:
                continue
            state = e.generate_S_Q_hmax()
            out.update({"%s_p%d_%s" % (name, p, k): v for k, v in state_parts(state).items()})
            rn, ri, z_vec, rem = one_attempt(alg, Z, gX, state, 700 + 10 * seed + p)
            rec["randv"].append(rn / np.linalg.norm(rn, axis=1, keepdims=True))  # row-normalised as at sdp_solver.py:49
            rec["randint"].append(ri)
            rec["z_vec"].append(z_vec)
            rec["rem"].append(rem)
            rec["sinr"].append(e.evaluate_sinr(z_vec, Z))
            rec["bler"].append(e.evaluate_bler(z_vec, Z))
            rec["sinr_bad"].append(e.evaluate_sinr(zb, 3))
            rec["bler_bad"].append(e.evaluate_bler(zb, 3))
        out[name + "_sta_locs"] = np.stack(locs)
        out[name + "_sta_dirs"] = np.stack(dirs)
        out[name + "_ap_locs"] = e.ap_locs.copy()
        if full:
            for k, v in rec.items():
                out[name + "_" + k] = np.array(v) if k == "rem" else np.stack(v)
        print(name, "K=%d" % K, "users with a new direction per call:", redraws, "rem per point:", rec["rem"] if full else "-")
    path = os.path.join(HERE, "online.npz")
    np.savez_compressed(path, **out)
    print("online %.0f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
