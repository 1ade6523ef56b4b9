"""Developer tool (GPU box): the parity instrument of the solver handle (csrc/solver.h and its parts), the counterpart of
tools/batch_dump.py.  `bench.py --dump-outputs` covers the timed path; this covers the handle's other entries at the smallest shapes
that reach each path (the shapes of the existing tests).  One fixed, seeded scenario; every result goes into one .npz.  Two trees
compute the same iff their dumps are bytewise equal:

    python tools/solver_dump.py --out a.npz
    python tools/solver_dump.py --compare a.npz b.npz

The legs:
  replay   journal_graph(8, 75e-4, 1), Z 12, fp32, MMW_NO_APOST=1, 40 iterations in one call: at least one chunk is discarded and run
           again (F_BLOCKING[3] >= 1, checked and recorded).
  handle   journal_graph(8, 75e-4, 2), fp32 and fp64: gap() before an iteration, iterate(4) + iterate(2), set_slots(9, 6) cold and a
           run, the factor (host copy and resident) and its rounding with seeded projections, set_slots(11, 4, warm=True) and a run,
           set_eta between calls, sketch(seed, it).  The order is the one the entries allow: gap() needs iterations still to come, so
           it is asked first and again after four; factor needs the announced iterations done, so it follows the cold run and
           comes before the warm rebinding.
  mfma     journal_graph(16, 0.02, 4), Z 24, fp32, eta 0.01, 60 iterations: matrix-core SpMM and SDDMM, X in tile order, first-order
           chunks (F_SPMM_KIND[0] == 3 checked; F_DUAL_INFO recorded); F_XVAL / F_XAVG out of the tile order, then the factor.
  env      the journal geometry once through DeviceEnv + Solver.from_env, fp32 and fp64: every read_i32 field, S_SUM / NORM_H / ST_DATA,
           three iterations.  The cell is journal_graph_device(10, 75e-4, 0), K = 300, Z 12 -- the small case of test_hip_env.py -- and
           not the mfma leg's 16 x 16 cells: that leg already runs the matrix-core path, and this one is about the creation path and
           the read fields, which the small cell reaches in both dtypes in a fraction of the time.
  randv    the golden case run_env75 with its uploaded sketches (fp64).
After each run: the fields of test_hip_handles.FIELDS and F_XHALF, F_E_THIS, F_E_MAX, F_EXPM_INFO, F_BLOCKING, F_SPMM_KIND, F_DUAL_INFO.
F_PHASE_US and F_KERNEL_US are times and are left out."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import journal_graph, journal_graph_device  # noqa: E402

FIELDS = [("XAVG", _lib.F_XAVG), ("E_ACCU", _lib.F_E_ACCU), ("LVAL", _lib.F_LVAL), ("YAVG", _lib.F_YAVG), ("XVAL", _lib.F_XVAL),
          ("Y", _lib.F_Y), ("XHALF", _lib.F_XHALF), ("E_THIS", _lib.F_E_THIS), ("E_MAX", _lib.F_E_MAX), ("EXPM_INFO", _lib.F_EXPM_INFO),
          ("BLOCKING", _lib.F_BLOCKING), ("SPMM_KIND", _lib.F_SPMM_KIND), ("DUAL_INFO", _lib.F_DUAL_INFO)]
I_FIELDS = ["I_L_INDPTR", "I_L_INDICES", "I_ST_INDPTR", "I_ST_INDICES", "I_GAIN_X", "I_GAIN_Y", "I_ASSO_X", "I_ASSO_Y", "I_DIAG_POS", "I_ASSO_POS"]
DTYPES = [("f32", _lib.F32), ("f64", _lib.F64)]


def scenario():
    out = {}

    def dump(tag, s):
        for name, which in FIELDS:
            out["%s/%s" % (tag, name)] = s.read(which)

    def projections(seed, n, Z, rank):
        rv = np.random.default_rng(seed).standard_normal((n, Z, rank))
        return rv / np.linalg.norm(rv, axis=2, keepdims=True)

    # ---- a discarded chunk, its cautious attempt and the replay
    os.environ["MMW_NO_APOST"] = "1"
    try:
        s = _lib.Solver(12, journal_graph(8, 75e-4, seed=1), 40, 0.05, dtype=_lib.F32)
    finally:
        del os.environ["MMW_NO_APOST"]
    s.iterate(40, None, seed=3)
    dump("replay", s)
    assert out["replay/BLOCKING"][3] >= 1, "the replay leg is expected to discard at least one chunk"
    s.close()

    # ---- resumed calls, rebinding cold and warm, the step size, the gap, the factor and its rounding, the sketch
    state = journal_graph(8, 75e-4, seed=2)
    for dn, dt in DTYPES:
        t = "handle/" + dn
        s = _lib.Solver(16, state, 6, 0.05, dtype=dt)
        out[t + "/gap0"] = s.gap()
        s.iterate(4, None, seed=11)
        out[t + "/gap4"] = s.gap()
        s.iterate(2, None, seed=11)
        dump(t + "/run", s)
        s.set_slots(9, 6)
        s.iterate(6, None, seed=12)
        dump(t + "/cold", s)
        rank = min(s.K - 1, 2 * (9 - 1))
        gX = s.factor(rank, seed=1)
        out[t + "/factor"] = gX
        rv = projections(2, 3, 9, rank)
        out[t + "/round_z"], out[t + "/round_rem"] = s.round(9, gX, rv)
        df = s.factor(rank, seed=1, resident=True)
        out[t + "/round_resident_z"], out[t + "/round_resident_rem"] = s.round(9, df, rv)
        out[t + "/factor_resident"] = np.asarray(df)
        s.set_slots(11, 4, warm=True)
        s.iterate(4, None, seed=5)
        dump(t + "/warm", s)
        s.set_eta(0.11)
        s.reset(5)
        s.iterate(3, None, seed=4)
        s.set_eta(0.07)
        s.iterate(2, None, seed=4)
        dump(t + "/eta", s)
        out[t + "/sketch"] = s.sketch(7, 3)
        s.close()

    # ---- matrix cores: X in tile order, first-order chunks
    s = _lib.Solver(24, journal_graph(16, 0.02, seed=4), 60, 0.01, dtype=_lib.F32)
    s.iterate(60, None, seed=9)
    dump("mfma", s)
    assert out["mfma/SPMM_KIND"][0] == 3.0, "the mfma leg is expected to run the matrix-core SpMM"
    out["mfma/factor"] = s.factor(min(s.K - 1, 2 * 23), seed=1)
    s.close()

    # ---- the handle built on the device from the generator
    _, env = journal_graph_device(10, 75e-4, 0)
    for dn, dt in DTYPES:
        t = "env/" + dn
        s = _lib.Solver.from_env(env, 12, 3, 0.04, dtype=dt)
        for f in I_FIELDS:
            out["%s/%s" % (t, f)] = s.read_i32(getattr(_lib, f))
        for f in ("F_S_SUM", "F_NORM_H", "F_ST_DATA"):
            out["%s/%s" % (t, f)] = s.read(getattr(_lib, f))
        s.iterate(3, None, seed=5)
        dump(t, s)
        s.close()
    env.close()

    # ---- uploaded sketches
    import scipy.sparse
    g = np.load(os.path.join(ROOT, "tests", "golden", "run_env75.npz"), allow_pickle=False)
    csr = lambda p: scipy.sparse.csr_matrix((g[p + "_data"], g[p + "_indices"], g[p + "_indptr"]), shape=tuple(int(x) for x in g[p + "_shape"]))
    nit = int(g["nit"])
    s = _lib.Solver(int(g["Z"]), (csr("S"), csr("Q"), np.array(g["h_max"])), nit, float(g["eta"]), dtype=_lib.F64)
    s.iterate(nit, g["randv"][:nit])
    dump("randv", s)
    s.close()
    return out


def compare(pa, pb):
    a, c = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(c.files))
    bad += [k for k in a.files if k in c.files and (a[k].dtype != c[k].dtype or a[k].shape != c[k].shape or a[k].tobytes() != c[k].tobytes())]
    print("[solver-dump] %s vs %s: %d arrays, %d differ%s" % (pa, pb, len(a.files), len(bad), "".join("\n  " + k for k in bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="solver_dump.npz")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    out = scenario()
    np.savez(a.out, **out)
    print("[solver-dump] %d arrays -> %s" % (len(out), a.out))


if __name__ == "__main__":
    main()
