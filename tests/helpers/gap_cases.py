"""Graphs and references of the solver handle's in-loop gap tests (test_hip_gap_handle.py): the handle kinds the phase is run on,
and the float64 recomputation of a gap row from running sums read back from a handle."""
import functools

import numpy as np

from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

from . import mfma_graphs as mg

# kind: (state, Z, rank_radio, dtype, eta, expm tolerance, on the matrix cores)
KINDS = {
    "f64-er240": (lambda: er_contention_graph(240, 0.04, 3), 14, 2, _lib.F64, 0.04, 1e-12, False),
    "f32-er240": (lambda: er_contention_graph(240, 0.04, 3), 14, 2, _lib.F32, 0.04, 1e-6, False),
    "f32-mfma-j9": (lambda: mg.state("j9"), 125, 1, _lib.F32, 0.04, 1e-6, True),
    "f32-mfma-hub": (lambda: mg.state("hub"), 125, 1, _lib.F32, 0.04, 1e-6, True),
}


@functools.lru_cache(maxsize=None)
def k300():
    """journal_graph(10, 75e-4, 0): K = 300, run at Z = 36."""
    return journal_graph(10, 75e-4, 0)


@functools.lru_cache(maxsize=None)
def pattern(kind_or_key, Z=None):
    if Z is None:
        mk, Z, _, _, _, _, _ = KINDS[kind_or_key]
        return orc.Pattern(Z, mk())
    return orc.Pattern(Z, kind_or_key)


def recompute(p, xsum, ysum, n):
    """The row {e_max, K lambda_min(L(Ybar)), difference} of mmw.py:79-117 from sums of n terms, in float64 with a dense eigvalsh."""
    e_max = float(np.max(orc.violations(p, np.asarray(xsum, dtype=np.float64) / n)))
    L = p.csr(orc.loss_values(p, np.asarray(ysum, dtype=np.float64) / n)).toarray()
    kt = float(np.linalg.eigvalsh(0.5 * (L + L.T))[0]) * p.K
    return np.array([e_max, kt, e_max - kt])


def make(kind, nit):
    mk, Z, rr, dtype, eta, tol, _ = KINDS[kind]
    s = _lib.Solver(Z, mk(), nit, eta, rank_radio=rr, dtype=dtype)
    s.set_expm(_lib.EXPM_LANCZOS, 12, tol)
    return s
