"""The reference's convergence sweep (sim_convergence_rho.py, sim_convergence_alp.py, sim_all_mmw.py: LOG_GAP = True over nit
iterations, one gap row per iteration, mmw.py:79-117) for ONE instance of any K, on a solver handle: the rows are logged inside the
loop (`Solver.set_gap`), so the run is the chunked `iterate(nit)` an unlogged run takes.  `batch.convergence_many` is the same sweep
for many instances of K <= 1024 in one launch."""
import numpy as np

from . import _lib


def convergence(Z, state, nit, eta, seed=0, rank_radio=2, dtype=None, device=0, expm_tol=None, m_cap=0):
    """`nit` iterations at `Z` slots with device sketches keyed `seed`; returns {"gap": [nit, 3], "lanczos_steps": [nit]}, the shape
    `convergence_many` returns per instance (columns 3:6 of the reference's LOGGED_NP_DATA["gap"]; steps negative where `m_cap` cut
    a Krylov space short).  state: a host triple (S_gain csr, Q_asso csr, h_max), or a `DeviceState` of a `DeviceEnv` or a
    `DeviceCSR` -- the handle is then built on the device the state lies on.  dtype: _lib.F64 (default) or _lib.F32."""
    dtype = _lib.F64 if dtype is None else dtype
    dev_state = isinstance(state, _lib.DeviceState)
    if dev_state:
        state.check()
    K = state.K if dev_state else state[0].shape[0]
    Z, nit = int(Z), int(nit)
    if not 1 <= Z <= K:
        raise ValueError("convergence: Z = %d must be in [1, K = %d]" % (Z, K))
    if nit < 1:
        raise ValueError("convergence: nit must be >= 1")
    if dev_state:
        s = state.env.solver(max(Z, 2), nit, eta, rank_radio=rank_radio, dtype=dtype)
    else:
        s = _lib.Solver(max(Z, 2), state, nit, eta, rank_radio=rank_radio, dtype=dtype, device=device)
    try:
        if expm_tol is not None:
            s.set_expm(_lib.EXPM_LANCZOS, 12, float(expm_tol))
        s.set_gap(True, m_cap=m_cap)
        s.iterate(nit, None, seed=int(seed))
        rows, steps = s.gap_log()
        return {"gap": rows, "lanczos_steps": steps}
    finally:
        s.close()
