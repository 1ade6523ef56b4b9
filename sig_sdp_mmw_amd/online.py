"""The reference's online sweeps on ONE instance of any K, on the solver handle.

`batch.online_many` / `online_greedy_many` run these sweeps for many small drops at once and stop at the batch epilogue's limit
(K <= 1024).  Here the same sweeps run for one `graphs.mobile_drop` of any size on the single-instance side: a `DeviceEnv` that
moves (`mmw_env_move`), the solver handle's resident factor rounded against the state the environment holds at every time point
(`mmw_round_env`), the device scorer, and for the greedy arm a `GreedyHandle.from_env`.  The state never crosses to the host.
"""
import time

import numpy as np

from . import _lib
from .batch import _fill, probe_seed
from .binary_search import binary_search_relaxation
from .graphs import _NOISE_FLOOR_DBM, min_sinr_dec
from .mmw import mmw


def _env(drop, device):
    return _lib.DeviceEnv(drop.sta_locs, drop.ap_locs, min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=device)


def _setup(drop, nit, eta, seed, rank_radio, device, dtype):
    """sim_mmw_online.py:34-40: the environment at the drop's positions, the bisection on its device-resident state (cold probes,
    one at a time), one more solve at the Z it ends at.  Returns (env, alg, solver, Z, gX): `solver` is the handle `alg` holds for
    that state, `gX` its resident factor."""
    env = _env(drop, device)
    alg = None
    try:
        state = env.device_state()
        alg = mmw(nit=nit, rank_radio=rank_radio, eta=eta, dtype="f32" if dtype == _lib.F32 else "f64", rng="device", device=device, seed=seed)
        bs = binary_search_relaxation()
        bs.verbose = False
        bs.feasibility_check_alg = alg
        _, Z, _ = bs.run(state)
        Z = int(Z)
        _, gX = alg.run_with_state(0, Z, state)
        return env, alg, alg._device_solver(Z, state), Z, gX
    except BaseException:
        if alg is not None:
            alg.close()
        env.close()
        raise


def round_point(solver, env, Z, gX, nattempt, rng):
    """`sdp_solver.rounding(Z, gX, the state env holds now)` on the handle: up to `nattempt` attempts, each with its own Z x D'
    projection vectors drawn from `rng` (standard normals, rows normalised, sdp_solver.py:48-49) when its turn comes; the first
    attempt that leaves nobody over wins, else the last; the users it left over are then drawn from `rng` too.
    Returns (z_vec float64[K], remainder)."""
    D = int(gX.shape[1])
    z = None
    for _ in range(max(1, int(nattempt))):
        randv = rng.standard_normal((Z, D))
        randv = randv / np.linalg.norm(randv, axis=1, keepdims=True)
        zb, rem = solver.round_env(env, Z, gX, randv[None])
        z = zb[0]
        if int(rem[0]) == 0:
            break
    un = z < 0
    z_vec = z.astype(np.float64)
    if np.any(un):
        z_vec[un] = rng.integers(0, Z, int(un.sum()))
    return z_vec, int(un.sum())


def online_sweep(drop, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e5, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2,
                 device=0, dtype=_lib.F32, timings=None):
    """sim_script/journal_version/sim_mmw_online.py:34-78 for one `graphs.mobile_drop` of any K, as `batch.online_many` runs it for
    many small ones.  Setup: a `DeviceEnv` at the drop's positions, `binary_search_relaxation` on `env.device_state()` with `mmw`
    (device sketches, cold probes: the reference's search), one more solve at the Z it ends at, the factor resident.  Then per
    time point p: `env.move(drop.sta_locs)`, `Solver.round_env` of the resident factor against the moved state with up to
    `nattempt` attempts (the first feasible one wins, as `sdp_solver.rounding`), `env.evaluate` of the colouring, and the drop
    walks `step_us` microseconds in `resolution_us` steps (0: the reference's "ideal" variant -- nobody moves, fresh draws per
    point).  The drop is moved in place.
    Randomness: point p draws everything from ONE generator, `np.random.default_rng(batch.probe_seed(seed, 0, 0x80000 | p))`: first
    the projection vectors of its attempts, attempt by attempt as each comes to run, then the slots of the users the chosen attempt
    left over (`round_point`).  The global NumPy stream is used by the search (the roundings of its probes) and not after it.
    Returns {"Z", "z_vec": [n_points, K], "remainder": [n_points], "bler": [n_points, K]}.  timings: a list that receives one
    {"device_s" (move + round + evaluate), "step_s" (the host's walk)} per point."""
    env, alg, solver, Z, gX = _setup(drop, int(nit), float(eta), int(seed), int(rank_radio), int(device), dtype)
    try:
        K = drop.K
        out = {"Z": Z, "z_vec": np.empty((n_points, K)), "remainder": np.empty(n_points, dtype=np.int64), "bler": np.empty((n_points, K))}
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move(drop.sta_locs)
            rng = np.random.default_rng(probe_seed(seed, 0, 0x80000 | p))
            z_vec, rem = round_point(solver, env, Z, gX, nattempt, rng)
            _, bler = env.evaluate(z_vec, Z)
            out["z_vec"][p], out["remainder"][p], out["bler"][p] = z_vec, rem, bler
            t1 = time.perf_counter()
            drop.step_time(float(step_us), mob_spd_meter_s, resolution_us)
            if timings is not None:
                timings.append({"device_s": t1 - t0, "step_s": time.perf_counter() - t1})
        return out
    finally:
        alg.close()
        env.close()


def online_greedy_sweep(drop, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e4, seed=0, device=0, timings=None):
    """The greedy arm of the reference's online comparison (ton_major_rv/sim_mmw_online_cmp_methods.py:79-88) for one
    `graphs.mobile_drop` of any K, as `batch.online_greedy_many` runs it for many small ones: MAX_GAIN.run(-1, not_Z_bound=True)
    once on the drop's state through `GreedyHandle.from_env` (the key from the handle, the stable visiting order, all slots in one
    device call; users left over drawn from [0, ZZ) by a generator keyed by probe_seed(seed, 0, 0x40000 | 1)), then per time point
    `env.move(drop.sta_locs)`, `env.evaluate` of that ONE colouring with Z = ZZ, and the drop walks `step_us` microseconds in
    `resolution_us` steps.  The drop is moved in place.
    Returns {"Z", "z_vec": [n_points, K] (the colouring repeated), "remainder": [n_points], "bler": [n_points, K]}; timings as
    `online_sweep`."""
    env = _env(drop, int(device))
    try:
        K = drop.K
        g = _lib.GreedyHandle.from_env(env)
        try:
            slot, ZZ, rem = g.run(g.key(0), K, 1)
        finally:
            g.close()
        ZZ = int(ZZ)
        zv, rem = _fill(slot, rem, ZZ, probe_seed(seed, 0, 0x40000 | 1))
        out = {"Z": ZZ, "z_vec": np.tile(zv, (n_points, 1)), "remainder": np.full(n_points, rem, dtype=np.int64), "bler": np.empty((n_points, K))}
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move(drop.sta_locs)
            _, bler = env.evaluate(zv, ZZ)
            out["bler"][p] = bler
            t1 = time.perf_counter()
            drop.step_time(float(step_us), mob_spd_meter_s, resolution_us)
            if timings is not None:
                timings.append({"device_s": t1 - t0, "step_s": time.perf_counter() - t1})
        return out
    finally:
        env.close()
