"""The reference's online sweeps on ONE instance of any K, on the solver handle.

`batch.online_many` / `online_greedy_many` run these sweeps for many small drops at once and stop at the batch epilogue's limit
(K <= 1024).  Here the same sweeps run for one `graphs.mobile_drop` of any size on the single-instance side: a `DeviceEnv` that
moves (`mmw_env_move`), the solver handle's resident factor rounded against the state the environment holds at every time point
(`mmw_round_env`), the device scorer, and for the greedy arm a `GreedyHandle.from_env`.  The state never crosses to the host.
`online_resolve_sweep` is `batch.online_resolve_many` on the same side: a re-solve at every time point on a handle built on the
device from the moved environment, optionally continuing from the previous point's iterate (`Solver.carry_from`, `mmw_carry`).
Opt-in (`online_sweep(draws="device")`, `online_resolve_sweep_device`): the attempts of a point's rounding as ONE device call,
`round_point_device` -- directions drawn on the device per (key, attempt), the winner picked there (`mmw_round_env_attempts`).
"""
import contextvars
import time

import numpy as np

from . import _lib
from .batch import ALL_METHODS, METHODS, OPT_IN_METHODS, _check_warm, _fill, probe_seed, warm_iterations
from .binary_search import binary_search_relaxation
from .graphs import _NOISE_FLOOR_DBM, min_sinr_dec
from .mmw import factor_rank_seed, mmw


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
        alg, _, Z, _, _ = _search(state, nit, eta, seed, rank_radio, device, dtype)
        _, gX = alg.run_with_state(0, Z, state)
        return env, alg, alg._device_solver(Z, state), Z, gX
    except BaseException:
        if alg is not None:
            alg.close()
        env.close()
        raise


def _search(state, nit, eta, seed, rank_radio, device, dtype):
    """`_setup`'s search by itself: `binary_search_relaxation` on the device-resident `state` with `mmw` (device sketches, cold
    probes, one at a time).  Returns (alg, z_vec, Z, remainder, probes): the colouring, slot count and leftover count of the probe
    the search ends at, and the slot counts probed, in order.  `alg` (open, the caller's to close) holds the handle of `state`."""
    alg = mmw(nit=nit, rank_radio=rank_radio, eta=eta, dtype="f32" if dtype == _lib.F32 else "f64", rng="device", device=device, seed=seed)
    try:
        bs = binary_search_relaxation()
        bs.verbose = False
        bs.feasibility_check_alg = alg
        z_vec, Z, rem = bs.run(state)
        probes = [int(m) for m in bs.LOGGED_NP_DATA["bs_search_per_it"][:, 5]]  # (rows: [g_step, step, time, left, right, mid, ...])
        return alg, z_vec, int(Z), int(rem), probes
    except BaseException:
        alg.close()
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


def round_point_device(solver, env, Z, gX, nattempt, key, pick="first"):
    """`round_point` with the draws, the attempts and the choice among them on the device: ONE `Solver.round_env_attempts` call with
    seed = `key`.  Attempt a rounds with `solver.round_randv(Z, D', key, a)` (Philox keyed by (key, a): the directions of an
    attempt do not depend on how many attempts run), so with pick="first" the call returns what the sequential loop over those
    attempts with stop-at-first returns: the first attempt that leaves nobody over, else the last.  pick="fewest" (not the
    reference's rule): the attempt with the fewest users left over.  The users the winner left over are drawn from
    `np.random.default_rng(key).integers(0, Z, n)`, the batch's convention (`batch._finish`).  gX: an array, a `DeviceFactor`
    or None (the handle's resident factor).  Returns (z_vec float64[K], remainder)."""
    z, _, _ = solver.round_env_attempts(env, Z, gX, max(1, int(nattempt)), key, pick=pick)
    un = z < 0
    z_vec = z.astype(np.float64)
    if np.any(un):
        z_vec[un] = np.random.default_rng(key).integers(0, Z, int(un.sum()))
    return z_vec, int(un.sum())


def _check_draws(draws, pick):
    if draws not in ("host", "device"):
        raise ValueError("draws must be 'host' or 'device', got %r" % (draws,))
    if pick not in _lib.Solver.PICK_RULES:
        raise ValueError("pick must be 'first' or 'fewest', got %r" % (pick,))
    if draws == "host" and pick != "first":
        raise ValueError("pick=%r needs draws='device': the host loop stops at the first feasible attempt" % (pick,))


# (draws, pick) of `online_resolve_sweep`'s roundings: ("host", "first") unless `online_resolve_sweep_device` is the caller
_RESOLVE_ROUTE = contextvars.ContextVar("online_resolve_route", default=("host", "first"))


def _round_at(draws, pick, solver, env, Z, gX, nattempt, key):
    """One point's rounding by either route; `key` = probe_seed(seed, 0, 0x80000 | p) seeds the host generator or is the device key."""
    if draws == "device":
        return round_point_device(solver, env, Z, gX, nattempt, key, pick)
    return round_point(solver, env, Z, gX, nattempt, np.random.default_rng(key))


def online_sweep(drop, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e5, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2,
                 device=0, dtype=_lib.F32, timings=None, draws="host", pick="first"):
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
    draws="device" (opt-in; "host" is the above): point p is ONE device call, `round_point_device` with the key
    probe_seed(seed, 0, 0x80000 | p) -- the same number that seeds the host generator above.  Attempt a of the point rounds with the
    directions the device draws from (key, a); `pick` chooses among the attempts ("first": the sequential rule above, to the integer
    what the loop over those attempts returns; "fewest": the attempt with the fewest users left over, not the reference's); the
    users the chosen attempt left over are drawn from `np.random.default_rng(key).integers(0, Z, n)`.  The colourings differ from
    draws="host" because the directions do.  pick="fewest" needs draws="device".
    Returns {"Z", "z_vec": [n_points, K], "remainder": [n_points], "bler": [n_points, K]}.  timings: a list that receives one
    {"device_s" (move + round + evaluate), "step_s" (the host's walk)} per point."""
    _check_draws(draws, pick)
    env, alg, solver, Z, gX = _setup(drop, int(nit), float(eta), int(seed), int(rank_radio), int(device), dtype)
    try:
        K = drop.K
        out = {"Z": Z, "z_vec": np.empty((n_points, K)), "remainder": np.empty(n_points, dtype=np.int64), "bler": np.empty((n_points, K))}
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move(drop.sta_locs)
            z_vec, rem = _round_at(draws, pick, solver, env, Z, gX, nattempt, probe_seed(seed, 0, 0x80000 | p))
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


def online_resolve_sweep(drop, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e5, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2,
                         device=0, dtype=_lib.F32, resolve_nit=None, carry=False, warm_fraction=1.0 / 3.0, timings=None):
    """`online_sweep` with a re-solve at every time point, for one `graphs.mobile_drop` of any K: the handle's
    `batch.online_resolve_many` (NOT one of the reference's scripts, which solve once and re-round that factor while the stations
    walk).  Setup and point 0 are `online_sweep`'s: the resident factor of the solve the bisection ends with, rounded against the
    unmoved environment.  Z stays at that Z throughout.  Every later point p: `env.move(drop.sta_locs)`, a new handle on the moved
    state built on the device (`Solver.from_env(env, Z, n_p, eta, rank_radio, dtype)`), `carry_from` the previous point's handle
    (carry=True; at p = 1 that is the first solve's), `iterate(n_p)` with device sketches keyed probe_seed(seed, 0, 0xC0000 | p),
    the factor left resident (rank and seed: `mmw.factor_rank_seed` with that key), `round_point` with the generator keyed
    probe_seed(seed, 0, 0x80000 | p), `env.evaluate`; the previous handle is closed and the drop walks `step_us` microseconds.
    Iterations per re-solve n_p: `resolve_nit`, or when that is None `batch.warm_iterations(nit, warm_fraction)` with carry=True and
    `nit` with carry=False (a cold re-solve from the initial point).  carry=False is the default, as in the batch.
    The host draws the rounding's directions here, as `online_sweep(draws="host")`; `online_resolve_sweep_device` is this sweep
    with draws="device": the point's rounding is one `round_point_device` call with the key probe_seed(seed, 0, 0x80000 | p)
    instead of `round_point` with the generator seeded by it.
    The drop is moved in place.  Returns `online_sweep`'s dictionary plus "iters", the iterations behind every point's factor.
    timings: a list that receives per point {"create_s" (move and the new handle), "carry_s" (`carry_from`, which returns after the device's work), "iterate_s" (to the end of the
    device's work), "epilogue_s" (factor and round), "evaluate_s", "step_s"}."""
    _check_warm(warm_fraction)
    draws, pick = _RESOLVE_ROUTE.get()
    if resolve_nit is not None and int(resolve_nit) < 1:
        raise ValueError("resolve_nit must be >= 1, got %r" % (resolve_nit,))
    n_p = int(resolve_nit) if resolve_nit is not None else warm_iterations(nit, warm_fraction) if carry else int(nit)
    env, alg, solver, Z, gX = _setup(drop, int(nit), float(eta), int(seed), int(rank_radio), int(device), dtype)
    prev = None  # the previous point's handle where it is this function's to close (the first solve's belongs to `alg`)
    try:
        K = drop.K
        out = {"Z": Z, "z_vec": np.empty((n_points, K)), "remainder": np.empty(n_points, dtype=np.int64), "bler": np.empty((n_points, K)),
               "iters": [int(nit)] + [n_p] * (n_points - 1)}
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move(drop.sta_locs)
            if p == 0:
                t1 = t2 = t3 = time.perf_counter()
            else:
                s = _lib.Solver.from_env(env, Z, n_p, eta, rank_radio=rank_radio, dtype=dtype)
                try:
                    t1 = time.perf_counter()
                    if carry:
                        s.carry_from(solver)
                    t2 = time.perf_counter()
                    key = probe_seed(seed, 0, 0xC0000 | p)
                    s.iterate(n_p, None, seed=key)
                    s.sync()
                    t3 = time.perf_counter()
                    rank, factor_seed = factor_rank_seed(K, Z, rank_radio, key)
                    gX = s.factor(rank, seed=factor_seed, resident=True)
                except BaseException:
                    s.close()
                    raise
                if prev is not None:
                    prev.close()
                prev = solver = s
            z_vec, rem = _round_at(draws, pick, solver, env, Z, gX, nattempt, probe_seed(seed, 0, 0x80000 | p))
            t4 = time.perf_counter()
            _, bler = env.evaluate(z_vec, Z)
            out["z_vec"][p], out["remainder"][p], out["bler"][p] = z_vec, rem, bler
            t5 = time.perf_counter()
            drop.step_time(float(step_us), mob_spd_meter_s, resolution_us)
            if timings is not None:
                timings.append({"create_s": t1 - t0, "carry_s": t2 - t1, "iterate_s": t3 - t2, "epilogue_s": t4 - t3, "evaluate_s": t5 - t4,
                                "step_s": time.perf_counter() - t5})
        return out
    finally:
        if prev is not None:
            prev.close()
        alg.close()
        env.close()


def online_resolve_sweep_device(drop, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e5, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2,
                                device=0, dtype=_lib.F32, resolve_nit=None, carry=False, warm_fraction=1.0 / 3.0, timings=None, pick="first"):
    """`online_resolve_sweep` with draws="device" (see `online_sweep`): every point's rounding is ONE device call,
    `round_point_device` with the key probe_seed(seed, 0, 0x80000 | p) -- the number that seeds the host generator of
    `online_resolve_sweep` -- and `pick` ("first": the sequential rule; "fewest": the fewest users left over) chooses among the
    attempts.  Everything else -- the setup, the re-solves and their keys probe_seed(seed, 0, 0xC0000 | p), the result, the timings
    -- is `online_resolve_sweep`'s, which runs with the route set for this call (a context variable: other threads and tasks keep
    theirs) and whose own arguments stay as they are."""
    _check_draws("device", pick)
    token = _RESOLVE_ROUTE.set(("device", pick))
    try:
        return online_resolve_sweep(drop, n_points, step_us, mob_spd_meter_s, resolution_us, nit, eta, seed, nattempt, rank_radio, device, dtype, resolve_nit,
                                    carry, warm_fraction, timings)
    finally:
        _RESOLVE_ROUTE.reset(token)


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


def _geometry_drop(d):
    """What `_env` reads of a drop, for a `graphs.mobile_drop` or a (sta_locs, ap_locs) pair."""
    if hasattr(d, "sta_locs"):
        return d
    import types
    return types.SimpleNamespace(sta_locs=np.asarray(d[0], dtype=np.float64), ap_locs=np.asarray(d[1], dtype=np.float64))


def _embedding_arm(solver, Z, gX, nattempt, key):
    """One `sdp_solver.rounding` of a resident, index-ordered block on the handle's own state, all attempts in ONE device call with the
    directions drawn there from (key, attempt); the users the winner left over come from `np.random.default_rng(key)`
    (`batch._finish`'s convention).  Returns (z_vec float64[K], remainder)."""
    z, _, _ = solver.round_attempts(Z, gX, max(1, int(nattempt)), key)
    return _fill(z, int((z < 0).sum()), Z, key)


def compare(drop_or_geometry, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2, device=0, dtype=_lib.F32, methods=METHODS, timings=None):
    """sim_script/journal_version/sim_all_bler.py:30-72 for ONE instance of any K (a `graphs.mobile_drop` or a (sta_locs, ap_locs)
    pair), as `batch.compare_many` runs it for many small ones: one MMW search, then every baseline at the slot count Z it ends at,
    scored by BLER -- on one `DeviceEnv`, one solver handle for the embedding arms and one `GreedyHandle.from_env`; the state and the
    embeddings never cross to the host.  (The script's `lrp_solver` arm needs cvxpy and SCS and is not run.)
    "mmw" (always): `_search` on `env.device_state()` -- `binary_search_relaxation` with `mmw`, device sketches, cold probes; its
    colouring is the one the search ends with.  Then the `methods`, in the order given:
    "rand": `Solver.factor_random(Z * rank_radio, key, resident=True, index_order=True)` on the search's handle, then
    `Solver.round_attempts(Z, block, nattempt, key)`; "spectral" (only when named): `Solver.factor_spectral(Z, resident=True,
    index_order=True)` and the same rounding; "mgain" / "masso": `GreedyHandle.key(0 / 1)` then `run(key, Z, 1)`; "mrand" (only when
    named): `GreedyHandle.rand(Z, 1, key)`, gm.MAX_RAND with its draws made on the device.  Users left over are
    drawn from `np.random.default_rng(key).integers(0, Z, n)`.  key = batch.probe_seed(seed, 0, 0x40000 | m), m the method's index in
    batch.ALL_METHODS (= METHODS + OPT_IN_METHODS + ("mrand",)): `batch.baselines_many`'s keys at instance 0.  One `env.evaluate` per method.
    Returns {"Z", "probes", "z_vec": {method: float64[K]}, "remainder": {method: int}, "bler": {method: float64[K]}}, "mmw"
    included.  timings: a dict that receives {"search_s", "baselines_s", "evaluate_s"} and "arm_s": {method: seconds}.  A method
    that is not one of batch.ALL_METHODS raises ValueError by name before any device work."""
    names = ALL_METHODS
    methods = tuple(methods)
    for name in methods:
        if name not in names:
            raise ValueError("compare: method must be one of %s, got %r" % (names, name))
    drop = _geometry_drop(drop_or_geometry)
    env = _env(drop, int(device))
    alg = greedy = None
    try:
        state = env.device_state()
        t0 = time.perf_counter()
        alg, z_mmw, Z, rem_mmw, probes = _search(state, int(nit), float(eta), int(seed), int(rank_radio), int(device), dtype)
        solver = alg._device_solver(Z, state)
        t1 = time.perf_counter()
        z_vec, remainder, arm_s = {"mmw": np.asarray(z_mmw, dtype=np.float64)}, {"mmw": rem_mmw}, {}
        for name in methods:
            ta = time.perf_counter()
            m = names.index(name)
            key = probe_seed(seed, 0, 0x40000 | m)
            if name == "rand":
                block = solver.factor_random(Z * int(rank_radio), key, resident=True, index_order=True)
                z_vec[name], remainder[name] = _embedding_arm(solver, Z, block, nattempt, key)
            elif name == "spectral":
                block = solver.factor_spectral(Z, resident=True, index_order=True)
                z_vec[name], remainder[name] = _embedding_arm(solver, Z, block, nattempt, key)
            else:
                if greedy is None:
                    greedy = _lib.GreedyHandle.from_env(env)
                if name == "mrand":
                    slot, rems, _ = greedy.rand(Z, 1, key)
                    rem = int(rems[0])
                else:
                    slot, _, rem = greedy.run(greedy.key(m - 1), Z, 1)
                z_vec[name], remainder[name] = _fill(slot, rem, Z, key)
            arm_s[name] = time.perf_counter() - ta
        t2 = time.perf_counter()
        bler = {}
        for name in ("mmw",) + methods:
            _, bler[name] = env.evaluate(z_vec[name], Z)
        if timings is not None:
            timings.update(search_s=t1 - t0, baselines_s=t2 - t1, evaluate_s=time.perf_counter() - t2, arm_s=arm_s)
        return {"Z": Z, "probes": probes, "z_vec": z_vec, "remainder": remainder, "bler": bler}
    finally:
        if greedy is not None:
            greedy.close()
        if alg is not None:
            alg.close()
        env.close()
