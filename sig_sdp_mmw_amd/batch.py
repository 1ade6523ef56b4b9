"""Many small MMW solves at once: the batched solver (one workgroup per instance, csrc/kernels_batch.h) behind the reference's
sweep loops (sim_script/journal_version/*: seeds x cell sizes, one `binary_search_relaxation` per instance).

    ok_xhalf = run_with_state_many(it, Zs, states, nit=150, eta=0.04, seeds=seeds)   # [(True, X_half), ...]
    results  = search_many(states, nit=150, eta=0.04, seed=0)                          # [{"Z", "z_vec", "remainder", "probes"}, ...]

    curves   = convergence_many(Zs, states, nit=625, eta=0.04)                         # [{"gap": [nit, 3], "lanczos_steps": [nit]}, ...]
    online   = online_many(drops, n_points=11, step_us=1e6, mob_spd_meter_s=0.1)       # [{"Z", "probes", "z_vec", "remainder", "bler"}, ...]
    base     = baselines_many(batch_solver, Zs)                                        # [{"rand" / "mgain" / "masso": (z_vec, Z, remainder)}, ...]
    cmp      = compare_many(drops, nit=150, eta=0.04)                                  # [{"Z", "probes", "bler": {"mmw", "rand", "mgain", "masso"}}, ...]
    resolved = online_resolve_many(drops, n_points=11, step_us=1e6, mob_spd_meter_s=1.0)  # online_many's results plus "iters"; a re-solve per point
    greedy   = online_greedy_many(drops, n_points=11, step_us=1e6)                     # [{"Z", "z_vec", "remainder", "bler"}, ...]

The iterations of every instance run in one launch per call.  The epilogue of a probe (X_half and the rounding) is chosen by
`epilogue=`: "handle" (the default) exports the instance's iterate into an fp64 handle of the same state (mmw_batch_export) and runs
`mmw_factor` / `mmw_round` there, one instance after another; "batch" runs both inside the batch (csrc/kernels_batch_epilogue.h):
a round of probes is then one `iterate`, one `factor` and one `round`, and instances over `_lib.BATCH_EPILOGUE_MAX_K` take the
handle path inside the same call.  The two factor by different methods, so their bases differ: the same bisection, not bitwise
the same slots.

`states` are (S_gain, Q_asso, h_max) triples.  When every one of them is a `DeviceCSR.device_state()` on one device,
`run_with_state_many`, `convergence_many` and `search_many` build their batch there (`BatchSolver.from_csr`) and make no host copy
of a state; the results are bitwise those of the triples `c.state()`.

`search_many` runs the bisection of binary_search_relaxation.py:44-72 for all instances in lockstep: each instance keeps its own
bounds, all current probes run in one `mmw_batch_iterate`, and an instance whose search has ended sits out.  Sketches are the
device's Philox blocks keyed by a per-(instance, probe) seed, and the rounding's projections come from a generator keyed the same
way, so `single(state, index)` -- the reference's `run_with_state` / `rounding` protocol backed by a batch of one -- driven by
`binary_search_relaxation` makes the same probes and ends at the same Z (instances are bitwise independent of their batch).
"""
import math
import time

import numpy as np

from . import _lib
from .binary_search import binary_search_relaxation
from .graphs import _NOISE_FLOOR_DBM, min_sinr_dec


def probe_seed(seed, index, probe):
    """The device sketch seed of probe `probe` of instance `index` (what search_many and single agree on)."""
    return ((int(seed) & 0xFFFFFF) << 40) | ((int(index) & 0xFFFFF) << 20) | (int(probe) & 0xFFFFF)


def _rank(K, Z, rank_radio):
    return int(min(K - 1, (Z - 1) * rank_radio))


class _Handles:
    """One fp64 handle per state, rebound to each probe's slot count (the export target)."""

    def __init__(self, states, nit, eta, rank_radio, device, owners=None):
        self.states, self.nit, self.eta, self.rank_radio, self.device = states, nit, eta, rank_radio, device
        self.owners = owners  # the states' DeviceCSRs when the batch was built from them (`_batch`): the handles are built there too
        self.h = [None] * len(states)

    def get(self, i, Z):
        h = self.h[i]
        if h is None and self.owners is not None:
            h = self.h[i] = self.owners[i].solver(Z, self.nit, self.eta, rank_radio=self.rank_radio, dtype=_lib.F64)
        elif h is None:
            h = self.h[i] = _lib.Solver(Z, self.states[i], self.nit, self.eta, rank_radio=self.rank_radio, dtype=_lib.F64, device=self.device)
        elif h.Z != Z:
            h.set_slots(Z, self.nit)
        return h

    def close(self):
        for h in self.h:
            if h is not None:
                h.close()
        self.h = [None] * len(self.states)


def _csr_route(states):
    """The `DeviceCSR` owners when EVERY state is a `DeviceState` of a `DeviceCSR` and all of them lie on one device >= 0, else None:
    host triples, a mix, a DeviceState of a DeviceEnv and device = -1 owners take the host path untouched."""
    owners = []
    for st in states:
        c = _lib.csr_owner(st) if isinstance(st, _lib.DeviceState) else None
        if c is None or c.device < 0 or (owners and c.device != owners[0].device):
            return None
        owners.append(c)
    return owners or None


def _batch(Zs, states, nit, eta, rank_radio, device):
    """(batch, owners): the batch of a workflow.  States that lie on the device as CSR arrays (`_csr_route`) are built into it there
    (`BatchSolver.from_csr`: no host copy of any state; bitwise the batch of the host triples `c.state()`), on their own device;
    anything else goes through `BatchSolver(Zs, states, ...)` on `device`, owners None."""
    owners = _csr_route(states)
    if owners is not None:
        return _lib.BatchSolver.from_csr(owners, list(Zs), nit, eta, rank_radio=rank_radio), owners
    return _lib.BatchSolver(list(Zs), states, nit, eta, rank_radio=rank_radio, device=device), None


def _factor(batch, i, handle, Z, rank_radio, seed):
    batch.export(i, handle)
    return handle.factor(_rank(handle.K, Z, rank_radio), seed=seed)


def _round(handle, Z, X_half, state, seed, nattempt):
    """sdp_solver.rounding (sdp_solver.py:18-25): up to `nattempt` attempts, the first with remainder 0 wins; projections and the
    random slots of users left over (:104-105) from a generator keyed by `seed`."""
    rng = np.random.default_rng(seed)
    Dp = X_half.shape[1]
    r = rng.standard_normal((nattempt, Z, Dp))
    r = r / np.linalg.norm(r, axis=2, keepdims=True)
    z, rem = handle.round(Z, X_half, r)
    a = int(np.argmax(rem == 0)) if np.any(rem == 0) else nattempt - 1
    z_vec = z[a].astype(np.float64)
    un = z[a] < 0
    if np.any(un):
        z_vec[un] = rng.integers(0, Z, size=int(un.sum()))
    return z_vec, Z, int(rem[a])


def _check_epilogue(epilogue):
    if epilogue not in ("handle", "batch"):
        raise ValueError('epilogue must be "handle" or "batch", got %r' % (epilogue,))
    return epilogue == "batch"


def _fits(b, i):
    return b.sizes[i]["K"] <= _lib.BATCH_EPILOGUE_MAX_K


def _split(b, split):
    """The `split=` keyword of the workflows: None is the single-launch kernel; an int, one int per instance or "auto" goes to
    `BatchSolver.set_split` (every result stays bitwise the same; see there)."""
    if split is not None:
        b.set_split(split)


def _row_split(b, row_split):
    """The `row_split=` keyword of the workflows, beside `split=`: None is no row split; an int, one int per instance or "auto" goes to
    `BatchSolver.set_row_split` after the column split is set (every result stays bitwise the same; see there)."""
    if row_split is not None:
        b.set_row_split(row_split)


def _head_split(b, head_split):
    """The `head_split=` keyword of the workflows, beside `split=` and `row_split=`: None leaves the head on one workgroup per instance; an
    int, one int per instance or "auto" goes to `BatchSolver.set_head_split` after both (every result stays bitwise the same; see there)."""
    if head_split is not None:
        b.set_head_split(head_split)


def _factor_split(b, factor_split, in_batch=True):
    """The `factor_split=` keyword of the workflows: None is k_batch_factor's one launch; an int, one int per instance or "auto" goes
    to `BatchSolver.set_factor_split` (every result stays bitwise the same; see there).  There is no batch factor to split under
    epilogue="handle"."""
    if factor_split is None:
        return
    if not in_batch:
        raise ValueError('factor_split needs epilogue="batch": the handle epilogue has no batch factor to split')
    if b is not None:
        b.set_factor_split(factor_split)


def _finish(z, rem, used, i, Z, seed):
    """The attempt sdp_solver.rounding returns (sdp_solver.py:21-25: the first with remainder 0, else the last) out of a batch `round`,
    users left over drawn from a generator keyed by the probe seed (:104-105)."""
    a = int(used[i]) - 1
    z_vec = z[i][a].astype(np.float64)
    un = z[i][a] < 0
    if np.any(un):
        z_vec[un] = np.random.default_rng(seed).integers(0, Z, int(un.sum()))
    return z_vec, Z, int(rem[i][a])


def run_with_state_many(bs_iteration, Zs, states, nit=150, eta=0.04, seeds=None, rank_radio=2, device=0, factor_seed=0, epilogue="handle", split=None,
                        factor_split=None, row_split=None, head_split=None):
    """mmw.run_with_state (mmw.py:44-222) for every (Z, state) pair at once: one batch, `nit` iterations in one launch, then
    X_half per instance through export + mmw_factor on one reused fp64 handle per state, or with epilogue="batch" all of them in one
    more launch (instances over the epilogue limit still go through a handle).  factor_split: workgroups per instance for that
    factor (`BatchSolver.set_factor_split`; epilogue="batch" only).  row_split: row parts per instance beside `split`
    (`BatchSolver.set_row_split`).  head_split: row parts per instance for the head of an iteration (`BatchSolver.set_head_split`).
    Returns [(True, X_half), ...]."""
    del bs_iteration  # the log index of the reference's signature; nothing here depends on it
    in_batch = _check_epilogue(epilogue)
    _factor_split(None, factor_split, in_batch)
    seeds = np.arange(len(states), dtype=np.uint64) if seeds is None else np.asarray(seeds, dtype=np.uint64)
    b, owners = _batch(Zs, states, nit, eta, rank_radio, device)
    hs = _Handles(states, nit, eta, rank_radio, device, owners)
    try:
        _split(b, split)
        _row_split(b, row_split)
        _head_split(b, head_split)
        _factor_split(b, factor_split, in_batch)
        b.iterate(nit, None, seeds)
        take = [in_batch and _fits(b, i) for i in range(len(states))]
        if any(take):
            b.factor(take)
        return [(True, b.read_factor(i) if take[i] else _factor(b, i, hs.get(i, int(Z)), int(Z), rank_radio, factor_seed))
                for i, Z in enumerate(Zs)]
    finally:
        hs.close()
        b.close()


def convergence_many(Zs, states, nit, eta, seeds=None, rank_radio=2, device=0, split=None, row_split=None, head_split=None):
    """The reference's convergence sweeps (sim_convergence_rho.py, sim_all_mmw.py: LOG_GAP = True, one run per instance) as one
    batch: `nit` and `eta` are one value for all or one per instance, the gap is logged inside the launch (mmw.py:79-117) and all
    iterations of all instances run in ONE `iterate`.  Returns per instance {"gap": [nit, 3], "lanczos_steps": [nit]}; the three
    columns are LOGGED_NP_DATA["gap"][:, 3:6] of the reference."""
    B = len(states)
    nits = [int(x) for x in np.broadcast_to(np.asarray(nit, dtype=np.int64), (B,))]
    etas = np.broadcast_to(np.asarray(eta, dtype=np.float64), (B,))
    seeds = np.arange(B, dtype=np.uint64) if seeds is None else np.asarray(seeds, dtype=np.uint64)
    b, _ = _batch(Zs, states, nits, float(etas[0]), rank_radio, device)
    try:
        b.set_eta(etas)
        b.set_gap(True)
        _split(b, split)
        _row_split(b, row_split)
        _head_split(b, head_split)
        b.iterate(max(nits), None, seeds)
        out = []
        for i in range(B):
            rows, steps = b.gap_log(i)
            out.append({"gap": rows, "lanczos_steps": steps})
        return out
    finally:
        b.close()


def warm_iterations(nit, warm_fraction):
    """Iterations of a warm-started probe: max(1, ceil(nit * warm_fraction)), the rule of `mmw._run`."""
    return max(1, int(math.ceil(int(nit) * float(warm_fraction))))


def _check_warm(warm_fraction):
    if not 0.0 < float(warm_fraction) <= 1.0:
        raise ValueError("warm_fraction must be in (0, 1], got %r" % (warm_fraction,))


def search_many(states, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2, device=0, epilogue="handle", timings=None, split=None,
                factor_split=None, row_split=None, head_split=None, warm_start=False, warm_fraction=1.0 / 3.0):
    """The bisection of binary_search_relaxation.py:44-72 for every state, in lockstep (one batch launch per round of probes).
    Returns per state {"Z", "z_vec", "remainder", "probes" (the slot counts probed, in order), "bounds"}.  epilogue="batch": the
    factors and the roundings of a round are one launch each (the rounding seed is the probe seed).  timings: a list that receives
    one {"probes", "iterate_s", "epilogue_s", "factor_call"} per round (epilogue_s: everything of the round after `iterate`, the
    bisection's own bookkeeping included; factor_call: `BatchSolver.factor_call()` of the round's batch factor, None without one).  split: workgroups per instance (`BatchSolver.set_split`: an int, one per instance or "auto", which
    follows the slot counts of every round; None: one each); the results are bitwise the same.  factor_split: the same for the
    factor of epilogue="batch" (`BatchSolver.set_factor_split`; with epilogue="handle" anything but None raises ValueError), row_split: row parts
    per instance multiplied with `split`'s column slices (`BatchSolver.set_row_split`: an int, one per instance or "auto"), bitwise
    too; head_split: row parts per instance for the head of an iteration and the plan (`BatchSolver.set_head_split`: the same values),
    bitwise too.  warm_start (opt-in; NOT the reference's search, which restarts every probe at mmw.py:62-68): the first probe of every
    instance runs cold with `nit`, every later round continues from the previous probe's iterate (`set_slots(..., warm=True)`) with
    `warm_iterations(nit, warm_fraction)` iterations; the probe seeds are unchanged.  Every result also holds "iters", the
    iterations of every probe in order, and every timings row "set_slots_s", the round's slot change."""
    in_batch = _check_epilogue(epilogue)
    _factor_split(None, factor_split, in_batch)
    _check_warm(warm_fraction)
    B = len(states)
    bs = binary_search_relaxation()
    bounds = [bs.set_bounds(st) for st in states]
    left = [lb for lb, _ in bounds]
    right = [ub for _, ub in bounds]
    done = [False] * B
    probes = [[] for _ in range(B)]
    iters = [[] for _ in range(B)]
    out = [None] * B
    mids = [max(2, math.floor(float(l + r) / 2.)) for l, r in zip(left, right)]
    b, owners = _batch(mids, states, nit, eta, rank_radio, device)
    hs = _Handles(states, nit, eta, rank_radio, device, owners)
    try:
        _split(b, split)
        _row_split(b, row_split)
        _head_split(b, head_split)
        _factor_split(b, factor_split, in_batch)
        while not all(done):
            mids = [0 if done[i] else math.floor(float(left[i] + right[i]) / 2.) for i in range(B)]
            warm = bool(warm_start) and any(probes)  # the instances run in lockstep: after the first round every one has iterated
            n_round = warm_iterations(nit, warm_fraction) if warm else nit
            ts = time.perf_counter()
            b.set_slots(mids, n_round, warm=warm)
            seeds = np.array([probe_seed(seed, i, len(probes[i])) for i in range(B)], dtype=np.uint64)
            t0 = time.perf_counter()
            b.iterate(n_round, None, seeds)
            t1 = time.perf_counter()
            take = [in_batch and not done[i] and _fits(b, i) for i in range(B)]
            if any(take):
                b.factor(take)
                zs, rems, used = b.round(nattempt, seeds, take)
            for i in range(B):
                if done[i]:
                    continue
                Z = mids[i]
                if take[i]:
                    z_vec, Z, rem = _finish(zs, rems, used, i, Z, int(seeds[i]))
                else:
                    h = hs.get(i, Z)
                    Xh = _factor(b, i, h, Z, rank_radio, 0)
                    z_vec, Z, rem = _round(h, Z, Xh, states[i], probe_seed(seed, i, len(probes[i])), nattempt)
                probes[i].append(Z)
                iters[i].append(n_round)
                left[i], right[i], fin = binary_search_relaxation._step(left[i], right[i], Z, rem)
                if fin:
                    done[i] = True
                    out[i] = {"Z": Z, "z_vec": z_vec, "remainder": rem, "probes": probes[i], "bounds": bounds[i], "iters": iters[i]}
            if timings is not None:
                timings.append({"probes": int(sum(1 for m in mids if m > 0)), "iterate_s": t1 - t0, "epilogue_s": time.perf_counter() - t1,
                                "factor_call": b.factor_call() if any(take) else None, "set_slots_s": t0 - ts})
        return out
    finally:
        hs.close()
        b.close()


def online_many(drops, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e5, nit=150, eta=0.04, seed=0, nattempt=10,
                rank_radio=2, device=0, timings=None, split=None, factor_split=None, row_split=None, head_split=None, warm_start=False, warm_fraction=1.0 / 3.0):
    """The reference's online sweeps (sim_script/journal_version/sim_mmw_online.py:34-78, ton_major_rv/sim_mmw_online_cmp_*.py) for
    many `graphs.mobile_drop`s at once: the bisection on the drops' states (`search_many(..., epilogue="batch")`), one more solve at
    the Z it ends at for gX (:40) -- a batch of the (Z, state) pairs, iterated and factored once, the sketches keyed by the probe
    index after the search's last -- and then, per time point, for all instances together: the state of the stations where they
    are now (`BatchEnv.move`), `rounding(Z, gX, that state)` on the resident factors (`round_env`, draws keyed by
    probe_seed(seed, i, 0x80000 | point), users left over drawn as in the search) and `evaluate_bler` of the colouring; then every
    drop walks `step_us` microseconds (one value, or one per instance: the reference passes its own measured search time; 0 is its
    "ideal" variant -- nobody moves, fresh draws per point).  The drops are moved in place.
    Returns per instance {"Z", "probes", "z_vec": [n_points, K], "remainder": [n_points], "bler": [n_points, K]}.  timings: a list
    that receives one {"device_s" (move + round + evaluate), "step_s" (the host's walk)} per point.  factor_split: workgroups per
    instance for every factor, the search's and the last solve's (`BatchSolver.set_factor_split`).  warm_start / warm_fraction go to
    the search and nowhere else (`search_many`)."""
    B = len(drops)
    for i, d in enumerate(drops):
        if d.K > _lib.BATCH_EPILOGUE_MAX_K:
            raise ValueError("online_many: instance %d has K = %d users, over the batch epilogue's limit %d" % (i, d.K, _lib.BATCH_EPILOGUE_MAX_K))
    steps = [float(x) for x in np.broadcast_to(np.asarray(step_us, dtype=np.float64), (B,))]
    states = [d.state() for d in drops]
    found = search_many(states, nit=nit, eta=eta, seed=seed, nattempt=nattempt, rank_radio=rank_radio, device=device, epilogue="batch", split=split,
                        factor_split=factor_split, row_split=row_split, head_split=head_split, warm_start=warm_start, warm_fraction=warm_fraction)
    Zs = [int(r["Z"]) for r in found]
    out = [{"Z": Zs[i], "probes": found[i]["probes"], "z_vec": np.empty((n_points, drops[i].K)), "remainder": np.empty(n_points, dtype=np.int64),
            "bler": np.empty((n_points, drops[i].K))} for i in range(B)]
    b = _lib.BatchSolver(Zs, states, nit, eta, rank_radio=rank_radio, device=device)
    env = _lib.BatchEnv([d.ap_locs for d in drops], [d.K for d in drops], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=device)
    try:
        _split(b, split)
        _row_split(b, row_split)
        _head_split(b, head_split)
        _factor_split(b, factor_split)
        b.iterate(nit, None, np.array([probe_seed(seed, i, len(found[i]["probes"])) for i in range(B)], dtype=np.uint64))
        b.factor()
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move([d.sta_locs for d in drops])
            seeds = np.array([probe_seed(seed, i, 0x80000 | p) for i in range(B)], dtype=np.uint64)
            z, rem, used = b.round_env(env, nattempt, seeds)
            fin = [_finish(z, rem, used, i, Zs[i], int(seeds[i])) for i in range(B)]
            _, bler = env.evaluate([f[0] for f in fin], Zs)
            for i in range(B):
                out[i]["z_vec"][p], out[i]["remainder"][p], out[i]["bler"][p] = fin[i][0], fin[i][2], bler[i]
            t1 = time.perf_counter()
            for d, t in zip(drops, steps):
                d.step_time(t, mob_spd_meter_s, resolution_us)
            if timings is not None:
                timings.append({"device_s": t1 - t0, "step_s": time.perf_counter() - t1})
        return out
    finally:
        env.close()
        b.close()


def online_resolve_many(drops, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e5, nit=150, eta=0.04, seed=0, nattempt=10,
                        rank_radio=2, device=0, resolve_nit=None, carry=False, warm_fraction=1.0 / 3.0, timings=None, split=None, factor_split=None,
                        row_split=None, head_split=None, handover="host"):
    """`online_many` with a re-solve at every time point (NOT one of the reference's scripts, which solve once and re-round that
    factor while the stations walk).  The start is `online_many`'s: the bisection on the drops' states, one more solve at the Z it
    ends at with the same sketch seed, and point 0 is that factor rounded on the unmoved state.  Z stays at that Z throughout.
    Every later point p, for all instances together: `BatchEnv.move`, the states fetched (`BatchEnv.state`), a new `BatchSolver` on
    them at the Zs with the splits applied, `carry_from` the previous point's batch (carry=True; at p = 1 that is the first
    solve's), `iterate` with sketches keyed by probe_seed(seed, i, 0xC0000 | p), `factor`, `round` with draws keyed by
    probe_seed(seed, i, 0x80000 | p) (users left over drawn as in the search), `BatchEnv.evaluate`; the previous batch is closed
    and every drop walks `step_us` microseconds.  Iterations per re-solve: `resolve_nit`, or when that is None
    `warm_iterations(nit, warm_fraction)` with carry=True and `nit` with carry=False (a cold re-solve from the initial point).
    carry=False is the default: measured on the sweep's mix, the carried re-solve's colourings were not better than a cold
    re-solve's at the same iterations.
    The drops are moved in place.  Returns `online_many`'s dictionaries plus "iters", the iterations behind every point's factor.
    timings: a list that receives per point {"create_s" (move, states, the new batch), "carry_s", "iterate_s", "epilogue_s" (factor
    and round), "evaluate_s", "step_s"}.
    handover: how a time point's states reach its new batch.  "host" (the default): `BatchEnv.state` per instance and
    `BatchSolver` on those arrays.  "device": `BatchSolver.from_env`, which builds the same batch on the device from the
    environment itself; the returned dictionaries are bitwise the same."""
    if handover not in ("host", "device"):
        raise ValueError("online_resolve_many: handover must be \"host\" or \"device\", got %r" % (handover,))
    B = len(drops)
    for i, d in enumerate(drops):
        if d.K > _lib.BATCH_EPILOGUE_MAX_K:
            raise ValueError("online_resolve_many: instance %d has K = %d users, over the batch epilogue's limit %d" % (i, d.K, _lib.BATCH_EPILOGUE_MAX_K))
    _check_warm(warm_fraction)
    if resolve_nit is not None and int(resolve_nit) < 1:
        raise ValueError("resolve_nit must be >= 1, got %r" % (resolve_nit,))
    n_p = int(resolve_nit) if resolve_nit is not None else warm_iterations(nit, warm_fraction) if carry else int(nit)
    steps = [float(x) for x in np.broadcast_to(np.asarray(step_us, dtype=np.float64), (B,))]
    states = [d.state() for d in drops]
    found = search_many(states, nit=nit, eta=eta, seed=seed, nattempt=nattempt, rank_radio=rank_radio, device=device, epilogue="batch", split=split,
                        factor_split=factor_split, row_split=row_split, head_split=head_split)
    Zs = [int(r["Z"]) for r in found]
    out = [{"Z": Zs[i], "probes": found[i]["probes"], "z_vec": np.empty((n_points, drops[i].K)), "remainder": np.empty(n_points, dtype=np.int64),
            "bler": np.empty((n_points, drops[i].K)), "iters": [int(nit)] + [n_p] * (n_points - 1)} for i in range(B)]

    def solver(sts, n):
        """The batch on the states `sts`, or (sts None) on the ones `env` holds, built on the device."""
        if sts is None:
            b = _lib.BatchSolver.from_env(env, Zs, n, eta, rank_radio=rank_radio)
        else:
            b = _lib.BatchSolver(Zs, sts, n, eta, rank_radio=rank_radio, device=device)
        try:
            _split(b, split)
            _row_split(b, row_split)
            _head_split(b, head_split)
            _factor_split(b, factor_split)
        except Exception:
            b.close()
            raise
        return b

    prev = solver(states, nit)
    env = None
    try:
        env = _lib.BatchEnv([d.ap_locs for d in drops], [d.K for d in drops], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=device)
        prev.iterate(nit, None, np.array([probe_seed(seed, i, len(found[i]["probes"])) for i in range(B)], dtype=np.uint64))
        prev.factor()
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move([d.sta_locs for d in drops])
            seeds = np.array([probe_seed(seed, i, 0x80000 | p) for i in range(B)], dtype=np.uint64)
            if p == 0:
                t1 = t2 = t3 = time.perf_counter()
                z, rem, used = prev.round_env(env, nattempt, seeds)
            else:
                b = solver([env.state(i) for i in range(B)] if handover == "host" else None, n_p)
                try:
                    t1 = time.perf_counter()
                    if carry:
                        b.carry_from(prev)
                    t2 = time.perf_counter()
                    b.iterate(n_p, None, np.array([probe_seed(seed, i, 0xC0000 | p) for i in range(B)], dtype=np.uint64))
                    t3 = time.perf_counter()
                    b.factor()
                    z, rem, used = b.round(nattempt, seeds)
                except Exception:
                    b.close()
                    raise
                prev.close()
                prev = b
            fin = [_finish(z, rem, used, i, Zs[i], int(seeds[i])) for i in range(B)]
            t4 = time.perf_counter()
            _, bler = env.evaluate([f[0] for f in fin], Zs)
            for i in range(B):
                out[i]["z_vec"][p], out[i]["remainder"][p], out[i]["bler"][p] = fin[i][0], fin[i][2], bler[i]
            t5 = time.perf_counter()
            for d, t in zip(drops, steps):
                d.step_time(t, mob_spd_meter_s, resolution_us)
            if timings is not None:
                timings.append({"create_s": t1 - t0, "carry_s": t2 - t1, "iterate_s": t3 - t2, "epilogue_s": t4 - t3, "evaluate_s": t5 - t4,
                                "step_s": time.perf_counter() - t5})
        return out
    finally:
        if env is not None:
            env.close()
        prev.close()


METHODS = ("rand", "mgain", "masso")  # the baselines of sim_all_bler.py:42-72 that run inside the batch, in its order
OPT_IN_METHODS = ("spectral",)  # what baselines_many also takes when it is named: spectral_sdp_solver (sdp_solver.py:165-185)
DEVICE_DRAW_METHODS = ("mrand",)  # likewise: gm.MAX_RAND (gm.py:131-200) with its draws on the device (`gm_rand`); index 4 in the key scheme
ALL_METHODS = METHODS + OPT_IN_METHODS + DEVICE_DRAW_METHODS


def _fill(slot, rem, high, seed):
    """gm.py:60-64: the users a greedy baseline left over (-1) drawn from [0, high), from a generator keyed by `seed`."""
    z_vec = slot.astype(np.float64)
    un = slot < 0
    if np.any(un):
        z_vec[un] = np.random.default_rng(seed).integers(0, high, int(un.sum()))
    return z_vec, int(rem)


def baselines_many(source, Zs, methods=METHODS, seed=0, nattempt_round=10, nattempt_gm=1):
    """The baselines the reference runs at each instance's Z (sim_all_bler.py:42-72) for all instances at once: "rand"
    (rand_sdp_solver: `factor_random` then `round`, both keyed by probe_seed(seed, i, 0x40000 | m) with m the method's index in
    METHODS), "mgain" and "masso" (gm.MAX_GAIN / MAX_ASSO in the stable order: `gm`, one launch each).  source: a `BatchSolver` (the
    states it was built from) or a `(BatchSolver, BatchEnv)` pair (the states the environment holds: `round_env`, `BatchEnv.gm`).
    Zs: one slot count per instance; the solver's slot counts must be these for "rand" (its embedding is K x Z rank_radio).  Users
    left over are drawn from a generator keyed by the same seed.  The resident factors are replaced by "rand".
    methods may also name "spectral" (OPT_IN_METHODS; spectral_sdp_solver: `factor_spectral(Zs)` then `round`, keyed by
    probe_seed(seed, i, 0x40000 | 3)): the embedding is that of the states the batch was built from, also when the rounding goes
    against an environment; it replaces the resident factors too.  "mrand" (DEVICE_DRAW_METHODS; gm.MAX_RAND with its draws on the
    device: `gm_rand`, one launch, `nattempt_gm` attempts of which the first that leaves nobody over counts, else the last, keyed by
    probe_seed(seed, i, 0x40000 | 4)) touches no factor.
    Returns per instance {method: (z_vec float64[K], Z, remainder)}."""
    b, env = source if isinstance(source, tuple) else (source, None)
    B = b.B
    Zs = [int(z) for z in Zs]
    if len(Zs) != B:
        raise ValueError("baselines_many: one slot count per instance")
    out = [{} for _ in range(B)]
    for name in methods:
        if name not in ALL_METHODS:
            raise ValueError("baselines_many: method must be one of %s, got %r" % (ALL_METHODS, name))
        m = ALL_METHODS.index(name)
        seeds = np.array([probe_seed(seed, i, 0x40000 | m) for i in range(B)], dtype=np.uint64)
        if name in ("rand", "spectral"):
            if any(b.sizes[i]["Z"] != Zs[i] for i in range(B)):
                raise ValueError("baselines_many: the batch's slot counts are not Zs (set_slots first)")
            if name == "rand":
                b.factor_random(seeds)
            else:
                b.factor_spectral(Zs)
            z, rem, used = b.round(nattempt_round, seeds) if env is None else b.round_env(env, nattempt_round, seeds)
            for i in range(B):
                out[i][name] = _finish(z, rem, used, i, Zs[i], int(seeds[i]))
        elif name == "mrand":
            z, rem, used = (b if env is None else env).gm_rand(Zs, seeds, nattempt_gm)
            for i in range(B):
                out[i][name] = _finish(z, rem, used, i, Zs[i], int(seeds[i]))
        else:
            slot, _, rem = (b if env is None else env).gm(m - 1, Zs, nattempt_gm)
            for i in range(B):
                out[i][name] = (_fill(slot[i], rem[i], Zs[i], int(seeds[i]))[0], Zs[i], int(rem[i]))
    return out


def _geometry(d):
    return (d.sta_locs, d.ap_locs) if hasattr(d, "sta_locs") else (np.asarray(d[0], dtype=np.float64), np.asarray(d[1], dtype=np.float64))


def compare_many(drops_or_geometries, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2, device=0, timings=None, split=None, factor_split=None, row_split=None, head_split=None,
                 warm_start=False, warm_fraction=1.0 / 3.0, methods=METHODS):
    """sim_all_bler.py:30-72 for many instances (`graphs.mobile_drop`s or (sta_locs, ap_locs) pairs): the MMW search
    (`search_many(..., epilogue="batch")`) on the states a `BatchEnv` generates, the three baselines at each instance's Z_fin
    (`baselines_many`) and one `BatchEnv.evaluate` per method.  Returns per instance {"Z", "probes", "bler": {"mmw", "rand",
    "mgain", "masso"}}.  timings: a dict that receives {"search_s", "baselines_s", "evaluate_s"}.  factor_split: workgroups per instance
    for the search's factors (`BatchSolver.set_factor_split`).  warm_start / warm_fraction go to the search and nowhere else.  methods:
    the baselines to run, METHODS or any of `baselines_many`'s names ("spectral", "mrand"); "bler" then holds "mmw" and these."""
    methods = tuple(methods)
    for name in methods:
        if name not in ALL_METHODS:
            raise ValueError("compare_many: method must be one of %s, got %r" % (ALL_METHODS, name))
    geo = [_geometry(d) for d in drops_or_geometries]
    B = len(geo)
    env = _lib.BatchEnv([g[1] for g in geo], [g[0].shape[0] for g in geo], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=device)
    b = None
    try:
        env.move([g[0] for g in geo])
        states = [env.state(i) for i in range(B)]
        t0 = time.perf_counter()
        found = search_many(states, nit=nit, eta=eta, seed=seed, nattempt=nattempt, rank_radio=rank_radio, device=device, epilogue="batch", split=split,
                            factor_split=factor_split, row_split=row_split, head_split=head_split, warm_start=warm_start, warm_fraction=warm_fraction)
        t1 = time.perf_counter()
        Zs = [int(r["Z"]) for r in found]
        b = _lib.BatchSolver(Zs, states, nit, eta, rank_radio=rank_radio, device=device)
        base = baselines_many((b, env), Zs, methods=methods, seed=seed, nattempt_round=nattempt)
        t2 = time.perf_counter()
        out = [{"Z": Zs[i], "probes": found[i]["probes"], "bler": {}} for i in range(B)]
        for name, zs in [("mmw", [r["z_vec"] for r in found])] + [(m, [base[i][m][0] for i in range(B)]) for m in methods]:
            _, bler = env.evaluate(zs, Zs)
            for i in range(B):
                out[i]["bler"][name] = bler[i]
        if timings is not None:
            timings.update(search_s=t1 - t0, baselines_s=t2 - t1, evaluate_s=time.perf_counter() - t2)
        return out
    finally:
        if b is not None:
            b.close()
        env.close()


def online_greedy_many(drops, n_points=11, step_us=1e6, mob_spd_meter_s=0.1, resolution_us=1e4, seed=0, device=0, timings=None, methods=("mgain",)):
    """The greedy arm of the reference's online comparison (sim_mmw_online_cmp_methods.py:79-88) for many `graphs.mobile_drop`s:
    MAX_GAIN.run(-1, not_Z_bound=True) once on the drops' states (`BatchEnv.move`, `BatchEnv.gm(0, Z <= 0)`; users left over drawn
    from [0, ZZ), keyed by probe_seed(seed, i, 0x40000 | 1)), then per time point the state where the stations are now (`move`),
    `evaluate` of that ONE colouring with Z = ZZ, and every drop walks `step_us` microseconds (one value or one per instance) in
    `resolution_us` steps.  The drops are moved in place.
    Returns per instance {"Z", "probes": [], "z_vec": [n_points, K], "remainder": [n_points], "bler": [n_points, K]} (the colouring
    repeated per point: `online_many`'s shape); timings as there.
    methods: ("mgain",) is that arm alone.  Naming "mrand" beside it adds gm.MAX_RAND with its draws on the device
    (`BatchEnv.gm_rand`, one attempt, keyed by probe_seed(seed, i, 0x40000 | 4)) once on the drops' states at the greedy's slot count
    ZZ, scored at every point like the greedy's colouring: out[i]["mrand"] = {"z_vec", "remainder", "bler"} in the same shapes."""
    methods = tuple(methods)
    for name in methods:
        if name not in ("mgain", "mrand"):
            raise ValueError("online_greedy_many: method must be one of %s, got %r" % (("mgain", "mrand"), name))
    if "mgain" not in methods:
        raise ValueError("online_greedy_many: methods must name 'mgain' (its slot count is the one 'mrand' colours with), got %r" % (methods,))
    B = len(drops)
    steps = [float(x) for x in np.broadcast_to(np.asarray(step_us, dtype=np.float64), (B,))]
    env = _lib.BatchEnv([d.ap_locs for d in drops], [d.K for d in drops], min_sinr=min_sinr_dec(), noise_floor_dbm=_NOISE_FLOOR_DBM, device=device)
    try:
        env.move([d.sta_locs for d in drops])
        slot, ZZ, rem = env.gm(0, 0)
        Zs = [int(z) for z in ZZ]
        zv = [_fill(slot[i], rem[i], Zs[i], probe_seed(seed, i, 0x40000 | 1))[0] for i in range(B)]
        out = [{"Z": Zs[i], "probes": [], "z_vec": np.tile(zv[i], (n_points, 1)), "remainder": np.full(n_points, int(rem[i]), dtype=np.int64),
                "bler": np.empty((n_points, drops[i].K))} for i in range(B)]
        zr = None
        if "mrand" in methods:
            keys = np.array([probe_seed(seed, i, 0x40000 | ALL_METHODS.index("mrand")) for i in range(B)], dtype=np.uint64)
            got = env.gm_rand(Zs, keys, 1)
            fin = [_finish(*got, i, Zs[i], int(keys[i])) for i in range(B)]
            zr = [f[0] for f in fin]
            for i in range(B):
                out[i]["mrand"] = {"z_vec": np.tile(zr[i], (n_points, 1)), "remainder": np.full(n_points, fin[i][2], dtype=np.int64),
                                   "bler": np.empty((n_points, drops[i].K))}
        for p in range(n_points):
            t0 = time.perf_counter()
            env.move([d.sta_locs for d in drops])
            _, bler = env.evaluate(zv, Zs)
            for i in range(B):
                out[i]["bler"][p] = bler[i]
            if zr is not None:
                _, bler = env.evaluate(zr, Zs)
                for i in range(B):
                    out[i]["mrand"]["bler"][p] = bler[i]
            t1 = time.perf_counter()
            for d, t in zip(drops, steps):
                d.step_time(t, mob_spd_meter_s, resolution_us)
            if timings is not None:
                timings.append({"device_s": t1 - t0, "step_s": time.perf_counter() - t1})
        return out
    finally:
        env.close()


class single:
    """The reference's solver protocol (run_with_state / rounding, binary_search_relaxation.py:50-53) for ONE state on a batch of
    one, with search_many's seeds: `binary_search_relaxation` driven by it probes what search_many probes for instance `index`
    (with the same warm_start / warm_fraction too)."""

    def __init__(self, state, index=0, nit=150, eta=0.04, seed=0, nattempt=10, rank_radio=2, device=0, epilogue="handle", split=None, factor_split=None, row_split=None, head_split=None,
                 warm_start=False, warm_fraction=1.0 / 3.0):
        _check_warm(warm_fraction)
        self.warm_start, self.warm_fraction = bool(warm_start), float(warm_fraction)
        self.iters = []  # the iterations of every probe, in order
        self.state, self.index, self.nit, self.eta, self.seed = state, int(index), int(nit), float(eta), int(seed)
        self.nattempt, self.rank_radio, self.device = int(nattempt), int(rank_radio), int(device)
        _factor_split(None, factor_split, _check_epilogue(epilogue))
        self._in_batch = _check_epilogue(epilogue) and state[0].shape[0] <= _lib.BATCH_EPILOGUE_MAX_K
        self.probes = []
        self._b = None
        self._split = split
        self._row_split = row_split
        self._head_split = head_split
        self._factor_split = factor_split
        self._hs = _Handles([state], self.nit, self.eta, self.rank_radio, self.device)

    def run_with_state(self, bs_iteration, Z, state):
        Z = int(Z)
        if self._b is None:
            self._b = _lib.BatchSolver([Z], [state], self.nit, self.eta, rank_radio=self.rank_radio, device=self.device)
            _split(self._b, self._split)
            _row_split(self._b, self._row_split)
            _head_split(self._b, self._head_split)
            _factor_split(self._b, self._factor_split)
        warm = self.warm_start and len(self.probes) > 0  # as search_many: the first probe cold, every later one from its predecessor
        n = warm_iterations(self.nit, self.warm_fraction) if warm else self.nit
        self._b.set_slots([Z], n, warm=warm)
        self._b.iterate(n, None, [probe_seed(self.seed, self.index, len(self.probes))])
        self.iters.append(n)
        if self._in_batch:
            self._b.factor()
            return True, self._b.read_factor(0)
        self._h = self._hs.get(0, Z)
        return True, _factor(self._b, 0, self._h, Z, self.rank_radio, 0)

    def rounding(self, Z, gX, state):
        if self._in_batch:  # the factor `run_with_state` just made is resident in the batch: gX is its copy
            sd = probe_seed(self.seed, self.index, len(self.probes))
            z_vec, Z, rem = _finish(*self._b.round(self.nattempt, [sd]), 0, int(Z), sd)
            self.probes.append(int(Z))
            return z_vec, Z, rem
        z_vec, Z, rem = _round(self._h, int(Z), gX, state, probe_seed(self.seed, self.index, len(self.probes)), self.nattempt)
        self.probes.append(int(Z))
        return z_vec, Z, rem

    def close(self):
        self._hs.close()
        if self._b is not None:
            self._b.close()
            self._b = None
