"""The greedy baselines of the reference's `sim_src/alg/gm.py` on the device: MAX_GAIN, MAX_ASSO and MAX_RAND.

Same static `run` signatures and return values `(z_vec float64[K], ZZ, remainder)` as the reference (gm.py:9-200), and the same
draws from the global NumPy stream in the same order (the `randint` fill of users left over, MAX_RAND's two `randn` draws), so a
seeded script continues with the same stream.  The slot passes run in HIP kernels (`mmw_gm_*`, include/mmw_hip.h,
csrc/kernels_gm.h); the host forms the keys with the reference's own scipy expressions.

A device-resident state of a generator (`DeviceEnv.device_state()`) gets its handle built on the device (`GreedyHandle.from_env`)
and its keys from the handle itself (`GreedyHandle.key`): the state is never copied to the host.  A `DeviceState` of CSR
arrays still hands out its host copy.

MAX_RAND's `draws="device"` (opt-in) leaves NumPy's two `randn` draws out: the user order and the slot preferences are drawn,
ranked and used on the device (`GreedyHandle.rand`, mmw_gm_rand; csrc/kernels_gm_rand.h), keyed by one integer from the global stream.

Visiting order (MAX_GAIN / MAX_ASSO), chosen by the keyword `order` or the environment variable MMW_GM_ORDER:
  * "reference" (default): every slot visits the unassigned users in `kindx[np.argsort(-key[not_assigned])]`, evaluated on the
    host exactly as the reference does (gm.py:31-32); one device pass per slot.  On the same host this is the reference's result.
    NumPy's default argsort is not stable and breaks the many ties of these keys (users behind one AP) in an order that depends on
    its algorithm and the CPU's SIMD dispatch, so no device sort can reproduce it.
  * "stable": ties go to the lower user index (argsort(-key, kind="stable")); the order is ranked on the device once and every slot
    and attempt runs in one device call.  A deliberate deviation: the colouring can differ from the reference's wherever ties exist.
"""
import os
import warnings

import numpy as np

from . import _lib

ORDERS = ("reference", "stable")
DEVICE = 0  # HIP device of the handles; -1 runs the same procedures as host C++

_cache = {"key": None, "held": None, "handle": None}


def _order_mode(order):
    mode = order if order is not None else os.environ.get("MMW_GM_ORDER", "reference")
    if mode not in ORDERS:
        raise ValueError("gm visiting order must be one of %s, got %r" % (ORDERS, mode))
    return mode


def _on_env(state, device):
    """True for the device-resident state of a generator: its greedy handle is built where the state lies (device -1, the host C++
    procedures, still takes the host copy)."""
    return (DEVICE if device is None else int(device)) >= 0 and isinstance(state, _lib.DeviceState) and isinstance(state.env, _lib.DeviceEnv)


def _host_state(state):
    """The host triple: a device-resident state of CSR arrays hands out its host copy, made once (GreedyHandle takes host arrays)."""
    return state.host() if isinstance(state, _lib.DeviceState) else state


def _env_handle(state):
    """The greedy handle of a generator's device-resident state (`GreedyHandle.from_env`), reused while that very state is asked for."""
    if _cache["key"] == "env" and _cache["held"] is state and _cache["handle"] is not None:
        state.check()
        return _cache["handle"]
    if _cache["handle"] is not None:
        _cache["handle"].close()
        _cache["handle"] = None
    g = _lib.GreedyHandle.from_env(state.env)
    _cache.update(key="env", handle=g, held=state)
    return g


def _state_key(state, device):
    S, Q, h = state
    return (int(device), S.shape[0], S.nnz, Q.nnz, float(S.data[:8].sum()) if S.nnz else 0.0, int(S.indices[:8].sum()) if S.nnz else 0,
            float(np.asarray(h)[:8].sum()))


def _handle(state, device=None):
    """The greedy handle of `state`, reused while the state's content is unchanged (the reference re-reads it every call)."""
    device = DEVICE if device is None else int(device)
    S, Q, h = state
    key = _state_key(state, device)
    held = _cache["held"]
    if _cache["key"] == key and held is not None:
        (sp0, si0, sx0), (qp0, qi0, qx0), h0 = held
        if np.array_equal(S.indptr, sp0) and np.array_equal(S.indices, si0) and np.array_equal(S.data, sx0) and \
                np.array_equal(Q.indptr, qp0) and np.array_equal(Q.indices, qi0) and np.array_equal(Q.data, qx0) and np.array_equal(np.asarray(h), h0):
            return _cache["handle"]
    if _cache["handle"] is not None:
        _cache["handle"].close()
        _cache["handle"] = None
    g = _lib.GreedyHandle(state, device=device)
    _cache.update(key=key, handle=g, held=((S.indptr.copy(), S.indices.copy(), S.data.copy()), (Q.indptr.copy(), Q.indices.copy(), Q.data.copy()),
                                           np.array(h, dtype=np.float64)))
    return g


def _gain_key(state):
    """S_sum of gm.py:11-18: column sums of S_gain with the diagonal zeroed, by the reference's expression."""
    S_gain = state[0].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (setdiag on a CSR without stored diagonal: scipy's efficiency warning)
        S_gain.setdiag(0)
    return np.asarray(S_gain.transpose().sum(axis=1)).ravel()


def _asso_key(state):
    """A_sum of gm.py:81."""
    return np.asarray(state[1].sum(axis=1)).ravel()


def _slot_major(kind, Z, state, nattempt, not_Z_bound, order, device):
    if _on_env(state, device):  # the handle and the key where the state lies (mmw_gm_create_from_env, mmw_gm_key): bitwise the host expressions below
        g = _env_handle(state)
        K, key = g.K, g.key(kind)
    else:
        state = _host_state(state)
        K = state[0].shape[0]
        g = _handle(state, device)
        key = _asso_key(state) if kind else _gain_key(state)
    if not_Z_bound:
        Z = K
    if _order_mode(order) == "stable":
        slot, ZZ, _ = g.run(key, Z, nattempt)
        not_assigned = slot < 0
        z_vec = np.where(not_assigned, 0, slot).astype(np.float64)
    else:
        not_assigned = np.ones(K, dtype=bool)
        z_vec = np.zeros(K)
        ZZ = 0
        for z in range(Z):
            ZZ += 1
            kindx = np.arange(K)[not_assigned]
            krank = kindx[np.argsort(-key[not_assigned])]
            k_list_z = g.pass_(krank, nattempt)
            if k_list_z.size == 0:  # nothing changes, so every remaining slot accepts nobody either: the reference enters them all
                ZZ = Z
                break
            z_vec[k_list_z] = z
            not_assigned[k_list_z] = False
            if not not_assigned.any():
                break
    if not_assigned.any():  # gm.py:60-64
        z_vec[not_assigned] = np.random.randint(ZZ if not_Z_bound else Z, size=int(not_assigned.sum()))
    return z_vec, ZZ, np.sum(not_assigned)


class MAX_GAIN:
    """gm.MAX_GAIN (gm.py:6-66): slots filled one after another, users by descending interference they cause."""

    @staticmethod
    def run(Z, state, nattempt=1, not_Z_bound=False, order=None, device=None):
        return _slot_major(0, Z, state, nattempt, not_Z_bound, order, device)


class MAX_ASSO:
    """gm.MAX_ASSO (gm.py:69-127): the same procedure, users by descending AP population."""

    @staticmethod
    def run(Z, state, nattempt=1, not_Z_bound=False, order=None, device=None):
        return _slot_major(1, Z, state, nattempt, not_Z_bound, order, device)


class MAX_RAND:
    """gm.MAX_RAND (gm.py:131-200): random user order, random slot preference, the rounding's user-major greedy."""

    @staticmethod
    def run(Z, state, nattempt=1, device=None, draws="host", seed=None):
        """draws="host" (default): the two `randn` draws of gm.py:148-150 from NumPy's global stream, sorted on the host and uploaded.
        draws="device": `GreedyHandle.rand` -- the order keys and the preference values are drawn, ranked and used where the state
        lies (include/mmw_hip.h, mmw_gm_rand), `nattempt` attempts of which the first that leaves nobody over counts, else the last;
        `seed` keys the draw, None takes one 64-bit integer from NumPy's global stream, so a seeded script stays reproducible.  The fill
        of users left over stays `np.random.randint` either way."""
        if draws not in ("host", "device"):
            raise ValueError("MAX_RAND draws must be 'host' or 'device', got %r" % (draws,))
        if _on_env(state, device):
            g = _env_handle(state)
            K = g.K
        else:
            state = _host_state(state)
            K = state[0].shape[0]
            g = _handle(state, device)
        if draws == "device":
            if seed is None:
                seed = int(np.random.randint(0, 1 << 64, dtype=np.uint64))
            slot, _, _ = g.rand(Z, max(1, int(nattempt)), int(seed))
        else:
            inprod = np.random.randn(Z, K)  # gm.py:148-150, same draws in the same order
            sorted_indices = np.argsort(-inprod, axis=0)
            rank = np.argsort(np.random.randn(K))
            slot, _ = g.assign(rank, np.ascontiguousarray(sorted_indices.T))
        not_assigned = slot < 0
        z_vec = np.where(not_assigned, 0, slot).astype(np.float64)
        if not_assigned.any():  # gm.py:196-199
            z_vec[not_assigned] = np.random.randint(Z, size=int(not_assigned.sum()))
            print(z_vec[not_assigned])
        return z_vec, Z, np.sum(not_assigned)
