"""The cases of the online-sweep tests on the solver handle (test_hip_online_handle.py, test_online_handle_host.py): three
`graphs.mobile_drop`s at rho = 75e-4, each moved once by `step_time(1e6, 3.0, 1e5)`, with the slot count their roundings use.
Host-side only: positions, the NumPy restatement of the generator at them, the deterministic factor the rounding tests share."""
import functools

import numpy as np

from sig_sdp_mmw_amd import scorer
from sig_sdp_mmw_amd.graphs import _state_at, mobile_drop

RHO = 75e-4
MIN_S_N_RATIO = 0.1
# name: (cell, seed, K, Z for the rounding)
CASES = {"k75": (5, 3, 75, 6), "k192": (8, 0, 192, 9), "k1083": (19, 1, 1083, 14)}
NAMES = list(CASES)


def drop(name):
    cell, seed, K, _ = CASES[name]
    d = mobile_drop(cell, RHO, seed)
    assert d.K == K
    return d


@functools.lru_cache(maxsize=None)
def positions(name):
    """(ap_locs, station positions before the walk, after it): read-only arrays."""
    d = drop(name)
    p0 = d.sta_locs.copy()
    d.step_time(1e6, 3.0, 1e5)
    p1 = d.sta_locs.copy()
    for a in (d.ap_locs, p0, p1):
        a.setflags(write=False)
    return d.ap_locs, p0, p1


@functools.lru_cache(maxsize=None)
def host_state(name, moved):
    """`drop.state()` at the old (moved = 0) or the new (1) positions."""
    ap, p0, p1 = positions(name)
    return _state_at(p1 if moved else p0, ap)[0]


def cut_margin(name, moved):
    """min |rx / min_s_n_ratio - 1| over all (station, AP) pairs: how far the nearest receive power lies from the threshold that
    decides the sparsity pattern (the device's pow and NumPy's may differ in the last bits)."""
    ap, p0, p1 = positions(name)
    rx = scorer.receive_power(p1 if moved else p0, ap)
    return float(np.min(np.abs(rx / MIN_S_N_RATIO - 1.0)))


@functools.lru_cache(maxsize=None)
def factor(name):
    """A deterministic K x 2Z factor with distinct row norms: unit rows of normals scaled by 1 - k 2^-32
    (`rand_sdp_solver.index_ordered`), so the visiting order does not hang on last-bit noise."""
    _, _, K, Z = CASES[name]
    g = np.random.default_rng(1000 + K).standard_normal((K, 2 * Z))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g *= (1.0 - np.arange(K) * 2.0 ** -32)[:, None]
    g.setflags(write=False)
    return g


def randv(name, draw):
    """Projection draw `draw` of a case: Z x 2Z normals, rows normalised (sdp_solver.py:48-49)."""
    _, _, K, Z = CASES[name]
    r = np.random.default_rng(7000 + 10 * K + draw).standard_normal((Z, 2 * Z))
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def oracle_slots(orc, name, state, draw):
    """(slot int64[K] with -1 for users left over, remainder) of the oracle's `rounding_one_attempt` on `state`."""
    Z = CASES[name][3]
    z_vec, _, rem, un = orc.rounding_one_attempt(Z, np.asarray(factor(name)), state, randv(name, draw), randint=lambda Z_, size: np.zeros(size))
    return np.where(un, -1, z_vec).astype(np.int64), int(rem)
