"""CPU restatement of a probe carried across two states, composed from the public pieces of oracle.mmw_oracle -- TEST INFRASTRUCTURE.

The stations have moved: the second state has the same K users, another L / X pattern and other association pairs.  What is
carried from the first probe's iterate is (e_accu, lval, xval, Y), re-indexed by keys and not by merging rows, so that this helper
shares no method with the library's host code:
  lval, xval   by row * K + col on the two `orc.Pattern`s; an entry the old pattern does not store is 0
  e_accu, Y    [D-part K | F-part E_asso | H-part K]: the D- and the H-part by user, the F-part by asso_x * K + asso_y; a pair the
               old state does not have is 0
Y is not renormalised.  The sums restart at zero and follow the convention of tests/helpers/warm_oracle.py, whose iteration loop
this module runs.  The state pairs the carry's tests share are built here too.
"""
import os
import sys

import numpy as np
import scipy.sparse

from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warm_oracle  # noqa: E402


def _lookup(old_keys, new_keys):
    """Position of every new key in `old_keys` (sorted or not), -1 where it is absent."""
    where = {int(k): i for i, k in enumerate(old_keys)}
    return np.array([where.get(int(k), -1) for k in new_keys], dtype=np.int64)


def maps(p_old, p_new):
    """(lmap[nnzL_new], cmap[C_new]): positions in the old value arrays / constraint vector, -1 where the old state has none."""
    assert p_old.K == p_new.K
    K = p_new.K
    lmap = _lookup(p_old.row * K + p_old.col, p_new.row * K + p_new.col)
    f = _lookup(p_old.asso_x * K + p_old.asso_y, p_new.asso_x * K + p_new.asso_y)
    f = np.where(f >= 0, f + K, -1)
    cmap = np.concatenate([np.arange(K), f, K + p_old.E_asso + np.arange(K)]).astype(np.int64)
    return lmap, cmap


def gather(v, m):
    """v[m] with -1 read as 0."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(m.size)
    out[m >= 0] = v[m[m >= 0]]
    return out


def carry(p_old, st, p_new):
    """The iterate `st` (a dict with lval, xval, Y, e_accu on `p_old`) mapped onto `p_new`; the sums restart."""
    lmap, cmap = maps(p_old, p_new)
    return {"lval": gather(st["lval"], lmap), "xval": gather(st["xval"], lmap), "Y": gather(st["Y"], cmap), "e_accu": gather(st["e_accu"], cmap),
            "xsum": np.zeros(p_new.nnzL), "ysum": np.zeros(p_new.C)}


def run(Z1, n1, state1, Z2, n2, state2, eta, sketch1, sketch2, rank_radio=2, expm=orc.expm_half):
    """n1 iterations at Z1 on state1 from the initial point, the carry, n2 iterations at Z2 on state2.  sketch1(i, K, D1) /
    sketch2(i, K, D2) as in warm_oracle.run.  Returns the final iterate and the sums (lval, xval, Y, e_accu, e_this, X_half, xsum,
    ysum) and the second pattern as "pattern"."""
    p1 = orc.Pattern(Z1, state1)
    xval = np.zeros(p1.nnzL)
    xval[p1.diag_pos] = 1.0
    st = {"Y": np.ones(p1.C) / p1.C, "e_accu": np.zeros(p1.C), "lval": np.zeros(p1.nnzL), "xval": xval, "xsum": np.zeros(p1.nnzL), "ysum": np.zeros(p1.C)}
    st = warm_oracle._iterate(p1, st, eta, sketch1, 0, n1, Z1 * rank_radio, expm)
    p2 = orc.Pattern(Z2, state2)
    st = carry(p1, st, p2)
    st = warm_oracle._iterate(p2, st, eta, sketch2, 0, n2, Z2 * rank_radio, expm)
    st["pattern"] = p2
    return st


# ---- the state pairs ---------------------------------------------------------------------------------------------------------------
PAIR_A_SEED = 3  # mobile_drop(5, 75e-4, 3): the test asserts on the CPU that this seed loses and gains L entries and pairs


def moved_pair(cell, seed, speed=3.0, t_us=1e6):
    """(state before, state after) of mobile_drop(cell, 75e-4, seed) walking `t_us` microseconds at `speed` m/s."""
    from sig_sdp_mmw_amd.graphs import mobile_drop
    d = mobile_drop(cell, 75e-4, seed)
    before = d.state()
    d.step_time(t_us, speed)
    return before, d.state()


def _state(K, gains, pairs, h):
    S = scipy.sparse.lil_matrix((K, K))
    for (a, b), v in gains.items():
        S[a, b] = v
    Q = scipy.sparse.lil_matrix((K, K))
    for a, b in pairs:
        Q[a, b] = Q[b, a] = 1.0
    return scipy.sparse.csr_matrix(S), scipy.sparse.csr_matrix(Q), np.asarray(h, dtype=np.float64)


def pair_b():
    """K = 4: users {0,1} | {2,3} re-associate to {0,2} | {1,3}; the one gain edge moves from (0,3) to (1,2), so the two L patterns
    share only the diagonal."""
    h = [1.5, 1.75, 2.0, 2.25]
    return (_state(4, {(0, 3): 0.3, (3, 0): 0.2}, [(0, 1), (2, 3)], h), _state(4, {(1, 2): 0.25, (2, 1): 0.35}, [(0, 2), (1, 3)], h))


def pair_c(which):
    """K = 2: "lose" has the one pair (0,1) before and a gain edge in its place after (E_asso 1 -> 0), "gain" the other way round."""
    h = [1.5, 2.0]
    one, none = _state(2, {}, [(0, 1)], h), _state(2, {(0, 1): 0.3, (1, 0): 0.2}, [], h)
    return (one, none) if which == "lose" else (none, one)
