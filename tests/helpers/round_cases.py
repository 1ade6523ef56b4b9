"""Designed instances for the handle's rounding (mmw_round) and the CPU reference they are compared with.  Plain NumPy/SciPy.

`reference_attempt` restates `oracle.mmw_oracle.rounding_one_attempt` with the documented tie rules made executable (both sorts
are stable on the negated keys: ties go to the lower user index in the visiting order and to the lower slot in a preference
list; `np.argsort`'s default is not stable) and with a trace of what every user's walk through its preference list met.  The three
checks of one user are evaluated for all slots at once -- nothing changes between two probes of the same user -- and the
sums are formed like the oracle's, one add per address and assignment, in assignment order.

Every builder returns `(state, Z, gX, randv)` with `randv` of shape (nbatch, Z, D').  Where a tie or an exact threshold decides
the output, the inputs are small integers or dyadic fractions: every product, every sum in any order and every argument of a
square root is then exact in float64, the device's projection and norms equal NumPy's bit for bit, and only the rule is under
test.  The sizes are the smallest that reach the path named in each builder (kernels_round.h: GB_NP = GB_NE = 4 register
chunks of 64, 64 prefetched same-AP partners, RANK_SPLIT = 16 groups of 256-key tiles, GS_W = 32, GS_CHUNK = 8192).
"""
import numpy as np
import scipy.sparse

CHECK_A, CHECK_B, CHECK_C = 1, 2, 3  # own sum over h_max; a member's sum over its h_max; a member on the same AP


# --------------------------------------------------------------------------------------------
# the reference
# --------------------------------------------------------------------------------------------
def _out_lists(S_gain):
    S = scipy.sparse.csr_matrix(S_gain).astype(np.float64).copy()
    S.setdiag(0)
    S.eliminate_zeros()
    S.sort_indices()
    return S


def stable_desc(key, axis=0, ties="lower"):
    """argsort of -key along `axis`; equal keys by lower index (`ties="lower"`, the documented rule) or by higher index."""
    key = np.asarray(key, dtype=np.float64)
    if ties == "lower":
        return np.argsort(-key, axis=axis, kind="stable")
    n = key.shape[axis]
    return n - 1 - np.argsort(-np.flip(key, axis=axis), axis=axis, kind="stable")


class Trace:
    """What the reference run met.  `order`: the visiting order.  Per user k: `depth[k]`, the number of slots it walked past
    (Z if it stayed out); `rejected[k]`, a list of (slot, check, positions) in walking order, where `check` is the first of
    CHECK_A / CHECK_B / CHECK_C that ruled the slot out and `positions` are, for CHECK_B, the positions in k's sorted out-list
    whose members would exceed their h_max, and for CHECK_C the positions in k's Q list that sit in the slot."""

    def __init__(self, K, order, deg, qdeg):
        self.order, self.deg, self.qdeg = order, deg, qdeg
        self.depth = np.zeros(K, dtype=np.int64)
        self.rejected = [()] * K

    def rejections(self, check=None):
        for k, rej in enumerate(self.rejected):
            for z, c, pos in rej:
                if check is None or c == check:
                    yield k, z, c, pos


def reference_attempt(Z, gX, state, randv, order_ties="lower", pref_ties="lower", order=None, drop_adds=None):
    """One rounding attempt.  Returns (z int64[K] with -1 = unassigned, remainder, Trace).

    `order_ties` / `pref_ties`: "lower" is the rule; "higher" breaks the ties the other way (to show that a case depends on it).
    `order`: a visiting order to use instead of the sorted norms (to show that a case depends on an interacting pair's order).
    `drop_adds`: {user: p}: the additions of that user from positions >= p of its out-list are left out (to show that a later
    decision depends on them)."""
    S_gain, Q_asso, h_max = state
    h_max = np.asarray(h_max, dtype=np.float64)
    gX = np.asarray(gX, dtype=np.float64)
    randv = np.asarray(randv, dtype=np.float64)
    K = S_gain.shape[0]
    S = _out_lists(S_gain)
    Q = scipy.sparse.csr_matrix(Q_asso)
    Q.sort_indices()
    if order is None:
        order = stable_desc(np.linalg.norm(gX, axis=1), 0, order_ties)   # sdp_solver.py:51
    inprod = np.matmul(randv, gX.transpose())                            # :56
    pref = np.ascontiguousarray(stable_desc(inprod, 0, pref_ties).T)     # :57, one row per user
    slot = np.full(K, -1, dtype=np.int64)
    gain_sum = np.zeros((K, Z))                                           # [n][z]
    tr = Trace(K, np.asarray(order), np.diff(S.indptr), np.diff(Q.indptr))
    drop_adds = drop_adds or {}
    for k in order:
        nb = S.indices[S.indptr[k]:S.indptr[k + 1]]
        gv = S.data[S.indptr[k]:S.indptr[k + 1]]
        qn = Q.indices[Q.indptr[k]:Q.indptr[k + 1]]
        nb_slot, qn_slot = slot[nb], slot[qn]
        bad_a = gain_sum[k] > h_max[k]                                    # (a): n = k, tmp_h[k] = 0 (:78-84)
        placed = np.flatnonzero(nb_slot >= 0)
        over = placed[gain_sum[nb[placed], nb_slot[placed]] + gv[placed] > h_max[nb[placed]]]  # (b)
        bad_b = np.zeros(Z, dtype=bool)
        bad_b[nb_slot[over]] = True
        same_ap = np.flatnonzero(qn_slot >= 0)                            # (c): asso_sum[z][k] >= 1 (:86-92)
        bad_c = np.zeros(Z, dtype=bool)
        bad_c[qn_slot[same_ap]] = True
        ok = ~(bad_a | bad_b | bad_c)[pref[k]]
        depth = int(np.argmax(ok)) if ok.any() else Z
        tr.depth[k] = depth
        if depth:
            rej = []
            for z in pref[k, :depth]:
                if bad_a[z]:
                    rej.append((int(z), CHECK_A, ()))
                elif bad_b[z]:
                    rej.append((int(z), CHECK_B, tuple(int(p) for p in over[nb_slot[over] == z])))
                else:
                    rej.append((int(z), CHECK_C, tuple(int(p) for p in same_ap[qn_slot[same_ap] == z])))
            tr.rejected[k] = rej
        if depth < Z:
            z = pref[k, depth]
            n_add = min(nb.size, drop_adds.get(int(k), nb.size))
            gain_sum[nb[:n_add], z] += gv[:n_add]                         # :94, assignment order = accumulation order
            slot[k] = z
    return slot, int((slot < 0).sum()), tr


# --------------------------------------------------------------------------------------------
# building blocks
# --------------------------------------------------------------------------------------------
def _csr(K, rows, cols, vals):
    m = scipy.sparse.csr_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=(K, K))
    m.sum_duplicates()
    m.sort_indices()
    return m


def _sym01(K, a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    m = _csr(K, np.concatenate([a, b]), np.concatenate([b, a]), np.ones(2 * a.size))
    m.data[:] = 1.0
    return m


def _with_diag(K, rows, cols, vals, own=2.0):
    return _csr(K, np.concatenate([rows, np.arange(K)]), np.concatenate([cols, np.arange(K)]),
                np.concatenate([vals, np.full(K, own)]))


def _ranked(prefs, Z):
    """Rows whose descending order is `prefs` (one permutation of the Z slots per row): entry Z - rank at each slot."""
    prefs = np.asarray(prefs, dtype=np.int64)
    v = np.empty(prefs.shape, dtype=np.float64)
    np.put_along_axis(v, prefs, np.broadcast_to(np.arange(Z, 0, -1, dtype=np.float64), prefs.shape), axis=1)
    return v


def _perms(rng, n, Z, first=None):
    p = np.argsort(rng.random((n, Z)), axis=1)
    if first is not None:  # move the wanted slot to the front
        first = np.broadcast_to(np.asarray(first, dtype=np.int64), (n,))
        for i in range(n):
            j = int(np.flatnonzero(p[i] == first[i])[0])
            p[i, 0], p[i, j] = p[i, j], p[i, 0]
    return p


def normalise(r):
    return r / np.linalg.norm(r, axis=-1, keepdims=True)


# --------------------------------------------------------------------------------------------
# preference window / association window
# --------------------------------------------------------------------------------------------
def shared_order_clique(m, Z, signs="pos", seed=0, nbatch=1):
    """One access point with `m` users (Q complete on them, so qdeg = m - 1), D' = 1.  |gX[k]| are distinct integers and
    randv[z] = Z - z is strictly decreasing, so every user with gX[k] > 0 prefers the slots 0, 1, 2, ... and every user with
    gX[k] < 0 the slots Z-1, Z-2, ...: the j-th visited user of one sign walks past exactly the j slots its predecessors took
    (check (c)), and the walked depths cover 0 .. m-1 -- every chunk of the preference window and the rows beyond it.
    Five more users lie outside the clique.  Two exchange a gain of 1/4 and are visited last.  The other three prefer the slots
    Z-1, Z-2, ...: m+2 is visited first, takes Z-1 and emits 1/2 to m+3 and m+4; m+3 (h_max = 1/4, visited after a hundred clique
    users) is kept out of Z-1 >= 256 by check (a) on its own row; m+4 (h_max = 1, a hundred users later) takes Z-1 -- unless the
    flags of the slots beyond the register window were left over from m+3, which the same wavefront decided.
    `nbatch` > 1 adds draws whose slot order is a fixed permutation of that one (batch entries must not mix)."""
    rng = np.random.default_rng(seed)
    K = m + 5
    a, b = np.triu_indices(m, 1)
    Q = _sym01(K, a, b)
    S = _with_diag(K, np.array([m, m + 1, m + 2, m + 2]), np.array([m + 1, m, m + 3, m + 4]), np.array([0.25, 0.25, 0.5, 0.5]))
    h_max = np.ones(K)
    h_max[m + 3] = 0.25
    mag = np.empty(K)
    mag[:m] = rng.permutation(m) + 3.0                       # 3 .. m + 2
    mag[m:] = [2.0, 1.0, m + 100.0, m - 97.5, m - 197.5]     # half-integers: between two clique users
    sign = np.ones(K)
    sign[m + 2:] = -1.0
    if signs == "mixed":
        sign[:m] = np.where(rng.random(m) < 0.5, -1.0, 1.0)
    gX = (mag * sign)[:, None]
    rv = np.empty((nbatch, Z, 1))
    rv[0, :, 0] = Z - np.arange(Z)
    for a_ in range(1, nbatch):
        rv[a_, :, 0] = rng.permutation(Z) + 1.0
    return (S, Q, h_max), Z, gX, rv


# --------------------------------------------------------------------------------------------
# neighbour window
# --------------------------------------------------------------------------------------------
HUB_DEGS = (256, 257, 300, 700)


def hubs_and_leaves(seed=0, nbatch=1):
    """Four hubs with out-degree 256, 257, 300 and 700 into leaves, every gain 1/2, Z = D' = 8 and randv[0] the identity, so
    that gX[k] spells out k's preference list.  The leaves have the larger norms: they are visited first and each takes its
    first slot.  Then the hubs, in this order, and last the leaf W:
      hub 0 (256: the register window exactly): its first slot holds the leaf at position 255, whose h_max = 1/4;
      hub 1 (257): its first slot holds the leaf at position 256 with h_max = 1/4 -- the one element of the re-read loop;
      hub 2 (300): its first slot is ruled out by position 299 alone; it takes its second slot t and adds 1/2 to all its leaves;
      hub 3 (700): lists positions 256 .. 275 of hub 2 as well.  Two of them (260, 270) sit in t with h_max = 3/4: the 1/2 hub 2
        added there from beyond its register window rules t out for hub 3.  Its second slot is ruled out by position 699 alone.
      W is position 290 of hub 2's list, h_max[W] = 1/4, and prefers t: check (a) on its own row reads hub 2's addition.
    `info` (the last element returned by `hubs_and_leaves_info`) names these users."""
    return hubs_and_leaves_info(seed, nbatch)[:4]


def hubs_and_leaves_info(seed=0, nbatch=1):
    rng = np.random.default_rng(seed)
    Z = 8
    K = 1500
    users = rng.permutation(K)
    hubs = np.sort(users[:4])
    rest = users[4:]
    sizes = (256, 257, 300, 680)
    lists, pos = [], 0
    for s in sizes:
        lists.append(np.sort(rest[pos:pos + s]))
        pos += s
    free = rest[pos:]
    lists[3] = np.sort(np.concatenate([lists[3], lists[2][256:276]]))
    assert tuple(len(x) for x in lists) == HUB_DEGS
    rows = np.concatenate([np.full(len(x), h) for h, x in zip(hubs, lists)])
    cols = np.concatenate(lists)
    S = _with_diag(K, rows, cols, np.full(rows.size, 0.5))
    # Q: the leaves outside every list pair up (the state needs association edges; they decide nothing here)
    Q = _sym01(K, free[0:-1:2], free[1::2])
    h_max = np.ones(K)
    # hubs' preference lists
    hub_pref = np.array([[0, 1, 2, 3, 4, 5, 6, 7],
                         [3, 4, 5, 6, 7, 0, 1, 2],
                         [5, 2, 6, 7, 0, 1, 3, 4],
                         [2, 6, 1, 0, 3, 4, 5, 7]])
    t = int(hub_pref[2, 1])
    assert hub_pref[3, 0] == t
    first = rng.integers(0, Z, size=K)
    tight = {int(lists[0][255]): int(hub_pref[0, 0]), int(lists[1][256]): int(hub_pref[1, 0]), int(lists[2][299]): int(hub_pref[2, 0]),
             int(lists[3][699]): int(hub_pref[3, 1])}
    for n, z in tight.items():
        h_max[n], first[n] = 0.25, z
    shared = [int(lists[2][260]), int(lists[2][270])]
    for n in shared:
        h_max[n], first[n] = 0.75, t
    W = int(lists[2][290])
    h_max[W], first[W] = 0.25, t
    assert len(set(tight) | set(shared) | {W}) == 7, "the named leaves must be seven different users: choose another seed"
    # every other leaf keeps h_max = 1, which no sum of two gains of 1/2 exceeds
    prefs = _perms(rng, K, Z, first=first)
    prefs[hubs] = hub_pref
    scale = np.empty(K)
    scale[rest] = rng.permutation(rest.size) + 10.0       # leaves first ...
    scale[hubs] = [8.0, 7.0, 6.0, 5.0]                    # ... the hubs in this order ...
    scale[W] = 1.0                                        # ... and W last
    gX = _ranked(prefs, Z) * scale[:, None]
    rv = np.empty((nbatch, Z, Z))
    rv[0] = np.eye(Z)
    for a in range(1, nbatch):
        rv[a] = np.eye(Z)[rng.permutation(Z)] if a == 1 else np.round(4 * rng.standard_normal((Z, Z))) / 4
    info = {"hubs": [int(h) for h in hubs], "lists": lists, "t": t, "shared": shared, "W": W, "tight": tight, "hub_pref": hub_pref}
    return (S, Q, h_max), Z, gX, rv, info


# --------------------------------------------------------------------------------------------
# ties
# --------------------------------------------------------------------------------------------
_NORM3 = np.array([[3, 0, 0], [0, 3, 0], [0, 0, 3], [-3, 0, 0], [0, -3, 0], [0, 0, -3],
                   [1, 2, 2], [2, 1, 2], [2, 2, 1], [-1, 2, 2], [2, -1, 2], [2, 2, -1],
                   [1, -2, 2], [-2, 1, 2], [2, -2, 1], [-1, -2, -2], [-2, -1, -2], [-2, -2, -1]], dtype=np.float64)  # all of 2-norm 3

TIE_CASES = ("mixed300", "equal255", "equal256", "equal257", "equal4097", "blocks4097")


def _tie_randv(rng, Z, Dp):
    """Integer rows, every second one a copy of the row before it: every user ties between those two slots."""
    rv = rng.integers(-3, 4, size=(Z, Dp)).astype(np.float64)
    rv[1::2] = rv[0::2][:Z // 2]
    return rv[None]


def tie_cases(name):
    """Integer gX (D' = 3) on an Erdos-Renyi contention state in which the order decides the outcome, Z = 6, randv with
    duplicated rows.
      mixed300: duplicated rows, all-zero rows, rows equal in norm but not in direction, among rows of other norms;
      equalK: every row has norm 3 -- the visiting order must be 0, 1, 2, ... across every tile (256 keys) and, at K = 4097
        (17 tiles, two per group, seven empty groups), every group seam of k_rank_count;
      blocks4097: runs of 256 equal norms that start at k = 128 mod 256, so every run straddles a tile seam and every other one a
        group seam; the runs' levels are shuffled."""
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    K = {"mixed300": 300, "equal255": 255, "equal256": 256, "equal257": 257, "equal4097": 4097, "blocks4097": 4097}[name]
    seed = TIE_CASES.index(name) + 11
    rng = np.random.default_rng(seed)
    state = er_contention_graph(K, 0.05 if K <= 300 else 0.004, seed, hi=1.2)
    Z, Dp = 6, 3
    if name == "mixed300":
        gX = rng.integers(-3, 4, size=(K, Dp)).astype(np.float64)
        gX[rng.choice(K, 20, replace=False)] = 0.0
        src = rng.choice(K, 40, replace=False)
        gX[src[:20]] = gX[src[20:]]                        # duplicated rows
        gX[rng.choice(K, 60, replace=False)] = _NORM3[rng.integers(0, len(_NORM3), 60)]
    else:
        gX = _NORM3[rng.integers(0, len(_NORM3), K)].copy()
        if name == "blocks4097":
            run = (np.arange(K) + 128) // 256
            level = rng.permutation(int(run.max()) + 1) + 1.0
            gX *= level[run][:, None]
    return state, Z, gX, _tie_randv(rng, Z, Dp)


# --------------------------------------------------------------------------------------------
# projection edges
# --------------------------------------------------------------------------------------------
PROJECTION_CASES = ((1, 2, 17), (3, 15, 63), (4, 16, 64), (5, 17, 65), (63, 65, 130), (64, 2, 63), (65, 16, 17), (130, 17, 130),
                    (1, 65, 65), (64, 15, 64), (63, 17, 17))  # (D', Z, K)


def projection_edges(Dp, Z, K, nbatch=3):
    """Random normal gX on a small Erdos-Renyi state that holds one access point with Z users (min(Z, K) of them): the whole
    preference order of every user of that clique decides the output, not only its first entry.  The shapes sit at the zero
    padding of k_project_mfma: D' to 64, Z to 16, users to 64."""
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    seed = 1000 * Dp + 10 * Z + K
    rng = np.random.default_rng(seed)
    S, Q, h_max = er_contention_graph(K, 0.2, seed, hi=1.2)
    mem = np.sort(rng.choice(K, min(Z, K), replace=False))
    a, b = np.triu_indices(mem.size, 1)
    Q = ((Q + _sym01(K, mem[a], mem[b])) > 0).astype(np.float64).tocsr()
    Q.sort_indices()
    gX = rng.standard_normal((K, Dp)) * rng.uniform(0.2, 2.0, size=(K, 1))
    rv = normalise(rng.standard_normal((nbatch, Z, Dp)))
    return (S, Q, h_max), Z, gX, rv


# --------------------------------------------------------------------------------------------
# schedule
# --------------------------------------------------------------------------------------------
CHAIN_CASES = ("path", "lag32", "lag33", "common")
COMMON_PAIRS = {1: ((40, 41), (44, 45)), 8: ((50, 58), (52, 60)), 31: ((70, 101), (72, 103)), 32: ((110, 142), (112, 144))}


def order_chains(name, seed=0):
    """Z = D' = 3 and randv the identity, gX[k] = (K + 10 - k) x a permutation of (3, 2, 1): the visiting order is 0, 1, 2, ...
    and gX[k] spells out k's preference list.
      path:   Q links k and k + 1, K = 8192 + 40: the schedule has to take one user per step, K steps -- the most its buffers are
              sized for -- and crosses GS_CHUNK;
      lag32 / lag33: Q links k and k + 32 (the last position the interaction masks cover) / k + 33 (the first one they do not);
      common: Q links nothing that competes; the pairs of COMMON_PAIRS (lags 1, 8, 31, 32) emit 1/2 to one earlier user each, whose
              h_max = 3/4 admits one of them in its slot, and both want that slot.
    Except in `common`, user k also emits 1/4 to user k + 100 (the state needs a gain edge; 1/4 never exceeds h_max = 1)."""
    rng = np.random.default_rng(seed + CHAIN_CASES.index(name))
    Z = 3
    K = {"path": 8192 + 40, "lag32": 200, "lag33": 200, "common": 160}[name]
    h_max = np.ones(K)
    prefs = _perms(rng, K, Z)
    if name == "common":
        a = np.arange(0, 16, 2)
        Q = _sym01(K, a, a + 1)          # among the earlier users only
        rows, cols = [], []
        for n, (x, y) in enumerate(p for lag in sorted(COMMON_PAIRS) for p in COMMON_PAIRS[lag]):
            n = 2 * n                    # one earlier user per pair, no two of them on one access point
            rows += [x, y]
            cols += [n, n]
            h_max[n] = 0.75
            prefs[[x, y]] = _perms(rng, 2, Z, first=prefs[n, 0])
        S = _with_diag(K, np.array(rows), np.array(cols), np.full(len(rows), 0.5))
    else:
        lag = {"path": 1, "lag32": 32, "lag33": 33}[name]
        k = np.arange(K - lag)
        Q = _sym01(K, k, k + lag)
        k = np.arange(K - 100)
        S = _with_diag(K, k, k + 100, np.full(k.size, 0.25))
    gX = _ranked(prefs, Z) * (K + 10.0 - np.arange(K))[:, None]
    return (S, Q, h_max), Z, gX, np.eye(Z)[None]


# --------------------------------------------------------------------------------------------
# slots in global memory
# --------------------------------------------------------------------------------------------
def global_slots(nbatch=1):
    """Z = 4600 on an Erdos-Renyi state of K = 1700: 32 Z + 4 K bytes exceed the 150 KiB of LDS the greedy kernel may take, so its
    slot table stays in global memory (k_greedy_b<false, true>), and every row is longer than the preference window."""
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    K, Z, Dp = 1700, 4600, 5
    assert 32 * Z + 4 * K > 150 * 1024 >= 32 * Z
    rng = np.random.default_rng(5)
    state = er_contention_graph(K, 0.02, 5, hi=1.2)
    gX = rng.standard_normal((K, Dp)) * rng.uniform(0.2, 2.0, size=(K, 1))
    rv = normalise(rng.standard_normal((nbatch, Z, Dp)))
    return state, Z, gX, rv


def check_state(state):
    """The rules build_pattern (csrc/pattern.h) sets for a state, restated: canonical CSR, an empty Q diagonal, norm_H > 0 (at the
    handle's Z = 2).  Raises AssertionError."""
    from oracle import mmw_oracle as orc
    S, Q, h = state
    K = S.shape[0]
    assert S.shape == (K, K) and Q.shape == (K, K) and len(h) == K
    for m in (S, Q):
        assert m.has_canonical_format and m.indices.dtype.kind == "i"
        m2 = m.copy()
        m2.sort_indices()
        assert np.array_equal(m2.indices, m.indices)
    assert Q.diagonal().sum() == 0 and (Q != Q.T).nnz == 0 and np.all(Q.data == 1.0)
    _, _, norm_H = orc.process_state(2, S, Q, np.asarray(h, dtype=np.float64))
    assert np.all(norm_H > 0)
