"""CPU restatements of the reference's greedy baselines (sim_src/alg/gm.py) for the tests.

`slot_major` / `max_rand` work on the nonzeros, O(deg) per probe, in the style of oracle.rounding_one_attempt.  Why that equals the
reference's dense K-vectors (gm.py:36-50):
  * the interference check (:36-39) compares gain_sum[j] + S[k, j] with h_max[j] for k and every member j of the list.  For k the
    zeroed diagonal adds 0.  A member j that k does not reach sees gain_sum[j] + 0, and gain_sum[j] <= h_max[j] has held for every
    member since it was accepted (each later acceptance checked it), so only k's out-neighbours among the members can fail;
  * the association check (:42-45) reduces the same way to k itself and k's Q-neighbours among the members;
  * the dense adds (:49-50) add 0.0 everywhere else, which changes no fp64 sum: adding the nonzeros in acceptance order gives
    the same bits.
The association check is kept as sums of Q rows (no clique shortcut), so it also checks the device's clique path.

`dense_slot_major` is a plain dense transcription of the procedure (K-vectors per slot, every member checked), small K only.
"""
import numpy as np
import scipy.sparse


def out_rows(state):
    """S_gain rows with the diagonal zeroed and explicit zeros dropped (gm.py:15), Q rows without zeros; CSR."""
    S = scipy.sparse.csr_matrix(state[0]).tolil()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    Q = scipy.sparse.csr_matrix(state[1]).copy()
    Q.eliminate_zeros()
    Q.sort_indices()
    return S, Q, np.asarray(state[2], dtype=np.float64)


def gain_key(state):
    S = scipy.sparse.csr_matrix(state[0]).tolil()
    S.setdiag(0)
    return np.asarray(S.tocsr().transpose().sum(axis=1)).ravel()


def asso_key(state):
    return np.asarray(state[1].sum(axis=1)).ravel()


def slot_pass(rows, order, nattempt):
    """One slot: `nattempt` attempts over `order` on sums carried between attempts; the first longest list."""
    S, Q, h = rows
    K = h.size
    gs = np.zeros(K)
    asum = np.zeros(K)
    best = []
    for _ in range(nattempt):
        member = np.zeros(K, dtype=bool)
        cur = []
        for k in order:
            if gs[k] > h[k] or asum[k] >= 1.0:
                continue
            nb = S.indices[S.indptr[k]:S.indptr[k + 1]]
            gv = S.data[S.indptr[k]:S.indptr[k + 1]]
            qn = Q.indices[Q.indptr[k]:Q.indptr[k + 1]]
            qv = Q.data[Q.indptr[k]:Q.indptr[k + 1]]
            m = member[nb]
            if np.any(gs[nb[m]] + gv[m] > h[nb[m]]):
                continue
            mq = member[qn]
            if np.any(asum[qn[mq]] + qv[mq] >= 1.0):
                continue
            for j, v in zip(nb, gv):  # one add per address, in acceptance order
                gs[j] += v
            for j, v in zip(qn, qv):
                asum[j] += v
            member[k] = True
            cur.append(int(k))
        if len(cur) > len(best):
            best = cur
    return best


def slot_major(key, Z, state, nattempt=1, not_Z_bound=False, orders=None, stable=False, randint=None):
    """MAX_GAIN / MAX_ASSO.  orders: the recorded per-slot-and-attempt argsort outputs (positions among the unassigned users), used
    in place of a live argsort; stable: argsort(kind="stable").  Returns (z_vec, ZZ, rem, passes run)."""
    rows = out_rows(state)
    K = rows[2].size
    if not_Z_bound:
        Z = K
    not_assigned = np.ones(K, dtype=bool)
    z_vec = np.zeros(K)
    ZZ = 0
    it = iter(orders) if orders is not None else None
    passes = 0
    for z in range(Z):
        ZZ += 1
        kindx = np.arange(K)[not_assigned]
        if it is not None:
            ords = [kindx[next(it)] for _ in range(nattempt)]
            if any(not np.array_equal(o, ords[0]) for o in ords):  # (the attempts of a slot see the same unassigned users)
                raise AssertionError("recorded orders differ between attempts of one slot")
            order = ords[0]
        else:
            order = kindx[np.argsort(-key[not_assigned], kind="stable" if stable else None)]
        lst = slot_pass(rows, order, nattempt)
        passes += 1
        z_vec[lst] = z
        not_assigned[lst] = False
        if not not_assigned.any():
            break
        if not lst and it is None:  # every later slot accepts nobody either
            ZZ = Z
            break
    if not_assigned.any():
        fn = np.random.randint if randint is None else randint
        z_vec[not_assigned] = fn(ZZ if not_Z_bound else Z, size=int(not_assigned.sum()))
    return z_vec, ZZ, int(not_assigned.sum()), passes


def max_rand(Z, state, rank, pref, randint=None):
    """MAX_RAND's user-major greedy for the user order `rank` and per-user slot preference pref[k] (gm.py:152-199)."""
    S, Q, h = out_rows(state)
    K = h.size
    slot = np.full(K, -1)
    gs = np.zeros((Z, K))
    for k in rank:
        nb = S.indices[S.indptr[k]:S.indptr[k + 1]]
        gv = S.data[S.indptr[k]:S.indptr[k + 1]]
        qn = Q.indices[Q.indptr[k]:Q.indptr[k + 1]]
        for z in pref[k]:
            m = slot[nb] == z
            if gs[z, k] > h[k] or np.any(gs[z, nb[m]] + gv[m] > h[nb[m]]) or np.any(slot[qn] == z):
                continue
            gs[z, nb] += gv
            slot[k] = z
            break
    un = slot < 0
    z_vec = np.where(un, 0, slot).astype(np.float64)
    if un.any():
        fn = np.random.randint if randint is None else randint
        z_vec[un] = fn(Z, size=int(un.sum()))
    return z_vec, Z, int(un.sum())


def dense_slot_major(key, Z, state, nattempt=1, not_Z_bound=False):
    """The procedure on dense K-vectors with every member checked (stable ties); small K."""
    Sd = np.asarray(scipy.sparse.csr_matrix(state[0]).todense(), dtype=np.float64)
    np.fill_diagonal(Sd, 0.0)
    Qd = np.asarray(scipy.sparse.csr_matrix(state[1]).todense(), dtype=np.float64)
    h = np.asarray(state[2], dtype=np.float64)
    K = h.size
    if not_Z_bound:
        Z = K
    free = np.ones(K, dtype=bool)
    z_vec = np.zeros(K)
    ZZ = 0
    for z in range(Z):
        ZZ += 1
        g_acc = np.zeros(K)
        a_acc = np.zeros(K)
        kept = []
        for _ in range(nattempt):
            idx = np.flatnonzero(free)
            visit = idx[np.argsort(-key[free], kind="stable")]
            lst = []
            for k in visit:
                chk = np.array(lst + [k], dtype=np.int64)
                if np.any(g_acc[chk] + Sd[k, chk] > h[chk]):
                    continue
                if np.any(a_acc[chk] + Qd[k, chk] >= 1):
                    continue
                g_acc = g_acc + Sd[k]
                a_acc = a_acc + Qd[k]
                lst.append(int(k))
            if len(lst) > len(kept):
                kept = lst
        z_vec[kept] = z
        free[kept] = False
        if not free.any():
            break
    return z_vec, ZZ, int(free.sum())


def drive_abi(h, key, Z, natt, nzb, orders=None, stable=False):
    """MAX_GAIN / MAX_ASSO through a `_lib.GreedyHandle` the way sig_sdp_mmw_amd.gm drives it, optionally on recorded orders;
    returns (slot with -1 = unassigned, ZZ, rem) before the random fill."""
    K = h.K
    if nzb:
        Z = K
    if stable:
        return h.run(key, Z, natt)
    slot = np.full(K, -1)
    it = iter(orders) if orders is not None else None
    ZZ = 0
    for z in range(Z):
        ZZ += 1
        kindx = np.flatnonzero(slot < 0)
        if it is not None:
            order = kindx[[next(it) for _ in range(natt)][0]]
        else:
            order = kindx[np.argsort(-key[kindx])]
        lst = h.pass_(order, natt)
        slot[lst] = z
        if (slot >= 0).all():
            break
        if lst.size == 0 and it is None:
            ZZ = Z
            break
    return slot, ZZ, int((slot < 0).sum())


def check_slots(state, z_vec, assigned):
    """Every slot on its own: the members' received gains (column sums of S without diagonal) within h_max, no two members on one
    access point (Q)."""
    S, Q, h = out_rows(state)
    z = np.asarray(z_vec).astype(np.int64)
    for s in np.unique(z[assigned]):
        mem = np.flatnonzero(assigned & (z == s))
        recv = np.asarray(S[mem][:, mem].sum(axis=0)).ravel()
        assert np.all(recv <= h[mem]), s
        assert Q[mem][:, mem].nnz == 0, s
