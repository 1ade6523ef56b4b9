"""NumPy restatement of the handle's Laplacian on the L pattern (csrc/kernels_spectral.h, MMW_F_LAPLACIAN).

Per pattern entry (r, c), c != r: -(S[r, c] + S[c, r]) with S = S_gain; on the diagonal the degree, the sum of S[r, c] + S[c, r] over
the row's off-diagonal pattern entries in ascending column order, accumulated one by one in Python's float (IEEE double, the order
the device states).  Stored zeros of S and its diagonal play no part, like in the handle's own copy of S_gain.
"""
import numpy as np
import scipy.sparse


def laplacian_on_pattern(S_gain, l_indptr, l_indices):
    """float64 [nnzL] in the pattern's order."""
    S = scipy.sparse.csr_matrix(S_gain, dtype=np.float64)
    val = {}
    coo = S.tocoo()
    for r, c, v in zip(coo.row.tolist(), coo.col.tolist(), coo.data.tolist()):
        if r != c and v != 0.0:
            val[(r, c)] = val.get((r, c), 0.0) + v
    out = np.empty(len(l_indices), dtype=np.float64)
    K = len(l_indptr) - 1
    for r in range(K):
        deg = 0.0
        dpos = -1
        for e in range(int(l_indptr[r]), int(l_indptr[r + 1])):
            c = int(l_indices[e])
            if c == r:
                dpos = e
                continue
            w = val.get((r, c), 0.0) + val.get((c, r), 0.0)
            out[e] = -w
            deg += w
        assert dpos >= 0, "the pattern holds every diagonal entry"
        out[dpos] = deg
    return out


def scatter(K, l_indptr, l_indices, values):
    """The K x K dense matrix of values on the pattern."""
    return scipy.sparse.csr_matrix((np.asarray(values, dtype=np.float64), l_indices, l_indptr), shape=(K, K)).toarray()


def pure_q_entries(state, l_indptr, l_indices):
    """Boolean mask [nnzL]: off-diagonal pattern entries (r, c) with neither S[r, c] nor S[c, r] stored non-zero (there through Q alone)."""
    S = scipy.sparse.csr_matrix(state[0], dtype=np.float64).tolil(copy=True)
    S.setdiag(0.0)
    W = scipy.sparse.csr_matrix(S)
    W.eliminate_zeros()
    W = ((W != 0) + (W.T != 0)).tocsr()
    K = len(l_indptr) - 1
    rows = np.repeat(np.arange(K), np.diff(l_indptr))
    cols = np.asarray(l_indices)
    hit = np.asarray(W[rows, cols]).ravel().astype(bool)
    return (rows != cols) & ~hit
