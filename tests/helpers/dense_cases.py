"""Inputs, NumPy restatements and bounds for the factor's dense building blocks (mmw_dense_gram / _gemm / _chol / _orth).

test_dense_cases_host.py shows on the CPU that every case has the property it is named for and that the restatements stay inside
the bounds; test_hip_dense_blocks.py holds the device to the same bounds on the same inputs.  Nothing here touches the library.
Every block is K x ld with the sentinel 7.0 in the padding columns [b, ld): a kernel that reads one of them shows it in a result.
"""
import functools

import numpy as np

SENTINEL = 7.0
U64 = 2.0 ** -53  # unit roundoff of float64
U32 = 2.0 ** -24
NS_MAX = {np.float32: 1.6e-3, np.float64: 5e-7}  # Factorizer::orthonormalise, ns_max
FLOOR_EPS = 1e-14  # the eigen fallback's relative floor as the factor calls it

# ---- the cases of the issue -------------------------------------------------------------------------------------------------------
GRAM_K = [1, 15, 16, 17, 255, 256, 257, 1000]
GRAM_B = [1, 3, 4, 5, 63, 64, 65, 100, 129]
GEMM_K = [1, 63, 64, 65, 130]
GEMM_B = [1, 15, 16, 17, 33, 100]
GEMM_N = [1, 63, 64, 65]
CHOL_B = [1, 2, 31, 32, 33, 64, 65, 96, 100, 289, 321]
CHOL_COND = [1e1, 1e3]
ORTH_SHAPES = [(1, 1), (64, 32), (65, 33), (200, 40), (130, 97), (200, 130), (400, 321)]
ORTH_PAD = [0, 7]
KAPPA_NS = [1.0, 1e2, 1e4]          # paths [0, 1], with MMW_FACTOR_NO_NS=1 [0, 0]
KAPPA_FREE = [1e5, 1e8, 1e9]        # at a threshold (Newton-Schulz test / Cholesky breakdown): the path is free, the quality is not
KAPPA_CHOL2 = 1e7                   # [0, 0]
KAPPA_FALLBACK = 1e10               # first pass 2
KAPPA_BEYOND = [1e12, 1e14]         # fp64 only: finite, and no worse than 8 x the restatement


def gram_cases():
    """(K, b, ld, sym): every K with b in {5, 65}, every b with K in {17, 257}; each pair with two of the four (ld, sym) choices,
    alternating, so that both paddings and both values of sym meet every K and every b."""
    pairs = [(K, b) for K in GRAM_K for b in GRAM_B if b in (5, 65) or K in (17, 257)]
    out = []
    for i, (K, b) in enumerate(pairs):
        first = (0, 0) if i % 2 == 0 else (0, 1)
        second = (5, 1) if i % 2 == 0 else (5, 0)
        for pad, sym in (first, second):
            out.append((K, b, b + pad, sym))
    return out


def gemm_cases(b):
    """(K, n, ld, ldq) for one b: every K, n in GEMM_N and n = b, ldq in {n, n + 3}; ld = max(b, n), every other case 5 wider."""
    out = []
    i = 0
    for K in GEMM_K:
        for n in sorted(set(GEMM_N + [b])):
            for ldq in (n, n + 3):
                out.append((K, n, max(b, n) + (5 if i % 2 else 0), ldq))
                i += 1
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def round_to(A, T):
    return np.asarray(A, dtype=T).astype(np.float64)


def int_block(K, b, ld, seed, T=np.float64):
    """integers in [-8, 8] in the columns < b, the sentinel in the padding"""
    rng = np.random.default_rng(seed)
    V = np.full((K, ld), SENTINEL)
    V[:, :b] = rng.integers(-8, 9, size=(K, b))
    return round_to(V, T)


def normal_block(K, b, ld, seed, T=np.float64):
    rng = np.random.default_rng(seed)
    V = np.full((K, ld), SENTINEL)
    V[:, :b] = rng.standard_normal((K, b))
    return round_to(V, T)


def haar(n, m, rng):
    Q, R = np.linalg.qr(rng.standard_normal((n, m)))
    return Q * np.sign(np.diag(R))


def svd_block(K, b, ld, kappa, seed, T=np.float64):
    """U diag(logspace(0, -log10 kappa, b)) W^T with Haar U (K x b) and W (b x b): a conditioning no column scaling removes"""
    assert K >= b
    rng = np.random.default_rng(seed)
    s = np.logspace(0.0, -np.log10(kappa), b)
    V = np.full((K, ld), SENTINEL)
    V[:, :b] = (haar(K, b, rng) * s) @ haar(b, b, rng).T
    return round_to(V, T)


def zero_column_block(K, b, ld, seed, T=np.float64):
    """a well-conditioned block with its middle column exactly zero"""
    V = svd_block(K, b, ld, 1e2, seed, T)
    V[:, b // 2] = 0.0
    return V


@functools.lru_cache(maxsize=None)
def spd(b, cond, seed):
    """the unit-diagonal-scaled Gram matrix of an svd_block with kappa = sqrt(cond)"""
    V = svd_block(2 * b + 3, b, b, np.sqrt(cond), seed)
    G = V.T @ V
    G = 0.5 * (G + G.T)
    d = 1.0 / np.sqrt(np.diag(G))
    G = G * (d[:, None] * d[None, :])
    G.setflags(write=False)
    return G


def indefinite(b, k, seed):
    """symmetric with a positive diagonal, positive leading minors up to index k - 1 and a negative pivot at index k:
    L0 diag(1, ..., 1, -0.01 at k, 1, ...) L0^T with a unit lower-triangular L0"""
    assert 1 <= k < b
    rng = np.random.default_rng(seed)
    L0 = np.eye(b) + np.tril(rng.uniform(-1.0, 1.0, (b, b)), -1) / np.sqrt(b)
    L0[k, :k] = np.where(L0[k, :k] < 0, -0.5, 0.5) / np.sqrt(k)  # G_kk = 0.25 - 0.01: the diagonal stays positive
    D = np.ones(b)
    D[k] = -0.01
    G = (L0 * D) @ L0.T
    return 0.5 * (G + G.T)


BREAKDOWN = {"panel0": (64, 10), "later_full_panel": (100, 40), "partial_last_panel": (70, 68), "zero_diagonal": (50, 20)}


def breakdown_case(name):
    """(G, index of the first pivot that is not positive)"""
    b, k = BREAKDOWN[name]
    if name == "zero_diagonal":
        G = np.array(spd(b, 1e1, 5))
        G[k, :] = 0.0
        G[:, k] = 0.0
        return G, k
    return indefinite(b, k, 11 * b + k), k


# ---- restatements -----------------------------------------------------------------------------------------------------------------
def scale_unit_diagonal(G):
    """k_scale_sym + k_apply_scale_sym: d = 1 / sqrt(diag G), 0 where the diagonal is not positive; G' = G * (d_i d_j)"""
    dg = np.diag(G)
    d = np.zeros_like(dg)
    pos = dg > 0.0
    d[pos] = 1.0 / np.sqrt(dg[pos])
    return G * (d[:, None] * d[None, :]), d


def chol_restatement(G):
    """Right-looking Cholesky in panels of 32, the rows below a panel multiplied by the explicit inverse of the 32 x 32 factor (what
    k_chol_panel does).  Returns (L, [inverse of each diagonal block], ok, index of the first pivot that is not positive or -1)."""
    A = np.array(G, dtype=np.float64)
    b = A.shape[0]
    dinv = []
    for j0 in range(0, b, 32):
        nb = min(32, b - j0)
        D = A[j0:j0 + nb, j0:j0 + nb].copy()
        for j in range(nb):
            g = D[j, j]
            if not g > 0.0:
                return None, dinv, False, j0 + j
            dj = np.sqrt(g)
            D[j, j] = dj
            D[j + 1:, j] *= 1.0 / dj
            D[j + 1:, j + 1:] -= np.outer(D[j + 1:, j], D[j + 1:, j])
        D = np.tril(D)
        Di = np.zeros((nb, nb))
        for c in range(nb):
            Di[c, c] = 1.0 / D[c, c]
            for k in range(c + 1, nb):
                Di[k, c] = -(D[k, c:k] @ Di[c:k, c]) * (1.0 / D[k, k])
        dinv.append(Di)
        A[j0:j0 + nb, j0:j0 + nb] = D
        if j0 + nb < b:
            X = A[j0 + nb:, j0:j0 + nb] @ Di.T
            A[j0 + nb:, j0:j0 + nb] = X
            A[j0 + nb:, j0 + nb:] -= X @ X.T
    return np.tril(A), dinv, True, -1


def trsm_restatement(V, d, L, dinv):
    """k_trsm_blocked: X_J = (V_J D_J - X_<J L[J, <J]^T) Linv_JJ^T in column blocks of 32"""
    b = L.shape[0]
    X = np.zeros_like(V)
    for p, j0 in enumerate(range(0, b, 32)):
        j1 = min(b, j0 + 32)
        T = V[:, j0:j1] * d[j0:j1] - X[:, :j0] @ L[j0:j1, :j0].T
        X[:, j0:j1] = T @ dinv[p].T
    return X


def orth_restatement(V, T, no_ns=False, eps=FLOOR_EPS):
    """Factorizer::orthonormalise on the columns of V (K x b, already rounded to T) in plain NumPy: float64 Gram, storage rounded to T
    after each pass.  Returns (Q, [path of pass 1, path of pass 2], ||G - I||_F seen by pass 2)."""
    A = np.array(V, dtype=np.float64)
    b = A.shape[1]
    path = []
    dev = None
    for p in range(2):
        G = A.T @ A
        G = 0.5 * (G + G.T)
        if p == 1:
            dev = float(np.linalg.norm(G - np.eye(b)))
            if not no_ns and dev <= NS_MAX[T]:
                A = round_to(A @ (1.5 * np.eye(b) - 0.5 * G), T)
                path.append(1)
                continue
        Gs, d = scale_unit_diagonal(G)
        L, dinv, ok, _ = chol_restatement(Gs)
        if ok:
            A = round_to(trsm_restatement(A, d, L, dinv), T)
            path.append(0)
        else:
            # A row and column of zeros (d = 0) is decoupled: a Jacobi method never rotates it, its eigenvector is the unit vector and its
            # eigenvalue 0 exactly.  LAPACK leaves rounding noise there, which the floor's 1 / sqrt(1e-14 b) would amplify into a column.
            live = np.flatnonzero(d > 0.0)
            lam, Q = np.zeros(b), np.eye(b)
            if live.size:
                lam[live], Q[np.ix_(live, live)] = np.linalg.eigh(Gs[np.ix_(live, live)])
            A = round_to(A @ (d[:, None] * Q / np.sqrt(np.maximum(lam, eps * b))), T)
            path.append(2)
    return A, path, dev


# ---- measures and bounds ----------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U64 / (1.0 - n * U64)


def chol_residual_share(L, G):
    """max over the entries of |L L^T - G| / (gamma_{b+1} |L||L^T|), the product formed in extended precision"""
    b = L.shape[0]
    Lx = np.asarray(L, dtype=np.longdouble)
    R = np.abs(Lx @ Lx.T - np.asarray(G, dtype=np.longdouble))
    B = gamma(b + 1) * (np.abs(Lx) @ np.abs(Lx).T)
    return float(np.max(R / B))


def dinv_share(Di, L, p):
    """max |Dinv_p L_pp - I| over the block's nb rows and columns, as a share of 32 * 2^-53 * cond(L_pp)"""
    b = L.shape[0]
    nb = min(32, b - 32 * p)
    blk = L[32 * p:32 * p + nb, 32 * p:32 * p + nb]
    return float(np.max(np.abs(Di[:nb, :nb] @ blk - np.eye(nb))) / (32 * U64 * np.linalg.cond(blk)))


def err_o(Q):
    return float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))))


def err_s(V, Q):
    nv = np.linalg.norm(V)
    return float(np.linalg.norm(V - Q @ (Q.T @ V)) / nv) if nv > 0 else 0.0


def ns_term(T):
    return 0.375 * NS_MAX[T] ** 2


def orth_bounds(T, b, r, last_pass):
    """(bound on err_o, bound on err_s) for kappa <= 1e10; r = the restatement's err_o on the same input"""
    extra = ns_term(T) if last_pass == 1 else 0.0
    if T == np.float64:
        return 8.0 * max(r, b * U64) + extra, 8.0 * b * U64
    return 2.0 ** -22 + 8.0 * b * U64 + extra, np.sqrt(b) * 2.0 ** -23


def qr_bound(T, b, kappa):
    return 8.0 * kappa ** 2 * b * U64 + (2.0 ** -23 if T == np.float32 else 0.0)


def orth_list(Tname):
    """(kind, kappa, no_ns) of every orthonormalisation case of one dtype"""
    out = [("svd", k, no_ns) for k in KAPPA_NS for no_ns in (False, True)]
    out += [("svd", k, False) for k in sorted(KAPPA_FREE + [KAPPA_CHOL2, KAPPA_FALLBACK])]
    out.append(("zero", 0.0, False))
    if Tname == "f64":
        out += [("svd", k, False) for k in KAPPA_BEYOND]
    return out


def expected_path(b, kind, kappa, Tname, no_ns):
    """the passes a case was built for (a prefix of the path), or None where the path is free"""
    if kind == "zero":
        return [2, 2]
    if b == 1 or kappa in KAPPA_NS:  # (one column has no conditioning)
        return [0, 0] if no_ns else [0, 1]
    if kappa == KAPPA_CHOL2:
        return [0, 0] if Tname == "f64" else None  # fp32: at the Newton-Schulz threshold (test_dense_cases_host.py)
    if kappa == KAPPA_FALLBACK:
        # fp32: rounding the block to fp32 leaves it a condition number of 4e8 ... 1e9 whatever kappa is, inside the band 1e8 ... 1e9
        # where the Cholesky factorisation breaks down or not by the rounding noise of the Gram matrix (test_dense_cases_host.py)
        return [2] if Tname == "f64" else None
    return None


def zero_case_spectrum(Q, T):
    """(eigenvalues of Q^T Q ascending, how far they may lie from {0, 1})"""
    b = Q.shape[1]
    return np.linalg.eigvalsh(Q.T @ Q), b * orth_bounds(T, b, 0.0, 2)[0]


def qr_positive(V):
    """the QR factor of V with a positive diagonal of R"""
    Q, R = np.linalg.qr(V)
    return Q * np.sign(np.diag(R))


@functools.lru_cache(maxsize=None)
def orth_case(K, b, pad, kind, kappa, Tname, no_ns):
    """One orthonormalisation case, its restatement and the restatement's figures, computed once for both test modules.
    kind: "svd" (kappa as given) or "zero" (one zero column).  Returns a dict; the arrays are read-only."""
    T = np.float32 if Tname == "f32" else np.float64
    seed = 1000 * K + b
    V = svd_block(K, b, b + pad, kappa, seed, T) if kind == "svd" else zero_column_block(K, b, b + pad, seed, T)
    Q, path, dev = orth_restatement(V[:, :b], T, no_ns)
    V.setflags(write=False)
    Q.setflags(write=False)
    return {"V": V, "T": T, "Q": Q, "path": path, "dev2": dev, "err_o": err_o(Q), "err_s": err_s(V[:, :b], Q)}
