"""Dense restatement of spectral_sdp_solver.run_with_state (sim_src/alg/sdp_solver.py:165-185) and the measures its tests compare by.

The reference takes `eigsh(k=Z, which='LM', tol=1e-5)` of the Laplacian of S_gain + S_gain^T (diagonal zeroed) and normalises the rows
of the K x Z block.  Here the eigenvectors come from `numpy.linalg.eigh` of the dense Laplacian.  Eigenvectors are defined up to
sign (and up to a rotation inside a degenerate eigenspace), and the row normalisation amplifies noise on users whose row of
V[:, top Z] is tiny, so nothing is compared entry by entry:

  projector(V)          P = V V^T of the un-normalised block: invariant to signs and to rotations inside the kept space
  gram_distance(N, M)   max |N N^T - M M^T| over the users whose un-normalised row has norm >= TAU: invariant the same way
  relgap                (lambda_Z - lambda_{Z+1}) / lambda_1, what the kept space's conditioning hangs on (Davis-Kahan)
"""
import numpy as np

TAU = 1e-3
EPS = 2.0 ** -52


def laplacian(S_gain):
    """L = D - W, W = S + S^T with the diagonal zeroed, D = diag(W 1): dense float64."""
    S = np.asarray(S_gain.toarray() if hasattr(S_gain, "toarray") else S_gain, dtype=np.float64)
    W = S + S.T
    np.fill_diagonal(W, 0.0)
    return np.diag(W.sum(axis=1)) - W


class Dense:
    """eigh of the state's Laplacian, once; `top(Z)` cuts it."""

    def __init__(self, S_gain):
        self.L = laplacian(S_gain)
        self.K = self.L.shape[0]
        self.lam, self.vec = np.linalg.eigh(self.L)  # ascending

    def top(self, Z):
        """(eigenvalues [Z] ascending, V [K, Z] in that order): eigsh's layout."""
        return self.lam[self.K - Z:], self.vec[:, self.K - Z:]

    def relgap(self, Z):
        """(lambda_Z - lambda_{Z+1}) / lambda_1 in descending numbering; lambda_{K+1} is taken as 0 at Z = K."""
        d = self.lam[::-1]
        if d[0] <= 0.0:
            return 0.0
        return float((d[Z - 1] - (d[Z] if Z < self.K else 0.0)) / d[0])

    def lam_max(self):
        return float(self.lam[-1])


def normalise_rows(V):
    """sdp_solver.py:182, with the batch's stated deviation: an exactly zero row stays zero."""
    n = np.linalg.norm(V, axis=1, keepdims=True)
    return np.divide(V, n, out=np.zeros_like(V), where=n > 0.0)


def block(S_gain, Z):
    """The restatement's answer: the row-normalised top-Z block."""
    return normalise_rows(Dense(S_gain).top(Z)[1])


def projector(V):
    return V @ V.T


def big_rows(V, tau=TAU):
    """Users whose row of the un-normalised block has norm >= tau."""
    return np.linalg.norm(V, axis=1) >= tau


def gram_distance(N, M, rows):
    """max |N N^T - M M^T| over the users `rows` (a boolean mask) of two row-normalised blocks."""
    if not np.any(rows):
        return 0.0
    a, b = N[rows], M[rows]
    return float(np.max(np.abs(a @ a.T - b @ b.T)))


def unnormalised_from(N, row_norms):
    """A block's rows scaled back by the given row norms (the device hands out the normalised block only)."""
    return N * np.asarray(row_norms)[:, None]
