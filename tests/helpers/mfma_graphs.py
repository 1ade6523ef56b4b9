"""Graphs designed for the shape limits of the matrix-core SpMM / SDDMM (csrc/kernels_mfma.h), shared by test_mfma_shapes_host.py
(which pins the blocks each one gives, on a host-only handle) and test_hip_mfma_shapes.py (which runs them on the device).

A case is (state, switches): the switches are the MMW_* variables a handle must be created under for the blocks the table names.
`SHAPES` holds, per case, what build_mfma_blocking makes of it: (blocks, row tiles, k-steps in all, smallest and largest k-steps of
a block).  A block is written rows:k-steps; a k-step is 16 union columns and a block's k-steps are padded to a multiple of 4.

  j5       journal_graph(5, 75e-4, 0), K 75             64:8 11:4
  j9       journal_graph(9, 75e-4, 0), K 243            64:8 64:8 64:8 51:12
  j9r20    the same, MMW_MF_ROWS=20                     twelve blocks of 20 rows with 4 or 8 k-steps, then 3:4; one row tile
  j9cap48  the same, MMW_MF_UNION_CAP=48                47 blocks of 1 to 30 rows, every one exactly 4 k-steps; one row tile
  b97r33   band_state(97, 20), MMW_MF_ROWS=33           33:4 33:8 31:4: the second row tile of a block holds one row
  one64    band_state(64, 31)                           64:4: the whole matrix is one block
  hub      band_state(400, 6, hub of 330, 3 isolated)   64:8 x5, 64:24, 11:4, 2:4, 1:4 x3: a 340-entry row, rows that hold only their diagonal
  hubr32   the same, MMW_MF_ROWS=32                     18 blocks, one row tile, 32:24 beside 1:4
  cap      journal_graph(8, 0.05, seed=2), K 1280       21 blocks of 16 to 40 k-steps, two of them cut by the 640-column cap (40 k-steps)
  dense    er_contention_graph(640, 0.35, 1)            the LDS-staged blocking is not usable: the verifier's regression case only
"""
import functools

import numpy as np
import scipy.sparse as sp

from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph


def band_state(K, w, clique=3, hub=None, isolated=(), seed=0):
    """A band of half-width w (the interference matrix S, log-uniform gains, diagonal 3.7), optionally a hub row linked to n rows
    outside its band and rows left with their diagonal only; associations Q in cliques of `clique` consecutive rows."""
    rng = np.random.default_rng(seed); rows, cols = [], []
    for d in range(1, w + 1):
        i = np.arange(K - d); rows += [i, i + d]; cols += [i + d, i]
    if hub is not None:
        h, n = hub
        c = rng.choice(np.setdiff1d(np.arange(K), np.arange(max(0, h - w), min(K, h + w + 1))), size=n, replace=False)
        rows += [np.full(n, h), c]; cols += [c, np.full(n, h)]
    rows = np.concatenate(rows); cols = np.concatenate(cols)
    keep = ~np.isin(rows, isolated) & ~np.isin(cols, isolated)
    rows, cols = rows[keep], cols[keep]
    vals = np.exp(rng.uniform(np.log(0.1), np.log(3.7), rows.size))
    S = (sp.csr_matrix((vals, (rows, cols)), shape=(K, K)) + sp.diags(np.full(K, 3.7))).tocsr()
    qr, qc = [], []
    for a in range(0, K - clique + 1, clique):
        for i in range(clique):
            for j in range(clique):
                if i != j and a + i not in isolated and a + j not in isolated: qr.append(a + i); qc.append(a + j)
    return S, sp.csr_matrix((np.ones(len(qr)), (qr, qc)), shape=(K, K)), np.ones(K)


@functools.lru_cache(maxsize=None)
def _state(key):
    return {
        "j5": lambda: journal_graph(5, 75e-4, 0),
        "j9": lambda: journal_graph(9, 75e-4, 0),
        "b97": lambda: band_state(97, 20),
        "one64": lambda: band_state(64, 31),
        "hub": lambda: band_state(400, 6, hub=(133, 330), isolated=(0, 57, 399)),
        "cap": lambda: journal_graph(8, 0.05, seed=2),
        "k2048": lambda: journal_graph(16, 0.02, seed=4),
        "dense": lambda: er_contention_graph(640, 0.35, 1),
    }[key]()


# name: (state key, switches)
CASES = {
    "j5": ("j5", {}),
    "j9": ("j9", {}),
    "j9r20": ("j9", {"MMW_MF_ROWS": "20"}),
    "j9cap48": ("j9", {"MMW_MF_UNION_CAP": "48"}),
    "b97r33": ("b97", {"MMW_MF_ROWS": "33"}),
    "one64": ("one64", {}),
    "hub": ("hub", {}),
    "hubr32": ("hub", {"MMW_MF_ROWS": "32"}),
    "cap": ("cap", {}),
    "k2048r64": ("k2048", {"MMW_MF_ROWS": "64"}),
    "dense": ("dense", {}),
}

# name: (blocks, row tiles, k-steps in all, smallest, largest k-steps of a block) -- test_mfma_shapes_host.py holds the builder to it
SHAPES = {
    "j5": (2, 2, 12, 4, 8),
    "j9": (4, 2, 36, 8, 12),
    "j9r20": (13, 1, 84, 4, 8),
    "j9cap48": (47, 1, 188, 4, 4),
    "b97r33": (3, 2, 16, 4, 8),
    "one64": (1, 2, 4, 4, 4),
    "hub": (11, 2, 84, 4, 24),
    "hubr32": (18, 1, 92, 4, 24),
    "cap": (21, 2, 588, 16, 40),
}


def state_key(name):
    return CASES[name][0]


def state(name):
    """(S_gain, Q_asso, h_max) of a case; cases on the same graph share one object."""
    return _state(CASES[name][0])


def switches(name):
    return dict(CASES[name][1])


def apply_switches(monkeypatch, name, extra=None):
    """Sets the case's MMW_* variables (and `extra`) for the handles created after it; a handle reads them once, at creation."""
    for k, v in {**CASES[name][1], **(extra or {})}.items():
        monkeypatch.setenv(k, v)
