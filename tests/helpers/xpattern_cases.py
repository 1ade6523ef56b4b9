"""Cases for the tests of X on the pattern (tests/test_hip_xpattern_shapes.py, tests/test_xpattern_cases_host.py): the row layouts of the
dense block restated, the float64 reference of the operation on the handle's own X_half, the widths that reach every layout, the
states, and the rounding bounds.

The operation: X[a,b] = <y_a, y_b> / tr on the fixed pattern, y the rows of X_half = exp(L/2)R, tr = sum_k ||y_k||^2 / K
(k_sddmm / k_sddmm_blk / k_sddmm_blk2 in csrc/kernels_loop.h; the norms and the trace slabs come from k_lz_combine in
csrc/kernels_expm.h on the Lanczos path and from k_rownorm2 on the Taylor path).
"""
import functools
import math

import numpy as np
import scipy.sparse

from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

F64, F32 = _lib.F64, _lib.F32
VEC = {F64: 2, F32: 4}                   # columns per 16-byte lane
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24}  # unit roundoff of the handle's type
NAME = {F64: "f64", F32: "f32"}
NPTYPE = {F64: np.float64, F32: np.float32}
NIT, ETA = 3, 0.05
TOL = {F64: 1e-13, F32: 1e-7}            # set_expm's tolerance
BAR = {F64: 1e-9, F32: 1e-4}             # the trajectory bars of the existing tests (continuity with the oracle)


# ---- make_layout (csrc/expm_engine.h) restated ---------------------------------------------------------------------------------
def layout(D, dtype):
    """(LPR, G, NCH, Dpad): a row is LPR lanes of 16 bytes; up to 32 lanes it is rounded up to a power of two and G = 64 / LPR rows share
    a wave; wider rows are rounded up to a multiple of 8 lanes and take NCH = ceil(LPR / 64) chunks of a wave (at most 4)."""
    vec = VEC[dtype]
    lpr = (D + vec - 1) // vec
    if lpr <= 32:
        p = 1
        while p < lpr:
            p <<= 1
        lpr, G, nch = p, 64 // p, 1
    else:
        lpr = (lpr + 7) // 8 * 8
        G, nch = 1, (lpr + 63) // 64
        if nch > 4:
            raise ValueError("D = %d is wider than the layout takes" % D)
    return lpr, G, nch, lpr * vec


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def x_from_half(indptr, indices, X_half):
    """X on the pattern (CSR order of indptr / indices) from X_half, all in float64: nrm = (Y*Y).sum(1), tr = nrm.sum() / K,
    entry (a, b) -> Y[a] . Y[b] / tr, the diagonal nrm / tr."""
    Y = np.asarray(X_half, dtype=np.float64)
    K = Y.shape[0]
    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(indices, dtype=np.int64)
    rows = np.repeat(np.arange(K, dtype=np.int64), np.diff(indptr))
    nrm = (Y * Y).sum(1)
    tr = nrm.sum() / K
    out = np.empty(cols.size, dtype=np.float64)
    for lo in range(0, cols.size, 4096):  # (in pieces: a dense state at the widest row is 16 900 x 1024)
        hi = min(lo + 4096, cols.size)
        out[lo:hi] = np.einsum("ij,ij->i", Y[rows[lo:hi]], Y[cols[lo:hi]])
    dg = rows == cols
    out[dg] = nrm[rows[dg]]
    return out / tr


# ---- widths: (D, LPR, G, NCH) with the layout each is meant to reach ---------------------------------------------------------------
WIDTHS = {
    F64: [
        (2, 1, 64, 1),      # one lane
        (3, 2, 32, 1),      # ragged: the second lane half empty
        (4, 2, 32, 1),
        (5, 4, 16, 1),      # 3 lanes < 4: the smallest row of the transposed reduction, ragged
        (9, 8, 8, 1),       # 5 < 8
        (17, 16, 4, 1),     # 9 < 16
        (33, 32, 2, 1),     # 17 < 32
        (64, 32, 2, 1),
        (65, 40, 1, 1),     # 33 < 40: the first row that is no power of two
        (80, 40, 1, 1),
        (81, 48, 1, 1),     # 41 < 48
        (98, 56, 1, 1),     # 49 < 56
        (114, 64, 1, 1),    # 57 < 64
        (128, 64, 1, 1),
        (129, 72, 1, 2),    # 65 < 72
        (258, 136, 1, 3),   # 129 < 136
        (385, 200, 1, 4),   # 193 < 200
        (512, 256, 1, 4),   # the largest row
    ],
    F32: [
        (2, 1, 64, 1),
        (3, 1, 64, 1),
        (5, 2, 32, 1),
        (9, 4, 16, 1),      # 3 < 4
        (17, 8, 8, 1),      # 5 < 8
        (33, 16, 4, 1),     # 9 < 16
        (65, 32, 2, 1),     # 17 < 32
        (129, 40, 1, 1),    # 33 < 40
        (160, 40, 1, 1),
        (161, 48, 1, 1),    # 41 < 48
        (194, 56, 1, 1),    # 49 < 56
        (225, 64, 1, 1),    # 57 < 64
        (258, 72, 1, 2),    # 65 < 72
        (513, 136, 1, 3),   # 129 < 136
        (770, 200, 1, 4),   # 193 < 200
        (1024, 256, 1, 4),  # the largest row
    ],
}
TAYLOR_WIDTHS = {F64: [65, 258, 512], F32: [129, 513, 1024]}  # k_rownorm2 at a ragged, a three-chunk and a largest row
# the rows that are no power of two and the chunked rows: one call of three iterations against three calls of one
CHUNK_WIDTHS = {dt: [D for D, LPR, G, NCH in WIDTHS[dt] if LPR in (40, 48, 56) or NCH > 1] for dt in (F64, F32)}
# the LDS-staged kernels: widths that end inside, on and one past a 128-byte and a 256-byte tile, then rows of several tiles
LDS_WIDTHS = {F64: [2, 15, 16, 17, 31, 32, 33, 80, 129], F32: [3, 31, 32, 33, 63, 64, 65, 160, 258]}


def slots(D):
    """(Z, rank_radio) with Z * rank_radio = D: Z the smallest divisor of D that is at least 2 (the tables avoid the primes above 64)."""
    Z = next(z for z in range(2, D + 1) if D % z == 0)
    return Z, D // Z


# ---- states -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state(name):
    """A state by name: built once, shared, not to be changed."""
    if name == "dense130":  # row r has 129 - r upper-triangular edges: every residue modulo G * 4, rows past 64 edges, a last row with none
        return er_contention_graph(130, 1.0, 0)
    if name == "er300":     # user 5 isolated: a diagonal-only row in the middle; other rows end at their diagonal too
        S, Q, h = er_contention_graph(300, 0.05, 3)
        S = S.tolil()
        S[5, :] = 0
        S[:, 5] = 0
        S[5, 5] = 3.7
        S = S.tocsr()
        S.eliminate_zeros()
        Q = Q.tolil()
        Q[5, :] = 0
        Q[:, 5] = 0
        Q = Q.tocsr()
        Q.eliminate_zeros()
        return S, Q, h
    if name == "k3":        # csr_cases.k3: K = 3, one edge (0, 2), an isolated row 1, no association pairs
        import csr_cases
        return csr_cases.k3()
    if name == "journal12":  # the state of test_blocked_kernels_with_narrow_and_ragged_blocks: the blocking takes it
        return journal_graph(12, 0.012, seed=5)
    raise KeyError(name)


GENERIC_STATES = ("dense130", "er300", "k3")


def widths_for(name, dtype):
    """The table rows a state runs at: all of them, on k3 those with a slot count of 2 or 3."""
    return [w for w in WIDTHS[dtype] if name != "k3" or slots(w[0])[0] <= 3]


def upper_counts(indptr, indices):
    """Per row of a CSR pattern: the entries right of the diagonal."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    return np.bincount(rows[np.asarray(indices) > rows], minlength=indptr.size - 1)


@functools.lru_cache(maxsize=None)
def sketches(name, D):
    K = state(name)[0].shape[0]
    rng = np.random.default_rng(1000 + D)
    sk = np.stack([orc.sketch_rows(rng.standard_normal((K, D))) for _ in range(NIT)])
    sk.setflags(write=False)
    return sk


@functools.lru_cache(maxsize=None)
def oracle(name, D):
    """One run of the CPU oracle per (state, width): the handles of both types and both exponentials are held to it."""
    Z, rr = slots(D)
    sk = sketches(name, D)
    o = orc.MMWOracle(nit=NIT, rank_radio=rr, eta=ETA)
    o.run(Z, state(name), lambda i, K_, D_: sk[i], keep_trace=True, factor=False)
    return o


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# Off-diagonal entries: |x_e - ref_e| <= c u sqrt(ref_aa ref_bb).  By Cauchy-Schwarz sum_j |y_aj y_bj| <= ||y_a|| ||y_b||, so a sum
# whose every product passes through at most c roundings of relative size u is within c u ||y_a|| ||y_b|| of the exact one (to first
# order), and dividing by tr turns the norms into the diagonal of X.
#   k_sddmm: a lane sums at most 16 products in double and rounds its partial to T once; at most 64 lanes are combined in T (two
#   transposed steps and a tree of at most six levels); the quotient by tr is taken in double and rounded once: ten roundings in T.
#   c = 16 for fp32; c = 32 for fp64, where the in-lane double sums (16 more) count too.
C_GENERIC = {F64: 32, F32: 16}
# Diagonal: d_k = T(sum in double), tr the double sum of those d_k (each within u of its norm, so tr is), one quotient rounded to T.
C_DIAG = 8


def c_lds(dtype, Dpad):
    """The same count for the LDS-staged kernels, which do not reduce across lanes: a thread owns an entry and walks the row's tiles.
    k_sddmm_blk (256-byte tiles): per tile 16 fused multiply-adds in a row on each accumulator in T and Dot16::total() (one add in
      fp64, two levels in fp32), the tile's sum is added in double: 16 + 2 roundings in T, the tiles' sum and the quotient in double
      rounded once.
    k_sddmm_blk2 (128-byte tiles): per tile 8 fused multiply-adds in a row, total(), and the tiles are added up in T: 8 + 2 + ntiles
      roundings, ntiles = ceil(Dpad bytes / 128); then the quotient, and the trace's own u.
    fp64: at most 16 + 1 + 5 (the tiles in double) + 2 = 24 and 8 + 1 + 9 + 2 = 20 at the widest row here (Dpad 144): within the 32 of
      the generic kernels, kept.
    fp32 (half tiles only): 8 + 2 + ntiles + 2, which is 21 at the widest row here (Dpad 288, 9 tiles): above the generic kernels' 16,
      so the bound follows the row."""
    if dtype == F64:
        return C_GENERIC[F64]
    return 12 + math.ceil(Dpad * 4 / 128)


def pattern_csr(indptr, indices, vals):
    K = len(indptr) - 1
    return scipy.sparse.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(indices), np.asarray(indptr)), shape=(K, K))
