"""States for the tests of the device CSR entry point (mmw_csr_*, mmw_create_from_csr): the smallest shapes at which the kernels of
csrc/pattern_csr_device.h can go wrong, and malformed variants of a valid K = 6 state with one field spoiled each."""
import os

import numpy as np
import scipy.sparse

from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")

I_FIELDS = ["I_L_INDPTR", "I_L_INDICES", "I_ST_INDPTR", "I_ST_INDICES", "I_GAIN_X", "I_GAIN_Y", "I_ASSO_X", "I_ASSO_Y", "I_DIAG_POS", "I_ASSO_POS"]
F_FIELDS = ["F_S_SUM", "F_NORM_H", "F_ST_DATA"]
LOOP_FIELDS = ["F_E_THIS", "F_E_ACCU", "F_Y", "F_LVAL", "F_XVAL", "F_XAVG", "F_YAVG", "F_XHALF"]
SIZES = ("K", "Z", "D", "nnzL", "nnzST", "E_gain", "E_asso", "C")


def _csr(rows, cols, vals, K):
    m = scipy.sparse.csr_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))), shape=(K, K))
    m.sort_indices()
    return m


def k2():
    """K = 2: S holds the two diagonals only, Q is the pair (0, 1): nnzL 4, nnzST 0, E_asso 1."""
    return _csr([0, 1], [0, 1], [2.0, 3.0], 2), _csr([0, 1], [1, 0], [1.0, 1.0], 2), np.ones(2)


def k3():
    """K = 3, no Q at all (null Q pointers), S the single entry (0, 2): asymmetric S, an isolated row 1: nnzL 5, nnzST 1, E_gain 1."""
    return _csr([0], [2], [0.7], 3), scipy.sparse.csr_matrix((3, 3), dtype=np.float64), np.ones(3)


def er120_zeros():
    S, Q, h = er_contention_graph(120, 0.1, 3)
    S = S.copy()
    S.data[::7] = 0.0  # stored zeros: canonical_csr keeps them
    return S, Q, h


def er120_holes():
    """every third diagonal entry of S removed"""
    S, Q, h = er_contention_graph(120, 0.1, 3)
    S = S.tocoo()
    keep = ~((S.row == S.col) & (S.row % 3 == 0))
    return _csr(S.row[keep], S.col[keep], S.data[keep], 120), Q, h


def golden(name):
    g = np.load(os.path.join(GOLDEN, "run_" + name + ".npz"), allow_pickle=False)

    def m(p):
        return scipy.sparse.csr_matrix((g[p + "_data"], g[p + "_indices"], g[p + "_indptr"]), shape=tuple(int(x) for x in g[p + "_shape"]))
    return (m("S"), m("Q"), np.array(g["h_max"])), int(g["Z"])


# name -> (builder of the state, Z)
CASES = {
    "k2": (k2, 3),
    "k3": (k3, 3),
    "er65": (lambda: er_contention_graph(65, 1.0, 0), 8),
    "er130": (lambda: er_contention_graph(130, 1.0, 0), 8),
    "er120": (lambda: er_contention_graph(120, 0.1, 3), 6),
    "er120_zeros": (er120_zeros, 6),
    "er120_holes": (er120_holes, 6),
    "golden_env75": (lambda: golden("env75")[0], golden("env75")[1]),
    "golden_er120": (lambda: golden("er120")[0], golden("er120")[1]),
    "golden_dense60": (lambda: golden("dense60")[0], golden("dense60")[1]),
    "journal16": (lambda: journal_graph(16, 0.02, seed=0), 24),
}
EXPECTED_SIZES = {"k2": dict(nnzL=4, nnzST=0, E_asso=1), "k3": dict(nnzL=5, nnzST=1, E_gain=1), "er65": dict(nnzL=4225), "er130": dict(nnzL=16900)}

_cache = {}


def case(name):
    """(state, Z) of a case: built once, shared, not to be changed."""
    if name not in _cache:
        build, Z = CASES[name]
        _cache[name] = (build(), Z)
    return _cache[name]


def sizes(s):
    return tuple(getattr(s, n) for n in SIZES)


def assert_same_pattern(a, b):
    """Every size, every integer list and the three float fields a host-only handle holds too: equal."""
    assert sizes(a) == sizes(b)
    for f in I_FIELDS:
        assert np.array_equal(a.read_i32(getattr(_lib, f)), b.read_i32(getattr(_lib, f))), f
    for f in F_FIELDS:
        assert np.array_equal(a.read(getattr(_lib, f)), b.read(getattr(_lib, f))), f


def assert_same_handle(a, b, Z, nit=3):
    """Test A's assertions: sizes, lists, the three float fields; then three device-RNG iterations bit for bit, then another slot count."""
    assert_same_pattern(a, b)
    a.iterate(nit, None, seed=5)
    b.iterate(nit, None, seed=5)
    for f in LOOP_FIELDS:
        assert np.array_equal(a.read(getattr(_lib, f)), b.read(getattr(_lib, f))), f
    a.set_slots(Z - 1, nit)
    b.set_slots(Z - 1, nit)
    assert np.array_equal(a.read(_lib.F_NORM_H), b.read(_lib.F_NORM_H))


# ---- malformed inputs: a valid K = 6 state as seven raw arrays, one field spoiled ----------------------------------------------
def valid6():
    rng = np.random.default_rng(6)
    D = rng.uniform(0.2, 2.0, size=(6, 6)) * (rng.uniform(size=(6, 6)) < 0.7)
    np.fill_diagonal(D, 3.0)
    D[4, :] = 0.0; D[:, 4] = 0.0; D[4, 4] = 3.0  # user 4 neither emits nor hears: its norm_H is |c| alone
    S = scipy.sparse.csr_matrix(D)
    S.sort_indices()
    Q = _csr([0, 1, 2, 3], [1, 0, 3, 2], [1.0] * 4, 6)
    return [S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), Q.indptr.astype(np.int32), Q.indices.astype(np.int32),
            Q.data.astype(np.float64), np.ones(6)]


def _spoil(kind):
    sp, si, sx, qp, qi, qx, h = valid6()
    K, Z = 6, 3
    row = next(k for k in range(6) if sp[k + 1] - sp[k] >= 3)  # a row of S with room to spoil
    if kind == "indptr0":
        sp[0] = 1
    elif kind == "indptr_decreasing":
        sp[2] = sp[1] - 1
    elif kind == "indptr_end":
        sp[6] -= 1
    elif kind == "column_range":
        si[sp[row] + 1] = 6
    elif kind == "unsorted":
        i = sp[row]
        si[i], si[i + 1] = si[i + 1], si[i]
    elif kind == "duplicate":
        si[sp[row] + 1] = si[sp[row]]
    elif kind == "q_zero":
        qx[0] = 0.0
    elif kind == "q_diagonal":
        qi[qp[0]] = 0
    elif kind == "q_asymmetric":  # (1, 0) goes, (0, 1) stays
        keep = np.ones(qi.size, dtype=bool)
        keep[qp[1]] = False
        qi, qx = qi[keep], qx[keep]
        qp[2:] -= 1
    elif kind == "K_below_2":
        K = 1
        sp, si, sx = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0])
        qp, qi, qx, h = np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0), np.ones(1)
    elif kind == "Z_below_2":
        Z = 1
    elif kind == "zero_norm_H":
        h[4] = 0.0
    else:
        raise KeyError(kind)
    return K, Z, [sp, si, sx, qp, qi, qx, h]


# kind -> the words build_pattern (mmw_create) uses for that input; indptr_end is the one kind mmw_create cannot see (it is never told a length)
MALFORMED = {
    "indptr0": "indptr[0] must be 0",
    "indptr_decreasing": "indptr must be non-decreasing",
    "indptr_end": "indptr[K] must equal the number of stored entries announced",
    "column_range": "S_gain column index out of range",
    "unsorted": "S_gain must be canonical CSR (sorted, no duplicates)",
    "duplicate": "S_gain must be canonical CSR (sorted, no duplicates)",
    "q_zero": "Q_asso must not store explicit zeros",
    "q_diagonal": "Q_asso must have an empty diagonal",
    "q_asymmetric": "Q_asso must be symmetric",
    "K_below_2": "K must be >= 2",
    "Z_below_2": "Z must be >= 2",
    "zero_norm_H": "norm_H has a zero entry",
}
# the kinds whose bad value is never used as an address, even by a wrong validator: the only ones a GPU test may feed the device
DEVICE_SAFE = ["unsorted", "duplicate", "q_diagonal", "q_zero", "q_asymmetric"]


def malformed(kind):
    """(K, Z, seven arrays) of the valid K = 6 state with `kind` spoiled."""
    return _spoil(kind)


def mmw_create_message(K, Z, arrays, device=-1):
    """What mmw_create itself says to the raw arrays (the Python wrapper would canonicalise them first)."""
    import ctypes as C
    sp, si, sx, qp, qi, qx, h = [np.ascontiguousarray(a) for a in arrays]
    hnd = C.c_void_p()
    rc = _lib.lib().mmw_create(C.byref(hnd), device, _lib.F64, K, Z, 2, 0.1, 3, _lib._pi(sp), _lib._pi(si), _lib._pd(sx), _lib._pi(qp), _lib._pi(qi), _lib._pd(qx), _lib._pd(h))
    if rc == 0:
        _lib.lib().mmw_destroy(hnd)
        return None
    return _lib.lib().mmw_last_error().decode()
