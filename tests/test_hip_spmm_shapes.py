"""Shapes of the generic CSR SpMM, through the stand-alone seam `mmw_expm_apply`, against SciPy's expm_multiply in fp64.

Which kernel exp(A)B runs on follows from K and from the padded row of the dense block (csrc/expm_engine.h):
  * `make_layout`: a row is LPR lanes of 16 bytes (2 fp64 / 4 fp32 columns).  LPR <= 32 is rounded up to a power of two;
    above 32 to a multiple of 8 lanes (whole 128-byte lines), and `k_spmm` then takes NCH = ceil(LPR / 64) chunks of a
    wave (at most 4: D <= 512 fp64 / 1024 fp32);
  * `slice_bytes`: for 256 <= K the block's columns are staged in LDS slices (`k_spmm_slice<T, MODE, SB>`): SB = 64 when the
    padded row is a multiple of 64 bytes and K <= 2400, else SB = 32 when it is a multiple of 32 bytes and K <= 4800.
    A 16-byte row (fp64 D <= 2, fp32 D <= 4) never takes the slice form; a 32-byte row (fp64 D 3..4, fp32 D 5..8) only
    SB = 32.  So `k_spmm` itself runs at K < 256, at K > 4800, and for 16-byte rows.

Each case names the kernel it reaches.  The matrices: symmetric Erdos-Renyi patterns scaled to one-norms 0.05, 1 and 10 (the
last one needs substeps), a hub row of more than 300 nonzeros (and so a dense column: the slice kernel's entry loop takes
256 entries per pass), empty rows including the last one, and the zero matrix.  Bars: fp64 at tol 1e-12 <= 1e-10, fp32 at
tol 1e-7 <= 2e-6 relative Frobenius.
"""
import functools

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from conftest import relerr
from sig_sdp_mmw_amd import _lib

pytestmark = pytest.mark.gpu

F64, F32 = _lib.F64, _lib.F32
SETTINGS = {F64: (1e-12, 1e-10), F32: (1e-7, 2e-6)}  # dtype: (tol, bar)
MAX_ORDER = 16

# (dtype, K, D, matrix, one-norm, kernel it reaches)
CASES = [
    # fp64: 16-byte lanes of 2 columns
    (F64, 2401, 2, "er", 1.0, "k_spmm NCH 1 (16-byte rows: no slice form)"),
    (F64, 256, 4, "er", 1.0, "k_spmm_slice SB 32 (32-byte rows)"),
    (F64, 2400, 4, "hub", 1.0, "k_spmm_slice SB 32 (32-byte rows), hub row past one entry pass"),
    (F64, 255, 16, "er", 1.0, "k_spmm NCH 1 (K < 256)"),
    (F64, 256, 16, "er", 0.05, "k_spmm_slice SB 64"),
    (F64, 1000, 16, "hub", 1.0, "k_spmm_slice SB 64, hub row past one entry pass"),
    (F64, 2400, 16, "er", 1.0, "k_spmm_slice SB 64 (largest K)"),
    (F64, 2401, 16, "er", 1.0, "k_spmm_slice SB 32 (K > 2400)"),
    (F64, 3001, 16, "empty", 1.0, "k_spmm_slice SB 32, ragged K, empty rows"),
    (F64, 4800, 16, "er", 10.0, "k_spmm_slice SB 32 (largest K), substeps"),
    (F64, 4801, 16, "er", 1.0, "k_spmm NCH 1 (K > 4800)"),
    (F64, 300, 70, "empty", 1.0, "k_spmm_slice SB 64, LPR 40"),
    (F64, 4801, 70, "er", 1.0, "k_spmm NCH 1, LPR 40"),
    (F64, 200, 200, "er", 10.0, "k_spmm NCH 2"),
    (F64, 5000, 300, "er", 0.05, "k_spmm NCH 3"),
    (F64, 4801, 500, "hub", 1.0, "k_spmm NCH 4, hub row"),
    (F64, 6000, 512, "er", 1.0, "k_spmm NCH 4 (largest D)"),
    (F64, 3001, 512, "zero", 0.0, "k_spmm_slice SB 32 (largest D), exp(0)B = B"),
    # fp32: 16-byte lanes of 4 columns
    (F32, 1000, 3, "er", 0.05, "k_spmm NCH 1 (16-byte rows: no slice form)"),
    (F32, 2000, 5, "hub", 1.0, "k_spmm_slice SB 32 (32-byte rows), hub row past one entry pass"),
    (F32, 4800, 8, "empty", 1.0, "k_spmm_slice SB 32 (32-byte rows, largest K), empty rows"),
    (F32, 256, 70, "er", 10.0, "k_spmm_slice SB 64, substeps"),
    (F32, 4801, 70, "hub", 1.0, "k_spmm NCH 1 (K > 4800), hub row"),
    (F32, 2401, 140, "er", 1.0, "k_spmm_slice SB 32, LPR 40"),
    (F32, 200, 400, "er", 1.0, "k_spmm NCH 2"),
    (F32, 4900, 600, "empty", 1.0, "k_spmm NCH 3, empty rows"),
    (F32, 128, 800, "er", 10.0, "k_spmm NCH 4"),
    (F32, 5000, 1024, "er", 1.0, "k_spmm NCH 4 (largest D)"),
    (F32, 300, 1024, "zero", 0.0, "k_spmm_slice SB 64 (largest D), exp(0)B = B"),
]


def _case_id(c):
    return "%s-K%d-D%d-%s%g" % ("f64" if c[0] == F64 else "f32", c[1], c[2], c[3], c[4])


def _scaled(A, norm):
    A = scipy.sparse.csr_matrix(A)
    A.sum_duplicates()
    A.eliminate_zeros()
    one = abs(A).sum(axis=0).max()
    return (A * (norm / one)).tocsr()


@functools.lru_cache(maxsize=None)
def matrix(K, kind, norm, seed=0):
    """Symmetric test matrices (CSR, fp64)."""
    rng = np.random.default_rng(seed + 7 * K)
    if kind == "zero":
        return scipy.sparse.csr_matrix((K, K))
    A = scipy.sparse.random(K, K, density=min(1.0, 8.0 / K), random_state=rng, data_rvs=lambda n: rng.uniform(-1.0, 1.0, n))
    A = A + A.T
    if kind == "hub":  # row h linked to 320 others: more than 256 entries in that row and in that column
        h = K // 3
        cols = rng.choice(np.setdiff1d(np.arange(K), [h]), size=320, replace=False)
        v = rng.uniform(0.5, 1.0, cols.size)
        H = scipy.sparse.csr_matrix((np.concatenate([v, v]), (np.concatenate([np.full(cols.size, h), cols]), np.concatenate([cols, np.full(cols.size, h)]))),
                                    shape=(K, K))
        A = A + H
    elif kind == "empty":  # a tenth of the rows (and columns) empty, the first and the last among them
        keep = rng.random(K) >= 0.1
        keep[0] = keep[-1] = False
        M = scipy.sparse.diags(keep.astype(np.float64))
        A = M @ A @ M
    A = _scaled(A, norm)
    if kind == "hub":
        assert np.diff(A.indptr).max() > 300
    if kind == "empty":
        assert A.indptr[-1] == A.indptr[-2] and A.indptr[1] == 0
    return A


@functools.lru_cache(maxsize=None)
def reference(K, D, kind, norm):
    B = np.random.default_rng(K + D).standard_normal((K, D))
    A = matrix(K, kind, norm)
    return B, scipy.sparse.linalg.expm_multiply(A, B)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("method", [_lib.EXPM_LANCZOS, _lib.EXPM_TAYLOR], ids=["lanczos", "taylor"])
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_expm_apply_shape_against_scipy(case, method):
    dtype, K, D, kind, norm, kernel = case
    tol, bar = SETTINGS[dtype]
    A = matrix(K, kind, norm)
    B, ref = reference(K, D, kind, norm)
    if kind != "zero":
        assert abs(abs(A).sum(axis=0).max() - norm) < 1e-9 * norm
    out, info = _lib.expm_apply(A, B, dtype=dtype, method=method, max_order=MAX_ORDER, tol=tol)
    err = relerr(out, ref)
    assert err < bar, (kernel, info, err)
    if kind == "zero":
        assert relerr(out, B) < bar, (kernel, info)
    if method == _lib.EXPM_TAYLOR and norm >= 10:
        assert info["substeps"] > 1, (kernel, info)


@pytest.mark.parametrize("dtype,D", [(F64, 513), (F32, 1025)], ids=["f64-D513", "f32-D1025"])
def test_expm_apply_rejects_a_block_wider_than_the_layout(dtype, D):
    K = 300
    A = matrix(K, "er", 1.0)
    B = np.ones((K, D))
    with pytest.raises(_lib.MMWError, match="too large"):
        _lib.expm_apply(A, B, dtype=dtype)
    # the library is still usable after the refusal
    out, info = _lib.expm_apply(A, B[:, :D - 1], dtype=dtype, tol=SETTINGS[dtype][0], max_order=MAX_ORDER)
    assert relerr(out, scipy.sparse.linalg.expm_multiply(A, B[:, :D - 1])) < SETTINGS[dtype][1], info
