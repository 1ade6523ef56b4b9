"""ctypes binding of include/mmw_hip.h (the only way the Python host reaches the GPU).

There is no CPU fallback: if `libmmw_hip.so` is missing or cannot be loaded this module raises, and
every entry point raises `MMWError` with the library's message on a non-zero status.
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmw_hip.so")

F32, F64 = 0, 1
EXPM_LANCZOS, EXPM_TAYLOR = 0, 1

# enum mmw_field / mmw_ifield
F_Y, F_E_ACCU, F_E_THIS, F_LVAL, F_XVAL, F_XAVG, F_YAVG, F_XHALF, F_SKETCH = range(9)
F_S_SUM, F_NORM_H, F_ST_DATA, F_PHASE_US, F_EXPM_INFO, F_FACTOR, F_KERNEL_US, F_BLOCKING, F_SPMM_KIND, F_E_MAX, F_DUAL_INFO = range(9, 20)
F_FACTOR_INFO = 20
F_FACTOR_CALL = 21
F_FACTOR_ROWNORM = 23
F_SPLIT_CALL = 22
F_HEAD_CALL = 24
BATCH_F_PATTERN = 25  # (named apart from the F_ ids both kinds of handle share) batches: the pattern part of the fp64 arena [2 nnzL + 4 K]: sab, sba, h_max, S_sum, 1 / norm_H, cH
BATCH_F_BUILD_INFO = 26  # batches, per instance: {0 built from host arrays / 1 on the device, 1 once the host lists are complete}
SOLVER_F_LAPLACIAN = 27  # solver handles: the Laplacian of S_gain + S_gain^T on the L pattern [nnzL]
SOLVER_F_SPECTRAL_INFO = 28  # solver handles: the last mmw_factor_spectral's record [8]
SOLVER_F_SPECTRAL_EIG = 29  # solver handles: the Ritz values it kept, ascending [Z]
SOLVER_F_GAP_INFO = 30  # solver handles: mmw_set_gap's record [6]
BATCH_MAX_PARTS = 32  # MMW_BATCH_MAX_PARTS: workgroups per instance at most (mmw_batch_set_split, mmw_batch_set_factor_split)
BATCH_MAX_ROW_PARTS = 64  # MMW_BATCH_MAX_ROW_PARTS: row parts per instance at most (mmw_batch_set_row_split)
BATCH_MAX_HEAD_PARTS = 64  # MMW_BATCH_MAX_HEAD_PARTS: head parts per instance at most (mmw_batch_set_head_split)
BATCH_EPILOGUE_MAX_K = 1024  # MMW_BATCH_EPILOGUE_MAX_K: the largest instance mmw_batch_factor / mmw_batch_round take
KERNEL_CLASSES = ["spmm", "sddmm", "dual", "loss", "krylov_vec", "sketch", "project", "greedy", "factor"]
I_L_INDPTR, I_L_INDICES, I_ST_INDPTR, I_ST_INDICES, I_GAIN_X, I_GAIN_Y, I_ASSO_X, I_ASSO_Y, I_DIAG_POS, I_ASSO_POS = range(10)
I_ROUND_LIST_BUILDS = 11  # solver handles: how often the rounding's second list set was built [1]
I_PATTERN = 10  # batches: the int32 arena of an instance [2 K + 1 + 3 nnzL + E_asso]: indptr, col, row, pair id, diag pos, pair pos

EXPORTS = ["mmw_last_error", "mmw_version", "mmw_device_count", "mmw_create", "mmw_destroy", "mmw_sizes", "mmw_set_expm",
           "mmw_set_timing", "mmw_set_profile", "mmw_bench_spmm", "mmw_reset", "mmw_set_slots", "mmw_set_slots_warm", "mmw_set_eta", "mmw_iterate", "mmw_sync", "mmw_sketch", "mmw_read_f64", "mmw_read_i32", "mmw_gap",
           "mmw_factor", "mmw_expm_apply", "mmw_sym_eig", "mmw_round", "mmw_env_create", "mmw_env_destroy", "mmw_env_sizes", "mmw_env_state",
           "mmw_env_evaluate", "mmw_create_from_env", "mmw_env_bounds", "mmw_gm_create", "mmw_gm_destroy", "mmw_gm_sizes", "mmw_gm_pass",
           "mmw_gm_run", "mmw_gm_assign", "mmw_batch_create", "mmw_batch_destroy", "mmw_batch_sizes", "mmw_batch_set_slots",
           "mmw_batch_set_slots_warm", "mmw_batch_reset", "mmw_batch_set_eta", "mmw_batch_set_expm", "mmw_batch_iterate", "mmw_batch_read_f64", "mmw_batch_read_i32",
           "mmw_batch_sketch", "mmw_batch_export", "mmw_batch_set_gap", "mmw_batch_read_gap", "mmw_batch_factor", "mmw_batch_round",
           "mmw_batch_round_randv", "mmw_batch_env_create", "mmw_batch_env_destroy", "mmw_batch_env_move", "mmw_batch_env_sizes",
           "mmw_batch_env_state", "mmw_batch_env_evaluate", "mmw_batch_round_env", "mmw_batch_gm", "mmw_batch_env_gm",
           "mmw_batch_factor_random", "mmw_batch_factor_spectral", "mmw_batch_set_split", "mmw_batch_set_factor_split", "mmw_batch_set_row_split",
           "mmw_batch_row_ranges", "mmw_batch_carry", "mmw_batch_carry_map", "mmw_batch_set_head_split", "mmw_batch_head_ranges",
           "mmw_batch_create_from_env", "mmw_batch_create_from_csr", "mmw_csr_upload", "mmw_csr_wrap", "mmw_csr_destroy", "mmw_csr_sizes", "mmw_csr_pointers", "mmw_csr_state",
           "mmw_csr_bounds", "mmw_create_from_csr", "mmw_factor_spectral", "mmw_env_move", "mmw_round_env", "mmw_gm_create_from_env", "mmw_gm_key", "mmw_carry", "mmw_carry_map",
           "mmw_round_attempts", "mmw_round_env_attempts", "mmw_round_randv", "mmw_factor_random",
           "mmw_gm_rand", "mmw_gm_rand_draw", "mmw_batch_gm_rand", "mmw_batch_env_gm_rand",
           "mmw_set_gap", "mmw_read_gap", "mmw_gap_checks", "mmw_dense_gram", "mmw_dense_gemm", "mmw_dense_chol", "mmw_dense_orth"]


class MMWError(RuntimeError):
    pass


_lib = None


def lib():
    """Load the shared library once; raise loudly if it is absent (build it with `python __graft_entry__.py`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MMWError("HIP library %s not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                       "There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    p_i32 = C.POINTER(C.c_int32)
    p_f64 = C.POINTER(C.c_double)
    L.mmw_last_error.restype = C.c_char_p
    L.mmw_last_error.argtypes = []
    L.mmw_version.restype = C.c_int
    L.mmw_device_count.argtypes = [C.POINTER(C.c_int)]
    L.mmw_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                             p_i32, p_i32, p_f64, p_i32, p_i32, p_f64, p_f64]
    L.mmw_destroy.argtypes = [C.c_void_p]
    L.mmw_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mmw_set_expm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    L.mmw_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.mmw_set_profile.argtypes = [C.c_void_p, C.c_int]
    L.mmw_bench_spmm.argtypes = [C.c_void_p, C.c_int, C.c_int, p_f64]
    L.mmw_reset.argtypes = [C.c_void_p, C.c_int32]
    L.mmw_set_slots.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.mmw_set_slots_warm.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.mmw_set_eta.argtypes = [C.c_void_p, C.c_double]
    L.mmw_carry.argtypes = [C.c_void_p, C.c_void_p]
    L.mmw_carry_map.argtypes = [C.c_void_p, C.c_void_p, p_i32, C.c_int64, p_i32, C.c_int64]
    L.mmw_iterate.argtypes = [C.c_void_p, C.c_int32, p_f64, C.c_uint64]
    L.mmw_sync.argtypes = [C.c_void_p]
    L.mmw_sketch.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, p_f64, C.c_int64]
    L.mmw_read_f64.argtypes = [C.c_void_p, C.c_int, p_f64, C.c_int64]
    L.mmw_read_i32.argtypes = [C.c_void_p, C.c_int, p_i32, C.c_int64]
    L.mmw_gap.argtypes = [C.c_void_p, p_f64]
    L.mmw_set_gap.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32]
    L.mmw_read_gap.argtypes = [C.c_void_p, p_f64, C.c_int64]
    L.mmw_gap_checks.argtypes = [C.c_int32, C.c_int32, p_i32, C.c_int32, p_i32]
    L.mmw_factor.argtypes = [C.c_void_p, C.c_int32, p_f64, C.c_uint64]
    L.mmw_factor_spectral.argtypes = [C.c_void_p, C.c_int32, C.c_int32, p_f64, C.c_uint64]
    L.mmw_factor_random.argtypes = [C.c_void_p, C.c_int32, C.c_int32, p_f64, C.c_uint64]
    L.mmw_sym_eig.argtypes = [C.c_int, C.c_int32, p_f64, C.c_double, C.c_int32, p_f64, p_f64, C.POINTER(C.c_int32)]
    L.mmw_dense_gram.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, p_f64, p_f64, C.c_int, p_f64]
    L.mmw_dense_gemm.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, p_f64, C.c_int32, p_f64, p_f64]
    L.mmw_dense_chol.argtypes = [C.c_int, C.c_int32, p_f64, p_f64, p_f64, p_f64, p_i32]
    L.mmw_dense_orth.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, p_f64, C.c_double, p_f64, p_i32]
    L.mmw_expm_apply.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int32, C.c_int32, p_i32, p_i32, p_f64,
                                 p_f64, p_f64, p_f64, C.c_int32, p_f64]
    L.mmw_round.argtypes = [C.c_void_p, C.c_int32, C.c_int32, p_f64, C.c_int32, p_f64, p_i32, p_i32]
    L.mmw_env_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, C.c_int32, p_f64, p_f64, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_double]
    L.mmw_env_destroy.argtypes = [C.c_void_p]
    L.mmw_env_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mmw_env_state.argtypes = [C.c_void_p, p_i32, p_i32, p_f64, p_i32, p_i32, p_f64, p_f64]
    L.mmw_env_evaluate.argtypes = [C.c_void_p, p_f64, C.c_int32, C.c_double, C.c_double, C.c_double, p_f64, p_f64]
    L.mmw_create_from_env.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.mmw_env_bounds.argtypes = [C.c_void_p, p_i32]
    L.mmw_env_move.argtypes = [C.c_void_p, p_f64]
    L.mmw_round_env.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, p_f64, C.c_int32, p_f64, p_i32, p_i32]
    L.mmw_round_attempts.argtypes = [C.c_void_p, C.c_int32, C.c_int32, p_f64, C.c_int32, C.c_uint64, C.c_int, p_i32, p_i32, p_i32, p_i32]
    L.mmw_round_env_attempts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, p_f64, C.c_int32, C.c_uint64, C.c_int, p_i32, p_i32, p_i32, p_i32]
    L.mmw_round_randv.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, p_f64, C.c_int64]
    L.mmw_gm_create_from_env.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
    L.mmw_gm_key.argtypes = [C.c_void_p, C.c_int, p_f64]
    for fn in (L.mmw_csr_upload, L.mmw_csr_wrap):  # (wrap's seven are device addresses: plain integers here)
        fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, C.c_int64, C.c_int64] + [C.c_void_p] * 7
    L.mmw_csr_destroy.argtypes = [C.c_void_p]
    L.mmw_csr_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mmw_csr_pointers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mmw_csr_state.argtypes = [C.c_void_p, p_i32, p_i32, p_f64, p_i32, p_i32, p_f64, p_f64]
    L.mmw_csr_bounds.argtypes = [C.c_void_p, p_i32]
    L.mmw_create_from_csr.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.mmw_gm_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, p_i32, p_i32, p_f64, p_i32, p_i32, p_f64, p_f64]
    L.mmw_gm_destroy.argtypes = [C.c_void_p]
    L.mmw_gm_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mmw_gm_pass.argtypes = [C.c_void_p, p_i32, C.c_int32, C.c_int32, p_i32, p_i32]
    L.mmw_gm_run.argtypes = [C.c_void_p, p_f64, C.c_int32, C.c_int32, p_i32, p_i32, p_i32]
    L.mmw_gm_assign.argtypes = [C.c_void_p, C.c_int32, p_i32, p_i32, p_i32, p_i32]
    L.mmw_gm_rand.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int, p_i32, p_i32, p_i32]
    L.mmw_gm_rand_draw.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, p_f64, p_f64]
    pp_i32 = C.POINTER(p_i32)
    pp_f64 = C.POINTER(p_f64)
    L.mmw_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, p_i32, p_i32, C.c_int32, C.c_double, p_i32,
                                   pp_i32, pp_i32, pp_f64, pp_i32, pp_i32, pp_f64, pp_f64]
    L.mmw_batch_destroy.argtypes = [C.c_void_p]
    L.mmw_batch_sizes.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    L.mmw_batch_set_slots.argtypes = [C.c_void_p, p_i32, C.c_int32]
    L.mmw_batch_set_slots_warm.argtypes = [C.c_void_p, p_i32, C.c_int32]
    L.mmw_batch_carry.argtypes = [C.c_void_p, C.c_void_p, p_i32]
    L.mmw_batch_carry_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, p_i32, C.c_int64, p_i32, C.c_int64]
    L.mmw_batch_reset.argtypes = [C.c_void_p, C.c_int32]
    L.mmw_batch_set_eta.argtypes = [C.c_void_p, p_f64]
    L.mmw_batch_set_expm.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.mmw_batch_iterate.argtypes = [C.c_void_p, C.c_int32, p_f64, C.POINTER(C.c_uint64)]
    L.mmw_batch_read_f64.argtypes = [C.c_void_p, C.c_int32, C.c_int, p_f64, C.c_int64]
    L.mmw_batch_read_i32.argtypes = [C.c_void_p, C.c_int32, C.c_int, p_i32, C.c_int64]
    L.mmw_batch_sketch.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, p_f64, C.c_int64]
    L.mmw_batch_export.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.mmw_batch_set_gap.argtypes = [C.c_void_p, C.c_int, C.c_int32]
    L.mmw_batch_read_gap.argtypes = [C.c_void_p, C.c_int32, p_f64, C.c_int64]
    L.mmw_batch_set_split.argtypes = [C.c_void_p, p_i32]
    L.mmw_batch_set_factor_split.argtypes = [C.c_void_p, p_i32]
    L.mmw_batch_set_row_split.argtypes = [C.c_void_p, p_i32]
    L.mmw_batch_row_ranges.argtypes = [C.c_void_p, C.c_int32, C.c_int32, p_i32]
    L.mmw_batch_set_head_split.argtypes = [C.c_void_p, p_i32]
    L.mmw_batch_head_ranges.argtypes = [C.c_void_p, C.c_int32, C.c_int32, p_i32]
    L.mmw_batch_factor.argtypes = [C.c_void_p, p_i32, p_i32, pp_f64]
    L.mmw_batch_round.argtypes = [C.c_void_p, p_i32, C.c_int32, C.c_int, C.POINTER(C.c_uint64), p_i32, p_i32, p_i32]
    L.mmw_batch_round_randv.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, p_f64, C.c_int64]
    L.mmw_batch_env_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, p_i32, p_i32, pp_f64, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_double]
    L.mmw_batch_env_destroy.argtypes = [C.c_void_p]
    L.mmw_batch_env_move.argtypes = [C.c_void_p, pp_f64]
    L.mmw_batch_env_sizes.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    L.mmw_batch_env_state.argtypes = [C.c_void_p, C.c_int32, p_i32, p_i32, p_f64, p_i32, p_i32, p_f64, p_f64]
    L.mmw_batch_env_evaluate.argtypes = [C.c_void_p, pp_f64, p_i32, C.c_double, C.c_double, C.c_double, pp_f64, pp_f64]
    L.mmw_batch_round_env.argtypes = [C.c_void_p, C.c_void_p, p_i32, C.c_int32, C.c_int, C.POINTER(C.c_uint64), p_i32, p_i32, p_i32]
    L.mmw_batch_gm.argtypes = [C.c_void_p, C.c_int, p_i32, p_i32, C.c_int32, p_i32, p_i32, p_i32, p_f64]
    L.mmw_batch_env_gm.argtypes = [C.c_void_p, C.c_int, p_i32, p_i32, C.c_int32, p_i32, p_i32, p_i32, p_f64]
    L.mmw_batch_gm_rand.argtypes = [C.c_void_p, p_i32, p_i32, C.c_int32, C.c_int, C.POINTER(C.c_uint64), p_i32, p_i32, p_i32]
    L.mmw_batch_env_gm_rand.argtypes = [C.c_void_p, p_i32, p_i32, C.c_int32, C.c_int, C.POINTER(C.c_uint64), p_i32, p_i32, p_i32]
    L.mmw_batch_factor_random.argtypes = [C.c_void_p, p_i32, C.POINTER(C.c_uint64)]
    L.mmw_batch_factor_spectral.argtypes = [C.c_void_p, p_i32, p_i32]
    L.mmw_batch_create_from_env.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, p_i32, C.c_int32, C.c_double, p_i32]
    L.mmw_batch_create_from_csr.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), p_i32, C.c_int32, C.c_double, p_i32]
    for name in EXPORTS:
        if name not in ("mmw_last_error",):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise MMWError("mmw_hip status %d: %s" % (rc, lib().mmw_last_error().decode("utf-8", "replace")))


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _u64(seeds, B):
    """One uint64 seed per instance, from one for all or one each."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (B,)))


def _pu(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _opt_pi(t):
    return None if t is None else _pi(t)


def _gm_call(fn, handle, B, Ks, who, kind, Zs, nattempt, t, keys):
    """mmw_batch_gm / mmw_batch_env_gm: (z list with None for instances left out, ZZ int32[B], rem int32[B][, keys list])."""
    Z = _i32(np.broadcast_to(np.asarray(Zs, dtype=np.int32), (B,)))
    n = max(1, sum(Ks[i] for i in who))
    zflat = np.empty(n, dtype=np.int32)
    kflat = np.empty(n, dtype=np.float64) if keys else None
    zz = np.empty(B, dtype=np.int32)
    rem = np.empty(B, dtype=np.int32)
    check(fn(handle, int(kind), _opt_pi(t), _pi(Z), int(nattempt), _pi(zflat), _pi(zz), _pi(rem), _pd(kflat) if keys else None))
    z, ks, o = [None] * B, [None] * B, 0
    for i in who:
        z[i] = zflat[o:o + Ks[i]]
        if keys:
            ks[i] = kflat[o:o + Ks[i]]
        o += Ks[i]
    return (z, zz, rem, ks) if keys else (z, zz, rem)


def _gm_rand_call(fn, handle, B, Ks, who, Zs, seeds, nattempt, t, stop_at_first):
    """mmw_batch_gm_rand / mmw_batch_env_gm_rand in `BatchSolver.round`'s shapes: (z, rem, used) with z[i] None for an instance left
    out (by `take` or by Z <= 0) or int32 (nattempt, K) with -1 = left over and -2 = attempt not run."""
    Z = _i32(np.broadcast_to(np.asarray(Zs, dtype=np.int32), (B,)))
    nattempt = int(nattempt)
    ran = [i for i in who if Z[i] > 0]
    zflat = np.empty(max(1, nattempt * sum(Ks[i] for i in ran)), dtype=np.int32)
    rem = np.empty((B, max(1, nattempt)), dtype=np.int32)
    used = np.empty(B, dtype=np.int32)
    check(fn(handle, _opt_pi(t), _pi(Z), nattempt, 1 if stop_at_first else 0, _pu(_u64(seeds, B)), _pi(zflat), _pi(rem), _pi(used)))
    z, o = [None] * B, 0
    for i in ran:
        z[i] = zflat[o:o + nattempt * Ks[i]].reshape(nattempt, Ks[i])
        o += nattempt * Ks[i]
    return z, rem, used


def device_count():
    n = C.c_int(0)
    check(lib().mmw_device_count(C.byref(n)))
    return n.value


def canonical_csr(m):
    """scipy CSR with sorted, de-duplicated indices as int32/float64 arrays (copies only when needed)."""
    import scipy.sparse
    m = scipy.sparse.csr_matrix(m)
    if not m.has_canonical_format:
        m = m.copy()
        m.sum_duplicates()
    return _i32(m.indptr), _i32(m.indices), _f64(m.data)


def _state_arrays(state):
    """(K, (S indptr, indices, data, Q indptr, indices, data, h_max)): a state's seven canonical arrays after its shape check."""
    S, Q, h = state
    K = int(S.shape[0])
    if S.shape != (K, K) or Q.shape != (K, K) or len(h) != K:
        raise MMWError("state must be (S_gain KxK, Q_asso KxK, h_max[K])")
    return K, canonical_csr(S) + canonical_csr(Q) + (_f64(h),)


def _state_out(K, nnzS, nnzQ, fill):
    """(S_gain csr, Q_asso csr, h_max) from the seven arrays `fill(sp, si, sx, qp, qi, qx, h)` writes (mmw_env_state / mmw_batch_env_state)."""
    import scipy.sparse
    sp = np.empty(K + 1, dtype=np.int32); si = np.empty(nnzS, dtype=np.int32); sx = np.empty(nnzS, dtype=np.float64)
    qp = np.empty(K + 1, dtype=np.int32); qi = np.empty(nnzQ, dtype=np.int32); qx = np.empty(nnzQ, dtype=np.float64)
    h = np.empty(K, dtype=np.float64)
    fill(_pi(sp), _pi(si), _pd(sx), _pi(qp), _pi(qi), _pd(qx), _pd(h))
    return scipy.sparse.csr_matrix((sx, si, sp), shape=(K, K)), scipy.sparse.csr_matrix((qx, qi, qp), shape=(K, K)), h


# mmw_read_f64 / mmw_read_i32: the size a field's length is (mmw_sizes' names), for the int fields (size, + offset)
_SIZE_NAMES = ("K", "Z", "D", "Dpad", "nnzL", "nnzST", "E_gain", "E_asso", "C", "iter")
_LEN = {F_Y: "C", F_E_ACCU: "C", F_E_THIS: "C", F_LVAL: "nnzL", F_XVAL: "nnzL", F_XAVG: "nnzL", F_YAVG: "C",
        F_S_SUM: "K", F_NORM_H: "K", F_ST_DATA: "nnzST", SOLVER_F_LAPLACIAN: "nnzL", F_FACTOR_ROWNORM: "K"}
_ILEN = {I_L_INDPTR: ("K", 1), I_L_INDICES: ("nnzL", 0), I_ST_INDPTR: ("K", 1), I_ST_INDICES: ("nnzST", 0), I_GAIN_X: ("E_gain", 0),
         I_GAIN_Y: ("E_gain", 0), I_ASSO_X: ("E_asso", 0), I_ASSO_Y: ("E_asso", 0), I_DIAG_POS: ("K", 0), I_ASSO_POS: ("E_asso", 0)}


def gap_checks(K, m_cap=0):
    """The Lanczos steps at which a logged gap row of (K, m_cap) is checked (mmw_gap_checks; needs no device)."""
    n = C.c_int32(0)
    check(lib().mmw_gap_checks(int(K), int(m_cap), None, 0, C.byref(n)))
    out = np.empty(n.value, dtype=np.int32)
    check(lib().mmw_gap_checks(int(K), int(m_cap), _pi(out), int(out.size), C.byref(n)))
    return [int(x) for x in out]


class _Handle:
    """What the owning wrappers share: `_h`, the handle; `_destroy`, the name of the C entry that frees it."""
    _destroy = None

    def _closing(self):
        """Called by `close` while the handle is still valid."""

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            try:
                self._closing()
            finally:
                getattr(lib(), self._destroy)(self._h)
                self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Solver(_Handle):
    """Owning wrapper of one `mmw_solver*` handle."""
    _destroy = "mmw_destroy"

    def __init__(self, Z, state, nit, eta, rank_radio=2, dtype=F64, device=0):
        self.K, (sp, si, sx, qp, qi, qx, hm) = _state_arrays(state)
        self._h = C.c_void_p()
        check(lib().mmw_create(C.byref(self._h), int(device), int(dtype), self.K, int(Z), int(rank_radio), float(eta), int(nit),
                               _pi(sp), _pi(si), _pd(sx), _pi(qp), _pi(qi), _pd(qx), _pd(hm)))
        self._load_sizes()
        self.dtype = dtype
        self._timing = False
        self._timed = 0

    @classmethod
    def from_env(cls, env, Z, nit, eta, rank_radio=2, dtype=F64):
        """The handle for the state a DeviceEnv holds, built on the device without the host round trip (mmw_create_from_env)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        check(lib().mmw_create_from_env(C.byref(self._h), env._h, int(dtype), int(Z), int(rank_radio), float(eta), int(nit)))
        self._load_sizes()
        self.dtype = dtype
        self._timing = False
        self._timed = 0
        return self

    @classmethod
    def from_csr(cls, csr, Z, nit, eta, rank_radio=2, dtype=F64):
        """The handle for the state a DeviceCSR holds, built on the device from its seven arrays (mmw_create_from_csr): bit for bit
        the handle `Solver(Z, csr.state(), ...)` is."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        check(lib().mmw_create_from_csr(C.byref(self._h), csr._h, int(dtype), int(Z), int(rank_radio), float(eta), int(nit)))
        self._load_sizes()
        self.dtype = dtype
        self._timing = False
        self._timed = 0
        return self

    def _sizes(self):
        sz = (C.c_int64 * 10)()
        check(lib().mmw_sizes(self._h, sz))
        return [int(x) for x in sz]

    def _load_sizes(self):
        (self.K, self.Z, self.D, self.Dpad, self.nnzL, self.nnzST, self.E_gain, self.E_asso, self.C, _) = self._sizes()

    def _closing(self):
        self._keep_resident_factor()

    @property
    def iterations_done(self):
        return self._sizes()[9]

    def set_expm(self, method=EXPM_LANCZOS, max_order=12, tol=1e-9):
        check(lib().mmw_set_expm(self._h, int(method), int(max_order), float(tol)))

    def set_timing(self, on):
        """False / 0: off; True / 1: phase events in every iteration; S > 1: in one iteration of every S (rows repeated in between)."""
        check(lib().mmw_set_timing(self._h, int(on)))
        self._timing = bool(on)

    def set_profile(self, on):
        """False / 0: off; True / 1: synchronous mode with exact launch counts; 2: the shipped path as launched."""
        check(lib().mmw_set_profile(self._h, int(on)))

    def kernel_times(self):
        """{class: (total device us, launches)} since set_profile(True)."""
        self.sync()
        v = self.read(F_KERNEL_US, 2 * len(KERNEL_CLASSES))
        return {k: (float(v[2 * i]), int(v[2 * i + 1])) for i, k in enumerate(KERNEL_CLASSES)}

    def bench_spmm(self, blocked=True, reps=20):
        us = C.c_double(0.0)
        check(lib().mmw_bench_spmm(self._h, int(blocked), int(reps), C.byref(us)))
        return us.value

    def reset(self, nit):
        check(lib().mmw_reset(self._h, int(nit)))
        self._timed = 0

    def set_eta(self, eta):
        check(lib().mmw_set_eta(self._h, float(eta)))

    def spmm_kernel_info(self):
        """Which SpMM kernel exp(L/2)R runs on for this handle, and what bounds it (for the benchmark's roofline record)."""
        kind = int(self.read(F_SPMM_KIND, 2)[0])
        return [
            {"name": "k_spmm (generic CSR gather SpMM)", "limiter": "L2 gather rate of the dense rows"},
            {"name": "k_spmm_blk (LDS-staged locality-blocked CSR SpMM, 256-byte tiles)", "limiter": "VALU issue + LDS latency"},
            {"name": "k_spmm_blk2 (LDS-staged locality-blocked CSR SpMM, 128-byte half tiles)",
             "limiter": "VALU issue + LDS latency; operands live in L2 / Infinity Cache, not HBM"},
            {"name": "k_spmm_mfma (locality blocks as dense bf16 hi/lo -- first-order form: fp16 -- products on the matrix cores)",
             "limiter": "gather of the blocks' union rows into LDS at the CU's L2 rate; operands live in L2 / Infinity Cache, not HBM"},
        ][kind]

    def set_slots(self, Z, nit, warm=False):
        """Rebind to another slot count on the same state (keeps pattern, blocking and device copies).
        warm=True continues from the previous probe's iterate (mmw_set_slots_warm)."""
        check((lib().mmw_set_slots_warm if warm else lib().mmw_set_slots)(self._h, int(Z), int(nit)))
        self._load_sizes()
        self._timed = 0

    def carry_from(self, src):
        """mmw_carry: take over the iterate (e_accu, L, X, Y) of `src`, a handle of the same users on the state they were in before
        they moved, into this handle, which has not iterated: L and X by (row, col), e_accu and Y by user and by association pair, 0
        for what `src` does not hold, matched on the device; Y is not renormalised.  The sums restart as `set_slots(..., warm=True)`
        leaves them (xavg = xval, yavg = Y), `iterations_done` stays 0 and `nit` is unchanged; this handle's first chunk is planned on
        `src`'s history.  A `src` that never iterated leaves this handle cold.  `src` is only read, and the call returns after the
        device's work: `src` may be iterated, reset or closed at once."""
        check(lib().mmw_carry(self._h, src._h))

    def carry_map(self, src):
        """mmw_carry_map: (lmap int32[nnzL], cmap int32[C]) -- for every entry of this handle's L pattern and of its constraint
        vector the position in `src`'s, -1 where `src` holds none.  Computed on the host; works on device=-1 handles."""
        lmap = np.empty(self.nnzL, dtype=np.int32)
        cmap = np.empty(self.C, dtype=np.int32)
        check(lib().mmw_carry_map(self._h, src._h, _pi(lmap), int(lmap.size), _pi(cmap), int(cmap.size)))
        return lmap, cmap

    def iterate(self, n, randv=None, seed=0):
        if self._timing:
            self._timed += int(n)
        if randv is None:
            check(lib().mmw_iterate(self._h, int(n), None, C.c_uint64(int(seed))))
        else:
            r = _f64(randv)
            if r.size != n * self.K * self.D:
                raise MMWError("randv must hold n*K*D = %d values, got %d" % (n * self.K * self.D, r.size))
            check(lib().mmw_iterate(self._h, int(n), _pd(r), C.c_uint64(0)))

    def sync(self):
        check(lib().mmw_sync(self._h))

    def sketch(self, seed, iteration):
        """The (K, D) sketch the device generator draws for `iteration` of a run with `seed` (counter-based: exact, any chunking)."""
        out = np.empty((self.K, self.D), dtype=np.float64)
        check(lib().mmw_sketch(self._h, C.c_uint64(int(seed)), int(iteration), _pd(out), int(out.size)))
        return out

    _LEN = _LEN

    def read(self, which, n=None):
        if n is None:
            if which in (F_XHALF, F_SKETCH):
                n = self.K * self.D
            elif which in (F_EXPM_INFO, F_BLOCKING):
                n = 4
            elif which == F_SPMM_KIND:
                n = 2
            elif which == F_DUAL_INFO:
                n = 4
            elif which == F_E_MAX:
                n = 1
            elif which == F_PHASE_US:
                n = 4 * self._timed_iters()
            else:
                n = getattr(self, self._LEN[which])
        out = np.empty(int(n), dtype=np.float64)
        check(lib().mmw_read_f64(self._h, int(which), _pd(out), int(n)))
        if which in (F_XHALF, F_SKETCH):
            out = out.reshape(self.K, self.D)
        return out

    def _timed_iters(self):
        return self._timed

    _ILEN = _ILEN

    def read_i32(self, which):
        name, off = self._ILEN[which]
        n = getattr(self, name) + off
        out = np.empty(int(n), dtype=np.int32)
        check(lib().mmw_read_i32(self._h, int(which), _pi(out), int(n)))
        return out

    def gap(self):
        out = np.empty(3, dtype=np.float64)
        check(lib().mmw_gap(self._h, _pd(out)))
        return out

    def set_gap(self, on=True, m_cap=0, first_steps=0):
        """Log the duality gap (mmw.py:79-117) of every iteration that follows, inside the loop (mmw_set_gap); m_cap <= 0: 600 steps.
        first_steps: how far a row is enqueued before any row of the run has been read back (<= 0: the cap); it changes no row."""
        check(lib().mmw_set_gap(self._h, 1 if on else 0, int(m_cap), int(first_steps)))

    def gap_log(self):
        """(rows[n, 3], steps[n]) of the n iterations done, like `BatchSolver.gap_log`: {e_max, K lambda_min(L(Ybar)), difference} --
        columns 3:6 of the reference's LOGGED_NP_DATA["gap"] -- and the Lanczos steps taken (negative: the cap was reached first).
        Rows of iterations that ran with the gap off are NaN (steps 0)."""
        n = self.iterations_done
        out = np.empty((n, 4), dtype=np.float64)
        check(lib().mmw_read_gap(self._h, _pd(out), int(out.size)))
        return out[:, :3].copy(), out[:, 3].astype(np.int64)

    def gap_info(self):
        """MMW_F_GAP_INFO: what the logged gap has cost since the handle was made."""
        v = self.read(SOLVER_F_GAP_INFO, 6)
        return {"rows": int(v[0]), "continued": int(v[1]), "capped": int(v[2]), "launches": int(v[3]), "max_steps": int(v[4]), "bytes": int(v[5])}

    def factor(self, rank, seed=0, resident=False):
        """X_half (K, rank) float64.  resident=True: a `DeviceFactor` -- the factor stays on the device, `round` takes it from there,
        and it becomes a NumPy array (one copy out) the moment anything else looks at it."""
        self._keep_resident_factor()
        if resident:
            check(lib().mmw_factor(self._h, int(rank), None, C.c_uint64(int(seed))))
            self._factor_serial, self._last_rank = getattr(self, "_factor_serial", 0) + 1, int(rank)
            df = DeviceFactor(self, int(rank), self._factor_serial)
            self._resident = weakref.ref(df)
            return df
        out = np.empty((self.K, int(rank)), dtype=np.float64)
        check(lib().mmw_factor(self._h, int(rank), _pd(out), C.c_uint64(int(seed))))
        self._factor_serial, self._last_rank = getattr(self, "_factor_serial", 0) + 1, int(rank)
        return out

    def factor_spectral(self, Z, seed=0, resident=False, index_order=False):
        """spectral_sdp_solver.run_with_state (sdp_solver.py:165-185) on this handle's state, any K (mmw_factor_spectral): the K x Z
        block of the Laplacian's Z eigenvectors of largest eigenvalue, columns in ascending eigenvalue (signs arbitrary), every row
        divided by its norm; an exactly zero row stays zero.  index_order=True: `rand_sdp_solver.index_ordered` of that block, bit for
        bit.  resident=True: a `DeviceFactor` (its `index_ordered` says which of the two it is) that `round` reads where it lies.
        The handle's own slot count plays no part."""
        self._keep_resident_factor()
        Z, io = int(Z), 1 if index_order else 0
        if resident:
            check(lib().mmw_factor_spectral(self._h, Z, io, None, C.c_uint64(int(seed))))
            self._factor_serial, self._last_rank = getattr(self, "_factor_serial", 0) + 1, Z
            df = DeviceFactor(self, Z, self._factor_serial, index_ordered=bool(io))
            self._resident = weakref.ref(df)
            return df
        out = np.empty((self.K, max(Z, 0)), dtype=np.float64)  # (a Z out of range is the library's to refuse)
        check(lib().mmw_factor_spectral(self._h, Z, io, _pd(out), C.c_uint64(int(seed))))
        self._factor_serial, self._last_rank = getattr(self, "_factor_serial", 0) + 1, Z
        return out

    def factor_random(self, cols, seed, resident=False, index_order=False):
        """rand_sdp_solver.run_with_state (sdp_solver.py:109-114) on this handle, any K (mmw_factor_random): a K x cols float64 block of
        standard normals with its rows normalised, drawn on the device -- the fp64 sketch of (seed, iteration 0), bitwise what
        `BatchSolver.factor_random` leaves for that seed, whatever this handle's dtype.  index_order=True:
        `rand_sdp_solver.index_ordered` of that block, bit for bit.  resident=True: a `DeviceFactor` (its `index_ordered` says which of
        the two it is) that `round` reads where it lies.  The iterate, its sums and a chunk in flight are not touched."""
        self._keep_resident_factor()
        cols, io = int(cols), 1 if index_order else 0
        if resident:
            check(lib().mmw_factor_random(self._h, cols, io, None, C.c_uint64(int(seed))))
            self._factor_serial, self._last_rank = getattr(self, "_factor_serial", 0) + 1, cols
            df = DeviceFactor(self, cols, self._factor_serial, index_ordered=bool(io))
            self._resident = weakref.ref(df)
            return df
        out = np.empty((self.K, max(cols, 0)), dtype=np.float64)  # (a width out of range is the library's to refuse)
        check(lib().mmw_factor_random(self._h, cols, io, _pd(out), C.c_uint64(int(seed))))
        self._factor_serial, self._last_rank = getattr(self, "_factor_serial", 0) + 1, cols
        return out

    def laplacian(self):
        """The Laplacian of S_gain + S_gain^T (diagonal zeroed) on the L pattern, float64 [nnzL] in `read_i32(I_L_INDICES)`'s order
        (MMW_F_LAPLACIAN); a device = -1 handle answers it too."""
        return self.read(SOLVER_F_LAPLACIAN)

    def spectral_info(self):
        """The last `factor_spectral`: {"outer", "resid", "Z", "block", "theta_Z", "theta_next" (0 when block = Z), "mfma_passes"}."""
        v = self.read(SOLVER_F_SPECTRAL_INFO, 8)
        return {"outer": int(v[0]), "resid": float(v[1]), "Z": int(v[2]), "block": int(v[3]), "theta_Z": float(v[4]), "theta_next": float(v[5]),
                "mfma_passes": int(v[6])}

    def spectral_eig(self, Z):
        """The Z Ritz values the last `factor_spectral` kept, ascending (the block's column order)."""
        return self.read(SOLVER_F_SPECTRAL_EIG, int(Z))

    def factor_row_norms(self):
        """After `factor_spectral`: every user's row norm of the eigenvector block before its rows were normalised
        (MMW_F_FACTOR_ROWNORM); status -3 after any other factor."""
        return self.read(F_FACTOR_ROWNORM)

    def _keep_resident_factor(self):
        """A resident factor somebody still holds is copied out before the handle overwrites it (next factor) or goes away (close)."""
        ref = getattr(self, "_resident", None)
        df = ref() if ref is not None else None
        if df is not None and df._host is None and getattr(self, "_h", None) is not None and self._h.value:
            np.asarray(df)
        self._resident = None

    def round(self, Z, gX, randv):
        """randv: (nbatch, Z, D') row-normalised; returns (z[nbatch,K] int32 with -1 = unassigned, rem[nbatch])."""
        return self._round(None, Z, gX, randv)

    def round_env(self, env, Z, gX, randv):
        """`round` against the state the DeviceEnv `env` holds now (mmw_round_env): the handle's factor -- gX, or a resident
        `DeviceFactor` of this handle read where it lies -- rounded on the moved stations, the lists built on the device from the
        environment's CSR and kept until it moves again.  The handle's own state, iterate and factor stay as they are."""
        return self._round(env, Z, gX, randv)

    def _round(self, env, Z, gX, randv):
        on_device = isinstance(gX, DeviceFactor) and gX.on_device_of(self)
        if not on_device:
            gX = _f64(gX)
        randv = _f64(randv)
        if randv.ndim == 2:
            randv = randv[None]
        nb, Zr, Dp = randv.shape
        if Zr != Z or tuple(gX.shape) != (self.K, Dp):
            raise MMWError("round: gX must be (K, D') and randv (nbatch, Z, D')")
        z = np.empty((nb, self.K), dtype=np.int32)
        rem = np.empty(nb, dtype=np.int32)
        args = (int(Z), int(Dp), None if on_device else _pd(gX), int(nb), _pd(randv), _pi(z), _pi(rem))
        if env is None:
            check(lib().mmw_round(self._h, *args))
        else:
            check(lib().mmw_round_env(self._h, env._h, *args))
        return z, rem

    PICK_RULES = {"first": 0, "fewest": 1}

    def round_attempts(self, Z, gX, nattempt, seed, pick="first", all_attempts=False):
        """All `nattempt` attempts of one `sdp_solver.rounding` call (sdp_solver.py:18-25) in one device call (mmw_round_attempts):
        attempt a rounds with the Z x D' directions drawn on the device from Philox keyed by (seed, a) -- `round_randv(Z, D', seed,
        a)`, whatever nattempt is -- and the device picks one.  pick="first", the reference's rule: the lowest attempt that leaves
        nobody over, else the last, i.e. what the loop over single attempts with stop-at-first returns; "fewest" (not the
        reference's): the attempt with the fewest users left over, ties to the lower attempt.  gX: an array, a resident
        `DeviceFactor` of this handle, or None for the factor the handle computed last (read where it lies; D' is its rank).
        Returns (z int32[K] with -1 = left over, rem int32[nattempt], pick), plus z_all int32[nattempt, K] with all_attempts=True."""
        return self._round_attempts(None, Z, gX, nattempt, seed, pick, all_attempts)

    def round_env_attempts(self, env, Z, gX, nattempt, seed, pick="first", all_attempts=False):
        """`round_attempts` against the state the DeviceEnv `env` holds now (mmw_round_env_attempts), with `round_env`'s list cache."""
        return self._round_attempts(env, Z, gX, nattempt, seed, pick, all_attempts)

    def _round_attempts(self, env, Z, gX, nattempt, seed, pick, all_attempts):
        if pick not in self.PICK_RULES:
            raise MMWError("round_attempts: pick must be 'first' or 'fewest', got %r" % (pick,))
        on_device = gX is None or (isinstance(gX, DeviceFactor) and gX.on_device_of(self))
        if gX is None:  # the factor this handle computed last, of the rank it was asked for (none yet: the library refuses)
            Dp = getattr(self, "_last_rank", 1)
        else:
            if not on_device:
                gX = _f64(gX)
            if len(gX.shape) != 2 or gX.shape[0] != self.K:
                raise MMWError("round_attempts: gX must be (K, D')")
            Dp = int(gX.shape[1])
        nattempt = int(nattempt)
        z = np.empty(self.K, dtype=np.int32)
        rem = np.empty(max(nattempt, 1), dtype=np.int32)
        z_all = np.empty((max(nattempt, 1), self.K), dtype=np.int32) if all_attempts else None
        picked = C.c_int32(-1)
        args = (int(Z), Dp, None if on_device else _pd(gX), nattempt, C.c_uint64(int(seed)), self.PICK_RULES[pick], _pi(z), _pi(rem), C.byref(picked),
                _opt_pi(z_all))
        if env is None:
            check(lib().mmw_round_attempts(self._h, *args))
        else:
            check(lib().mmw_round_env_attempts(self._h, env._h, *args))
        return (z, rem, int(picked.value)) + ((z_all,) if all_attempts else ())

    def round_list_builds(self):
        """How often `round_env` / `round_env_attempts` built this handle's second list set (MMW_I_ROUND_LIST_BUILDS): once per
        (environment, generation) they met in turn."""
        out = np.empty(1, dtype=np.int32)
        check(lib().mmw_read_i32(self._h, I_ROUND_LIST_BUILDS, _pi(out), 1))
        return int(out[0])

    def round_randv(self, Z, Dp, seed, attempt):
        """The Z x D' row-normalised directions attempt `attempt` of a `round_attempts(..., seed)` call rounds with (mmw_round_randv):
        the same kernel run for that one attempt, float64."""
        out = np.empty((max(int(Z), 0), max(int(Dp), 0)), dtype=np.float64)
        check(lib().mmw_round_randv(self._h, int(Z), int(Dp), C.c_uint64(int(seed)), int(attempt), _pd(out), int(out.size)))
        return out


class BatchSolver(_Handle):
    """Owning wrapper of one `mmw_batch*`: B small fp64 instances, one workgroup each, `n` iterations per launch
    (csrc/kernels_batch.h).  Mirrors `Solver` with an instance index on every per-instance call.  `nit` is one count for all
    instances or one per instance; Zs one slot count per instance."""
    _destroy = "mmw_batch_destroy"

    def __init__(self, Zs, states, nit, eta, rank_radio=2, device=0):
        self.B = B = len(states)
        if B < 1 or len(Zs) != B:
            raise MMWError("BatchSolver: one slot count per state, at least one state")
        nits = np.broadcast_to(np.asarray(nit, dtype=np.int32), (B,))
        self._keep = []
        arrays = {k: [] for k in ("sp", "si", "sx", "qp", "qi", "qx", "h")}
        Ks = []
        for state in states:
            K, seven = _state_arrays(state)
            Ks.append(K)
            for k, a in zip(("sp", "si", "sx", "qp", "qi", "qx", "h"), seven):
                arrays[k].append(a)
        self._keep.append(arrays)

        def ptrs(name, ctype):
            arr = (C.POINTER(ctype) * B)(*[a.ctypes.data_as(C.POINTER(ctype)) for a in arrays[name]])
            self._keep.append(arr)
            return arr
        Karr, Zarr, narr = _i32(Ks), _i32(Zs), _i32(nits)
        self._h = C.c_void_p()
        check(lib().mmw_batch_create(C.byref(self._h), int(device), B, _pi(Karr), _pi(Zarr), int(rank_radio), float(eta), _pi(narr),
                                     ptrs("sp", C.c_int32), ptrs("si", C.c_int32), ptrs("sx", C.c_double),
                                     ptrs("qp", C.c_int32), ptrs("qi", C.c_int32), ptrs("qx", C.c_double), ptrs("h", C.c_double)))
        self._keep = None
        self._created(device, nits)

    @classmethod
    def from_env(cls, env, Zs, nit, eta, rank_radio=2):
        """The batch for the states a `BatchEnv` holds after its last move, built on the environment's device without the host round
        trip (mmw_batch_create_from_env): the object `BatchSolver(Zs, [env.state(i) for i in range(env.B)], nit, eta, rank_radio)`
        gives, field for field.  It keeps nothing of `env`, which may move on at once."""
        B = int(env.B)
        if len(Zs) != B:
            raise MMWError("BatchSolver.from_env: %d slot counts for the environment's %d instances" % (len(Zs), B))
        nits = np.broadcast_to(np.asarray(nit, dtype=np.int32), (B,))
        self = cls.__new__(cls)
        self.B = B
        Zarr, narr = _i32(Zs), _i32(nits)
        self._h = C.c_void_p()
        check(lib().mmw_batch_create_from_env(C.byref(self._h), env._h, _pi(Zarr), int(rank_radio), float(eta), _pi(narr)))
        self._created(env.device, nits)
        return self

    @classmethod
    def from_csr(cls, csrs, Zs, nit, eta, rank_radio=2):
        """The batch for states that lie on the device as CSR arrays, built there without a host copy of any of them
        (mmw_batch_create_from_csr): the object `BatchSolver(Zs, [c.state() for c in csrs], nit, eta, rank_radio)` gives, field for
        field.  csrs: `DeviceCSR`s, or `DeviceState`s whose owner is one, all on one device (the same one may appear more than once);
        all with device = -1 gives the host-only batch.  It keeps nothing of them: each may be closed at once."""
        owners = [csr_owner(c) for c in csrs]
        B = len(owners)
        if B < 1 or len(Zs) != B:
            raise MMWError("BatchSolver.from_csr: one slot count per state, at least one state")
        for i, c in enumerate(owners):
            if c is None or not c._h:
                raise MMWError("BatchSolver.from_csr: entry %d is not an open DeviceCSR (or a DeviceState of one)" % i)
        nits = np.broadcast_to(np.asarray(nit, dtype=np.int32), (B,))
        self = cls.__new__(cls)
        self.B = B
        Zarr, narr = _i32(Zs), _i32(nits)
        handles = (C.c_void_p * B)(*[c._h.value for c in owners])
        self._h = C.c_void_p()
        check(lib().mmw_batch_create_from_csr(C.byref(self._h), B, handles, _pi(Zarr), int(rank_radio), float(eta), _pi(narr)))
        self._created(owners[0].device, nits)
        return self

    def _created(self, device, nits):
        B = self.B
        self.device = int(device)
        self.nits = [int(x) for x in nits]
        self.active = [True] * B
        self._auto = {}  # per setter in _SPLITS: the arguments of its suggest function while "auto" holds
        self.split_parts = None  # workgroups per instance as last accepted by set_split (None: the single-launch kernel)
        self.row_split_parts = None  # row parts per instance as last accepted by set_row_split (None: no row split)
        self.head_split_parts = None  # head parts per instance as last accepted by set_head_split (None: the head on one workgroup)
        self.factor_split_parts = None  # the same for the factor, as last accepted by set_factor_split (None: k_batch_factor's one launch)
        self._load_sizes()

    def _load_sizes(self):
        self.sizes = []
        for b in range(self.B):
            sz = (C.c_int64 * 10)()
            check(lib().mmw_batch_sizes(self._h, b, sz))
            self.sizes.append(dict(zip(_SIZE_NAMES, [int(x) for x in sz])))

    def iterations_done(self, inst):
        sz = (C.c_int64 * 10)()
        check(lib().mmw_batch_sizes(self._h, int(inst), sz))
        return int(sz[9])

    def set_expm(self, max_order=16, tol=1e-9):
        check(lib().mmw_batch_set_expm(self._h, int(max_order), float(tol)))

    def set_eta(self, eta):
        """One step size for every instance, or one per instance."""
        e = _f64(np.broadcast_to(np.asarray(eta, dtype=np.float64), (self.B,)))
        check(lib().mmw_batch_set_eta(self._h, _pd(e)))

    def reset(self, nit):
        check(lib().mmw_batch_reset(self._h, int(nit)))
        self.nits = [int(nit)] * self.B
        self._load_sizes()

    def set_slots(self, Zs, nit, warm=False):
        """Per-instance slot counts (0: the instance sits out until a later call gives it one); every instance restarts.
        warm=True (mmw_batch_set_slots_warm): an instance that has iterated continues from its previous probe's iterate with its
        sums restarted and `nit` more iterations announced, one that has not restarts cold, and one that sits out keeps its
        iterate and its counters, so a later warm call picks it up."""
        z = _i32(Zs)
        if z.size != self.B:
            raise MMWError("set_slots: one slot count per instance")
        check((lib().mmw_batch_set_slots_warm if warm else lib().mmw_batch_set_slots)(self._h, _pi(z), int(nit)))
        self.nits = [self.nits[b] if warm and int(z[b]) <= 0 else int(nit) for b in range(self.B)]
        self.active = [int(x) > 0 for x in z]
        self._load_sizes()
        for who in self._SPLITS:  # "auto" follows the slot counts (in _SPLITS' order: the row parts follow the column slices)
            if who in self._auto:
                self._apply_parts(who, getattr(self, self._SPLITS[who][1])(*self._auto[who]))

    def carry_from(self, src, take=None):
        """mmw_batch_carry: take the iterate (e_accu, L, X, Y) of `src`, a batch of the same users on the states they were in before
        they moved, over into this batch, which has not iterated: L and X by (row, col), e_accu and Y by user and by association
        pair, 0 for what `src` does not hold; Y is not renormalised (the first iteration rewrites it).  take: one flag per instance
        (None: all).  An instance whose source never iterated stays cold.  `iterations_done` stays 0 and `nit` is unchanged, so
        `set_slots(..., warm=True)` still treats a carried instance that has not iterated as cold."""
        t = None if take is None else _i32([1 if x else 0 for x in take])
        if t is not None and t.size != self.B:
            raise MMWError("carry_from: one flag per instance")
        check(lib().mmw_batch_carry(self._h, src._h, _opt_pi(t)))

    def carry_map(self, src, inst):
        """mmw_batch_carry_map: (lmap int32[nnzL], cmap int32[C]) of instance `inst` -- for every entry of this batch's L pattern and
        of its constraint vector the position in `src`'s, -1 where `src` holds none.  Works on device=-1 batches."""
        sz = self.sizes[inst]
        lmap = np.empty(sz["nnzL"], dtype=np.int32)
        cmap = np.empty(sz["C"], dtype=np.int32)
        check(lib().mmw_batch_carry_map(self._h, src._h, int(inst), _pi(lmap), int(lmap.size), _pi(cmap), int(cmap.size)))
        return lmap, cmap

    def iterate(self, n, randv=None, seeds=None):
        """randv: None (device Philox, `seeds` one per instance) or a list with, per instance, the (n_b, K, D) sketches of the
        n_b = min(n, nit - done) iterations it runs (instances that run nothing: None or an empty array)."""
        n = int(n)
        if randv is None:
            if seeds is None:
                raise MMWError("iterate: give sketches or one seed per instance")
            check(lib().mmw_batch_iterate(self._h, n, None, _pu(_u64(seeds, self.B))))
        else:
            if len(randv) != self.B:
                raise MMWError("iterate: one block list per instance")
            parts = []
            for b, r in enumerate(randv):
                sz = self.sizes[b]
                nb = max(0, min(n, self.nits[b] - sz["iter"])) if self.active[b] else 0
                a = np.zeros(0) if r is None or nb == 0 else _f64(r).ravel()
                if a.size != nb * sz["K"] * sz["D"]:
                    raise MMWError("iterate: instance %d runs %d iterations and needs %d sketch values, got %d"
                                   % (b, nb, nb * sz["K"] * sz["D"], a.size))
                parts.append(a)
            flat = _f64(np.concatenate(parts)) if parts else np.zeros(0)
            check(lib().mmw_batch_iterate(self._h, n, _pd(flat), None))
        self._load_sizes()

    def sketch(self, inst, seed, iteration):
        sz = self.sizes[inst]
        out = np.empty((sz["K"], sz["D"]), dtype=np.float64)
        check(lib().mmw_batch_sketch(self._h, int(inst), C.c_uint64(int(seed)), int(iteration), _pd(out), int(out.size)))
        return out

    _LEN = _LEN

    def read(self, inst, which, n=None):
        sz = self.sizes[inst]
        if n is None:
            if which in (F_XHALF, F_SKETCH):
                n = sz["K"] * sz["D"]
            elif which == F_EXPM_INFO:
                n = 4
            elif which == BATCH_F_PATTERN:
                n = 2 * sz["nnzL"] + 4 * sz["K"]
            elif which == BATCH_F_BUILD_INFO:
                n = 2
            else:
                n = sz[self._LEN[which]]
        out = np.empty(int(n), dtype=np.float64)
        check(lib().mmw_batch_read_f64(self._h, int(inst), int(which), _pd(out), int(n)))
        if which in (F_XHALF, F_SKETCH):
            out = out.reshape(sz["K"], sz["D"])
        return out

    _ILEN = _ILEN

    def read_i32(self, inst, which):
        if which == I_PATTERN:
            sz = self.sizes[inst]
            n = 2 * sz["K"] + 1 + 3 * sz["nnzL"] + sz["E_asso"]
        else:
            name, off = self._ILEN[which]
            n = self.sizes[inst][name] + off
        out = np.empty(int(n), dtype=np.int32)
        check(lib().mmw_batch_read_i32(self._h, int(inst), int(which), _pi(out), int(n)))
        return out

    def set_gap(self, on=True, m_cap=0):
        """Log the duality gap (mmw.py:79-117) of every iteration that follows, inside the batch launch; m_cap <= 0: 600 steps."""
        check(lib().mmw_batch_set_gap(self._h, 1 if on else 0, int(m_cap)))

    def gap_log(self, inst):
        """(rows[iterations, 3], steps[iterations]): per iteration done {e_max, K lambda_min, their difference} -- the columns 3:6 of
        the reference's LOGGED_NP_DATA["gap"] -- and the Lanczos steps taken (negative: the cap was reached first).  Rows of
        iterations that ran with the gap off are NaN (steps 0)."""
        n = self.iterations_done(inst)
        out = np.empty((n, 4), dtype=np.float64)
        check(lib().mmw_batch_read_gap(self._h, int(inst), _pd(out), int(out.size)))
        st = out[:, 3]
        return out[:, :3].copy(), np.where(np.isnan(st), 0, st).astype(np.int64)

    # ---- several workgroups per instance (csrc/kernels_batch_split.h)
    @staticmethod
    def split_slices(D, parts):
        """(W, G): the column slices `parts` workgroups cut D sketch columns into -- G = ceil(D / W) slices of W = 8 ceil(ceil(D / parts) / 8)
        columns, the last one possibly narrower."""
        W = 8 * -(-(-(-int(D) // int(parts))) // 8)
        return W, -(-int(D) // W)

    def suggest_split(self, cus=256):
        """The rule of set_split("auto"): instance i weighs w_i = nnzL_i D_i (the work of one Taylor term) and gets
        parts_i = clamp(round(w_i cus / sum w), 1, min(32, ceil(D_i / 8))) workgroups -- its share of `cus` compute units, at most
        one per 8 sketch columns.  Instances that sit out get 1 and do not weigh."""
        w = [float(s["nnzL"]) * s["D"] if a else 0.0 for s, a in zip(self.sizes, self.active)]
        tot = sum(w)
        if tot <= 0.0:
            return [1] * self.B
        return [max(1, min(int(round(wi * cus / tot)), BATCH_MAX_PARTS, -(-s["D"] // 8))) for wi, s in zip(w, self.sizes)]

    # setter -> (C entry, suggest function, attribute holding the accepted parts)
    _SPLITS = {"set_split": ("mmw_batch_set_split", "suggest_split", "split_parts"),
               "set_row_split": ("mmw_batch_set_row_split", "suggest_row_split", "row_split_parts"),
               "set_head_split": ("mmw_batch_set_head_split", "suggest_head_split", "head_split_parts"),
               "set_factor_split": ("mmw_batch_set_factor_split", "suggest_factor_split", "factor_split_parts")}

    def _apply_parts(self, who, parts):
        entry, _, attr = self._SPLITS[who]
        p = _i32(np.broadcast_to(np.asarray(parts, dtype=np.int64), (self.B,)))
        check(getattr(lib(), entry)(self._h, _pi(p)))
        setattr(self, attr, [int(x) for x in p] if np.any(p > 1) else None)

    def _set_parts(self, who, parts, *suggest_args):
        """The protocol of both setters: an int for all, one per instance, "auto" (the suggest function, taken again after every
        `set_slots`), or None for the unsplit path."""
        entry, suggest, attr = self._SPLITS[who]
        if parts is None:
            check(getattr(lib(), entry)(self._h, None))
            setattr(self, attr, None)
            self._auto.pop(who, None)
        elif isinstance(parts, str):
            if parts != "auto":
                raise MMWError("%s: parts must be an int, one int per instance, \"auto\" or None" % who)
            self._apply_parts(who, getattr(self, suggest)(*suggest_args))
            self._auto[who] = suggest_args
        else:
            if np.ndim(parts) and len(parts) != self.B:
                raise MMWError("%s: one part count per instance" % who)
            self._apply_parts(who, parts)
            self._auto.pop(who, None)

    def set_split(self, parts, cus=256):
        """Workgroups per instance for the iterations that follow: an int for all, one per instance, "auto" (`suggest_split(cus)`,
        taken again after every `set_slots`), or None / all ones for the single-launch kernel.  Every field stays bitwise what the
        single launch gives; an instance gains when it is the straggler of its batch."""
        self._set_parts("set_split", parts, int(cus))

    # ---- the rows of a Taylor term over workgroups (csrc/kernels_batch_rows.h)
    @staticmethod
    def row_bounds(indptr, rows):
        """The rows + 1 boundaries the library cuts a pattern's K rows at: boundary p is the first row at which the prefix of `indptr`
        reaches p nnzL / rows (compared in integers), the last one is K.  Contiguous ranges that cover [0, K), balanced by stored
        entries: every range holds at most ceil(nnzL / rows) entries plus its last row's, and a range may be empty."""
        ip = [int(x) for x in indptr]
        K, rows = len(ip) - 1, int(rows)
        nnz, out, r = ip[K], [], 0
        for p in range(rows):
            while r < K and ip[r] * rows < p * nnz:
                r += 1
            out.append(r)
        return out + [K]

    def row_ranges(self, inst, rows):
        """The boundaries the library uses for instance `inst` at `rows` row parts (mmw_batch_row_ranges): part p owns the rows
        [out[p], out[p + 1]).  Answers on a host-only batch too."""
        out = np.empty(int(rows) + 1, dtype=np.int32)
        check(lib().mmw_batch_row_ranges(self._h, int(inst), int(rows), _pi(out)))
        return [int(x) for x in out]

    def suggest_row_split(self, cus=256):
        """The rule of set_row_split("auto"): with w_i = nnzL_i D_i (the work of one Taylor term) and G_i the instance's current
        column slices, rows_i = clamp(ceil(round(w_i cus / sum w) / G_i), 1, min(64, ceil(K_i / 64))): the instance's share of `cus`
        compute units, divided by the workgroups its column slices already give it, at least 64 rows per part.  The rule is a
        choice, not a measurement (DESIGN section 12 has what was measured).  Instances that sit out get 1 and do not weigh."""
        w = [float(s["nnzL"]) * s["D"] if a else 0.0 for s, a in zip(self.sizes, self.active)]
        tot = sum(w)
        if tot <= 0.0:
            return [1] * self.B
        cols = self.split_parts or [1] * self.B
        out = []
        for wi, s, cp in zip(w, self.sizes, cols):
            G = self.split_slices(s["D"], cp)[1]
            out.append(max(1, min(-(-int(round(wi * cus / tot)) // G), BATCH_MAX_ROW_PARTS, -(-s["K"] // 64))))
        return out

    def set_row_split(self, rows, cus=256):
        """Row parts per instance for the iterations that follow, multiplied with the column slices of `set_split`: an int for all,
        one per instance, "auto" (`suggest_row_split(cus)`, taken again after every `set_slots`), or None / all ones for no row split.
        One launch per Taylor term and one host synchronisation per iteration; every field stays bitwise what the single launch gives
        (DESIGN section 12)."""
        self._set_parts("set_row_split", rows, int(cus))

    def split_call(self):
        """The last `iterate` of this batch (MMW_F_SPLIT_CALL): {"path": 0 one launch / 1 the column split's three per iteration / 2 the
        row split's one per Taylor term, "launches", "idle" (launches in which every workgroup was past its schedule or had all its
        columns stopped; path 2 only), "widest" (workgroups of the largest launch)}."""
        v = self.read(0, F_SPLIT_CALL, 4)
        return {"path": int(v[0]), "launches": int(v[1]), "idle": int(v[2]), "widest": int(v[3])}

    # ---- the head and the plan over workgroups (csrc/kernels_batch_head.h)
    def head_ranges(self, inst, parts):
        """The row boundaries the library uses for instance `inst` at `parts` head parts (mmw_batch_head_ranges): the rule of
        `row_bounds`; part p owns the rows [out[p], out[p + 1]).  Answers on a host-only batch too."""
        out = np.empty(int(parts) + 1, dtype=np.int32)
        check(lib().mmw_batch_head_ranges(self._h, int(inst), int(parts), _pi(out)))
        return [int(x) for x in out]

    def suggest_head_split(self, cus=256):
        """The rule of set_head_split("auto"): the head's work is O(nnzL), so instance i gets its share of `cus` compute units by stored
        entries, parts_i = clamp(round(nnzL_i cus / sum nnzL), 1, min(64, ceil(K_i / 64))): at least 64 rows per part.  The rule is a
        choice, not a measurement (DESIGN section 12 has what was measured).  Instances that sit out get 1 and do not weigh."""
        w = [float(s["nnzL"]) if a else 0.0 for s, a in zip(self.sizes, self.active)]
        tot = sum(w)
        if tot <= 0.0:
            return [1] * self.B
        return [max(1, min(int(round(wi * cus / tot)), BATCH_MAX_HEAD_PARTS, -(-s["K"] // 64))) for wi, s in zip(w, self.sizes)]

    def set_head_split(self, parts, cus=256):
        """Row parts per instance for everything in front of the exponential (averaging, DUAL, LOSS, the plan's pass over L) and for the
        row sums of X behind it, in the iterations that follow: an int for all, one per instance, "auto" (`suggest_head_split(cus)`,
        taken again after every `set_slots`), or None / all ones for the head on one workgroup.  With it on an iteration runs through
        the split paths even when `set_split` and `set_row_split` are off; every field stays bitwise what the single launch gives
        (DESIGN section 12)."""
        self._set_parts("set_head_split", parts, int(cus))

    def head_call(self):
        """The last `iterate` of this batch (MMW_F_HEAD_CALL): {"on": the head split ran, "launches" (of the head path's own kernels),
        "widest" (workgroups of the largest of them)}."""
        v = self.read(0, F_HEAD_CALL, 4)
        return {"on": bool(v[0]), "launches": int(v[1]), "widest": int(v[2])}

    # ---- several workgroups per instance for the factor (csrc/kernels_batch_factor_split.h)
    @staticmethod
    def factor_items(K, parts):
        """[(first pair, count), ...]: the items `parts` workgroups cut the P = ceil((K + (K & 1)) / 2) row pairs of a tournament round
        into -- contiguous ranges of ceil(P / parts) pairs, G = ceil(P / that) <= parts of them, none empty."""
        K, parts = int(K), int(parts)
        P = (K + (K & 1)) // 2
        per = -(-P // parts)
        return [(p0, min(per, P - p0)) for p0 in range(0, P, per)]

    def suggest_factor_split(self):
        """The rule of set_factor_split("auto"): parts_i = clamp(ceil(P_i / 16), 1, 32) with P_i the row pairs of a round, so each of a
        workgroup's eight waves holds at most one two-pair step per round.  Instances that sit out get 1."""
        return [max(1, min(-(-((s["K"] + (s["K"] & 1)) // 2) // 16), BATCH_MAX_PARTS)) if a else 1 for s, a in zip(self.sizes, self.active)]

    def set_factor_split(self, parts):
        """Workgroups per instance and tournament round for the `factor` calls that follow: an int for all, one per instance, "auto"
        (`suggest_factor_split()`, taken again after every `set_slots`), or None / all ones for the one launch of k_batch_factor.  The
        factor, its record and every rounding stay bitwise what the single launch gives."""
        self._set_parts("set_factor_split", parts)

    def factor_call(self):
        """The last `factor` of this batch (MMW_F_FACTOR_CALL): {"path": 0 one launch / 1 one launch per round, "launches", "sweeps"
        (of the host loop; path 0: 0), "widest" (workgroups of the largest launch)}."""
        v = self.read(0, F_FACTOR_CALL, 4)
        return {"path": int(v[0]), "launches": int(v[1]), "sweeps": int(v[2]), "widest": int(v[3])}

    def export(self, inst, solver):
        """The instance's iterate into `solver` (an fp64 `Solver` of the same state and Z), which then factors / rounds it."""
        check(lib().mmw_batch_export(self._h, int(inst), solver._h))
        solver._timed = 0

    # ---- the epilogue inside the batch (csrc/kernels_batch_epilogue.h): one launch for all factors, one for all roundings
    def _take(self, take):
        if take is None:
            return None, [i for i in range(self.B) if self.active[i]]
        t = _i32([1 if x else 0 for x in take])
        if t.size != self.B:
            raise MMWError("take: one flag per instance")
        return t, [i for i in range(self.B) if t[i]]

    def factor(self, take=None, ranks=None, xavg=None):
        """X_half of every taking instance (take: one flag per instance, None = every active one) in one launch; it stays on the
        device for `round`, `read_factor(i)` copies it out.  ranks: one per instance (None: min(K-1, (Z-1) rank_radio)).  xavg: parity
        mode, a list with per instance None or its Xbar values on the pattern (F_XAVG's order) to factor instead of the run's."""
        t, _ = self._take(take)
        r = None if ranks is None else _i32(ranks)
        if r is not None and r.size != self.B:
            raise MMWError("factor: one rank per instance")
        xp, keep = None, []
        if xavg is not None:
            if len(xavg) != self.B:
                raise MMWError("factor: one entry per instance in xavg")
            xp = (C.POINTER(C.c_double) * self.B)()
            for i, x in enumerate(xavg):
                if x is None:
                    continue
                a = _f64(x).ravel()
                if a.size != self.sizes[i]["nnzL"]:
                    raise MMWError("factor: xavg of instance %d must hold nnzL = %d values" % (i, self.sizes[i]["nnzL"]))
                keep.append(a)
                xp[i] = _pd(a)
        check(lib().mmw_batch_factor(self._h, _opt_pi(t), _opt_pi(r), xp))

    def factor_info(self, inst):
        """{"sweeps", "max_cos" (largest |cos| of a row pair as met in the last sweep), "rank", "sigma_rank", "sigma_next"} of the last factor."""
        v = self.read(inst, F_FACTOR_INFO, 5)
        return {"sweeps": int(v[0]), "max_cos": float(v[1]), "rank": int(v[2]), "sigma_rank": float(v[3]), "sigma_next": float(v[4])}

    def factor_row_norms(self, inst):
        """After `factor_spectral`: every user's row norm of the eigenvector block before its rows were normalised (MMW_F_FACTOR_ROWNORM).
        The top eigenvectors are localised: users with a tiny norm here carry amplified rounding noise in `read_factor`."""
        return self.read(inst, F_FACTOR_ROWNORM, self.sizes[inst]["K"])

    def read_factor(self, inst):
        """X_half (K, rank) of the instance's last `factor`, columns in ascending singular value."""
        rank = self.factor_info(inst)["rank"]
        K = self.sizes[inst]["K"]
        return self.read(inst, F_FACTOR, K * rank).reshape(K, rank)

    def round(self, nattempt, seeds, take=None, stop_at_first=True, env=None):
        """sdp_solver.rounding of every taking instance's resident factor in one launch, attempt a of instance i drawn from
        (seeds[i], a).  Returns (z, rem, used): z[i] is None or int32 (nattempt, K) with -1 = unassigned and -2 = attempt not run,
        rem int32 (B, nattempt) with -1 = not run, used int32 (B,) attempts run.  env: see `round_env`."""
        t, who = self._take(take)
        nattempt = int(nattempt)
        sd = _u64(seeds, self.B)
        zflat = np.empty(max(1, nattempt * sum(self.sizes[i]["K"] for i in who)), dtype=np.int32)
        rem = np.empty((self.B, max(1, nattempt)), dtype=np.int32)
        used = np.empty(self.B, dtype=np.int32)
        args = (_opt_pi(t), nattempt, 1 if stop_at_first else 0, _pu(sd), _pi(zflat), _pi(rem), _pi(used))
        check(lib().mmw_batch_round(self._h, *args) if env is None else lib().mmw_batch_round_env(self._h, env._h, *args))
        z, o = [None] * self.B, 0
        for i in who:
            K = self.sizes[i]["K"]
            z[i] = zflat[o:o + nattempt * K].reshape(nattempt, K)
            o += nattempt * K
        return z, rem, used

    def factor_random(self, seeds, take=None):
        """rand_sdp_solver.run_with_state (sdp_solver.py:109-114) of every taking instance: its resident factor becomes the
        row-normalised K x D block of normals `sketch(i, seeds[i], 0)`, rank D; `round` / `round_env` / `read_factor` then work on it.
        All its rows have norm 1, so the rounding visits the users of such a block in index order (include/mmw_hip.h)."""
        t, _ = self._take(take)
        check(lib().mmw_batch_factor_random(self._h, _opt_pi(t), _pu(_u64(seeds, self.B))))

    def factor_spectral(self, Zs=None, take=None):
        """spectral_sdp_solver.run_with_state (sdp_solver.py:165-185) of every taking instance on the state the batch was built from:
        its resident factor becomes the K x Z block of the Laplacian's Z eigenvectors of largest eigenvalue (columns in ascending
        eigenvalue, signs arbitrary but deterministic), every row divided by its norm; a row that is exactly zero (an isolated user)
        stays zero.  Zs: one per instance (None: each instance's own slot count), 1 <= Z <= K.  `round` / `round_env` / `read_factor` /
        `factor_info` ({sweeps, max_cos, rank = Z, sigma_rank = lambda_Z, sigma_next = lambda_Z+1}) then work on it; the rounding visits
        the users in index order, as for `factor_random` (include/mmw_hip.h)."""
        t, _ = self._take(take)
        z = None if Zs is None else _i32(Zs)
        if z is not None and z.size != self.B:
            raise MMWError("factor_spectral: one Z per instance")
        check(lib().mmw_batch_factor_spectral(self._h, _opt_pi(t), _opt_pi(z)))

    def gm(self, kind, Zs, nattempt=1, take=None, keys=False):
        """gm.MAX_GAIN.run (kind 0) / gm.MAX_ASSO.run (kind 1) in the stable order for every taking instance's own state, one launch
        (mmw_batch_gm).  Zs: the slot bound, one for all or one per instance, <= 0 = not_Z_bound.  Returns (z, ZZ, rem[, keys]): z[i]
        None or int32 (K,) with -1 = left over, ZZ / rem int32 (B,) with -1 for instances left out, keys[i] the visiting key."""
        t, who = self._take(take)
        return _gm_call(lib().mmw_batch_gm, self._h, self.B, [s["K"] for s in self.sizes], who, kind, Zs, nattempt, t, keys)

    def gm_rand(self, Zs, seeds, nattempt=1, take=None, stop_at_first=True):
        """gm.MAX_RAND.run with its draws on the device for every taking instance's own state, one launch (mmw_batch_gm_rand):
        attempt a of instance i is `GreedyHandle.rand`'s draw of (seeds[i], a).  Zs: the slot count, one for all or one per
        instance; Z <= 0 leaves the instance out.  Returns (z, rem, used) in `round`'s shapes."""
        t, who = self._take(take)
        return _gm_rand_call(lib().mmw_batch_gm_rand, self._h, self.B, [s["K"] for s in self.sizes], who, Zs, seeds, nattempt, t, stop_at_first)

    def round_env(self, env, nattempt, seeds, take=None, stop_at_first=True):
        """`round` against the state a `BatchEnv` holds (the stations as they have moved) instead of the one the batch was built
        from: same factors, same draws, same greedy pass (mmw_batch_round_env).  Nothing of the batch changes."""
        return self.round(nattempt, seeds, take=take, stop_at_first=stop_at_first, env=env)

    def round_randv(self, inst, seed, attempt):
        """The (Z, rank) row-normalised projection vectors attempt `attempt` of `round` draws for the instance with `seed`, bitwise."""
        Z, rank = self.sizes[inst]["Z"], self.factor_info(inst)["rank"]
        out = np.empty((Z, rank), dtype=np.float64)
        check(lib().mmw_batch_round_randv(self._h, int(inst), C.c_uint64(int(seed)), int(attempt), _pd(out), int(out.size)))
        return out


class DeviceFactor(np.lib.mixins.NDArrayOperatorsMixin):
    """The X_half of `Solver.factor(resident=True)`: (K, rank) float64 that lives on the device.  The reference hands the factor from
    `run_with_state` straight to `rounding` (binary_search_relaxation.py:50-53): `Solver.round` recognises this object and reads the factor
    where it lies.  For everything else it is an array: `np.asarray`, arithmetic, indexing and attribute access copy it out (once)."""

    def __init__(self, solver, rank, serial, index_ordered=False):
        self._solver, self._serial, self._host = solver, serial, None
        self.index_ordered = index_ordered  # True: a block of unit rows already scaled for the index-order visit (Solver.factor_spectral)
        self.shape, self.ndim, self.dtype = (solver.K, rank), 2, np.dtype(np.float64)

    def on_device_of(self, solver):
        """True while `solver` is the handle that made this factor and has not made another one since."""
        return self._solver is solver and getattr(solver, "_factor_serial", 0) == self._serial and bool(solver._h.value)

    def __array__(self, dtype=None, copy=None):
        if self._host is None:
            if not self.on_device_of(self._solver):
                raise MMWError("this factor was not copied to the host before its handle computed another one (or was closed)")
            self._host = self._solver.read(F_FACTOR, self.shape[0] * self.shape[1]).reshape(self.shape)
        return self._host if dtype is None else self._host.astype(dtype, copy=False)

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        return getattr(ufunc, method)(*[np.asarray(x) if isinstance(x, DeviceFactor) else x for x in inputs], **kwargs)

    def __array_function__(self, func, types, args, kwargs):
        conv = lambda x: np.asarray(x) if isinstance(x, DeviceFactor) else x
        return func(*[conv(a) for a in args], **{k: conv(v) for k, v in kwargs.items()})

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, idx):
        return np.asarray(self)[idx]

    def __getattr__(self, name):  # (only reached for what the object itself lacks: T, sum, copy, ...)
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(np.asarray(self), name)


class DeviceEnv(_Handle):
    """Owning wrapper of one `mmw_env*`: the reference's problem generator and scorer on the device (env.py:136-233)."""
    _destroy = "mmw_env_destroy"

    def __init__(self, sta_locs, ap_locs, fre_Hz=4e9, txp_offset=2.0, min_s_n_ratio=0.1, min_sinr=1.0, noise_floor_dbm=-94.0, device=0):
        sta = _f64(sta_locs)
        ap = _f64(ap_locs)
        if sta.ndim != 2 or sta.shape[1] != 2 or ap.ndim != 2 or ap.shape[1] != 2:
            raise MMWError("station and AP locations must be (n, 2) arrays")
        self.K, self.A = int(sta.shape[0]), int(ap.shape[0])
        self._h = C.c_void_p()
        check(lib().mmw_env_create(C.byref(self._h), int(device), self.K, self.A, _pd(sta), _pd(ap), float(fre_Hz), float(txp_offset),
                                   float(min_s_n_ratio), float(min_sinr), float(noise_floor_dbm)))
        self.device = int(device)
        self.generation = 0  # counts the moves: a DeviceState belongs to the generation it was made in
        self._load_sizes()

    def _load_sizes(self):
        sz = (C.c_int64 * 4)()
        check(lib().mmw_env_sizes(self._h, sz))
        self.nnzS, self.nnzQ = int(sz[2]), int(sz[3])

    def move(self, sta_locs):
        """generate_S_Q_hmax at the stations' new positions sta_locs (K, 2), on the device (mmw_env_move): afterwards `state`, `bounds`
        and `evaluate` answer bitwise what a fresh DeviceEnv at those positions answers.  Handles built from this environment before
        are untouched; a `device_state()` handed out before belongs to the old generation and raises when it is used."""
        sta = _f64(sta_locs)
        if sta.shape != (self.K, 2):
            raise MMWError("move: station locations must be a (K, 2) array")
        self.generation += 1  # (first: after a move that failed nothing of an older generation may be read either)
        check(lib().mmw_env_move(self._h, _pd(sta)))
        self._load_sizes()

    def state(self):
        """(S_gain csr, Q_asso csr, h_max) as env.generate_S_Q_hmax returns them."""
        return _state_out(self.K, self.nnzS, self.nnzQ, lambda *a: check(lib().mmw_env_state(self._h, *a)))

    def bounds(self):
        """(lower, upper) slot-count bounds of binary_search_relaxation.py:13-29 for this state, from the device's count pass."""
        out = np.zeros(2, dtype=np.int32)
        check(lib().mmw_env_bounds(self._h, _pi(out)))
        return int(out[0]), int(out[1])

    def solver(self, Z, nit, eta, rank_radio=2, dtype=F64):
        return Solver.from_env(self, Z, nit, eta, rank_radio=rank_radio, dtype=dtype)

    def device_state(self):
        """The `state` to hand to the solver classes: behaves like the (S_gain, Q_asso, h_max) tuple (materialised on the host only if
        someone indexes it), and lets `mmw` / `binary_search_relaxation` stay on the device (Solver.from_env, bounds())."""
        return DeviceState(self)

    def evaluate(self, z, Z, packet_bit=800, bandwidth=5e6, slot_time=1.25e-4, bler=True):
        """(sinr, bler) per user under the colouring z (env.evaluate_sinr / evaluate_bler)."""
        zz = _f64(z)
        if zz.shape != (self.K,):
            raise MMWError("z must have one slot per user")
        sinr = np.empty(self.K, dtype=np.float64)
        bl = np.empty(self.K, dtype=np.float64) if bler else None
        check(lib().mmw_env_evaluate(self._h, _pd(zz), int(Z), float(packet_bit), float(bandwidth), float(slot_time), _pd(sinr),
                                     _pd(bl) if bler else None))
        return sinr, bl


class BatchEnv(_Handle):
    """Owning wrapper of one `mmw_batch_env*`: the generator and the scorer (env.py:136-233) for B small instances, one workgroup
    each (csrc/kernels_batch_env.h).  ap_locs: one (A, 2) array per instance; Ks: stations per instance.  `move` takes the
    stations' positions, one (K, 2) array per instance, and regenerates every state; until the first move nothing else answers."""
    _destroy = "mmw_batch_env_destroy"

    def __init__(self, ap_locs, Ks, fre_Hz=4e9, txp_offset=2.0, min_s_n_ratio=0.1, min_sinr=1.0, noise_floor_dbm=-94.0, device=0):
        aps = [_f64(a) for a in ap_locs]
        self.B = B = len(aps)
        if B < 1 or len(Ks) != B or any(a.ndim != 2 or a.shape[1] != 2 for a in aps):
            raise MMWError("BatchEnv: one (A, 2) array of AP locations and one station count per instance, at least one instance")
        self.Ks, self.As = [int(k) for k in Ks], [int(a.shape[0]) for a in aps]
        self.device = int(device)
        self._h = C.c_void_p()
        check(lib().mmw_batch_env_create(C.byref(self._h), int(device), B, _pi(_i32(self.Ks)), _pi(_i32(self.As)), self._ptrs(aps), float(fre_Hz),
                                         float(txp_offset), float(min_s_n_ratio), float(min_sinr), float(noise_floor_dbm)))

    def _ptrs(self, arrays):
        return (C.POINTER(C.c_double) * self.B)(*[_pd(a) for a in arrays])

    def move(self, sta_locs):
        """generate_S_Q_hmax of every instance at the positions sta_locs[i] (K_i, 2): two launches for all instances."""
        sta = [_f64(x) for x in sta_locs]
        if len(sta) != self.B or any(x.shape != (k, 2) for x, k in zip(sta, self.Ks)):
            raise MMWError("move: one (K, 2) array of station locations per instance")
        check(lib().mmw_batch_env_move(self._h, self._ptrs(sta)))

    def sizes(self, inst):
        sz = (C.c_int64 * 4)()
        check(lib().mmw_batch_env_sizes(self._h, int(inst), sz))
        return {"K": int(sz[0]), "A": int(sz[1]), "nnzS": int(sz[2]), "nnzQ": int(sz[3])}

    def state(self, inst):
        """(S_gain csr, Q_asso csr, h_max) of instance `inst` at its last positions, as env.generate_S_Q_hmax returns them."""
        sz = self.sizes(inst)
        return _state_out(sz["K"], sz["nnzS"], sz["nnzQ"], lambda *a: check(lib().mmw_batch_env_state(self._h, int(inst), *a)))

    def evaluate(self, zs, Zs, packet_bit=800, bandwidth=5e6, slot_time=1.25e-4, bler=True):
        """env.evaluate_sinr / evaluate_bler of one colouring per instance in one launch: zs[i] (K_i,) slot numbers, Zs[i] slots.
        Returns (sinr, bler): one array per instance each (bler None when not asked for)."""
        z = [_f64(x) for x in zs]
        if len(z) != self.B or len(Zs) != self.B or any(x.shape != (k,) for x, k in zip(z, self.Ks)):
            raise MMWError("evaluate: one colouring with one slot per user, and one slot count, per instance")
        sinr = [np.empty(k, dtype=np.float64) for k in self.Ks]
        bl = [np.empty(k, dtype=np.float64) for k in self.Ks] if bler else None
        check(lib().mmw_batch_env_evaluate(self._h, self._ptrs(z), _pi(_i32(Zs)), float(packet_bit), float(bandwidth), float(slot_time),
                                           self._ptrs(sinr), self._ptrs(bl) if bler else None))
        return sinr, bl

    def gm(self, kind, Zs, nattempt=1, take=None, keys=False):
        """`BatchSolver.gm` on the states of the last `move` (mmw_batch_env_gm); take: one flag per instance, None = all."""
        t = None if take is None else _i32([1 if x else 0 for x in take])
        if t is not None and t.size != self.B:
            raise MMWError("take: one flag per instance")
        who = [i for i in range(self.B) if t is None or t[i]]
        return _gm_call(lib().mmw_batch_env_gm, self._h, self.B, self.Ks, who, kind, Zs, nattempt, t, keys)

    def gm_rand(self, Zs, seeds, nattempt=1, take=None, stop_at_first=True):
        """`BatchSolver.gm_rand` on the states of the last `move` (mmw_batch_env_gm_rand); take: one flag per instance, None = all."""
        t = None if take is None else _i32([1 if x else 0 for x in take])
        if t is not None and t.size != self.B:
            raise MMWError("take: one flag per instance")
        who = [i for i in range(self.B) if t is None or t[i]]
        return _gm_rand_call(lib().mmw_batch_env_gm_rand, self._h, self.B, self.Ks, who, Zs, seeds, nattempt, t, stop_at_first)


_CSR_NAMES = ("S_indptr", "S_indices", "S_data", "Q_indptr", "Q_indices", "Q_data", "h_max")
_CSR_TYPES = ("int32", "int32", "float64", "int32", "int32", "float64", "float64")
_TYPESTR = {"<i4": "int32", "<i8": "int64", "<f8": "float64", "<f4": "float32"}


def _device_array(a, name, want, length):
    """(address, object to keep alive) of one of wrap's seven arrays: an int address (taken at its word: the lengths are the caller's),
    an object with data_ptr() / numel() (a torch tensor), or one with __cuda_array_interface__.  dtype and length are checked."""
    if isinstance(a, (int, np.integer)) or a is None:
        addr = int(a or 0)
        if addr == 0 and length:
            raise MMWError("DeviceCSR.wrap: %s is a null address but its length is %d" % (name, length))
        return addr, None
    if hasattr(a, "data_ptr") and hasattr(a, "numel"):
        dt, n, addr = str(a.dtype).split(".")[-1], int(a.numel()), int(a.data_ptr())
        if hasattr(a, "is_contiguous") and not a.is_contiguous():
            raise MMWError("DeviceCSR.wrap: %s must be contiguous" % name)
        if getattr(getattr(a, "device", None), "type", "cuda") == "cpu":
            raise MMWError("DeviceCSR.wrap: %s lies on the host (wrap borrows device arrays: use DeviceCSR.upload)" % name)
    elif hasattr(a, "__cuda_array_interface__"):
        d = a.__cuda_array_interface__
        if d.get("strides") is not None:
            raise MMWError("DeviceCSR.wrap: %s must be contiguous" % name)
        dt, n, addr = _TYPESTR.get(d["typestr"], d["typestr"]), int(np.prod(d["shape"], dtype=np.int64)), int(d["data"][0] or 0)
    else:
        raise MMWError("DeviceCSR.wrap: %s must be a device address, a tensor (data_ptr / numel) or a __cuda_array_interface__ object" % name)
    if dt != want:
        hint = " (convert the indices to int32 first: they are not converted silently)" if dt == "int64" else ""
        raise MMWError("DeviceCSR.wrap: %s is %s, must be %s%s" % (name, dt, want, hint))
    if n != length:
        raise MMWError("DeviceCSR.wrap: %s has %d elements, must have %d" % (name, n, length))
    return (addr if n else 0), a


class DeviceCSR(_Handle):
    """Owning wrapper of one `mmw_csr*`: a state on the device as its seven CSR arrays -- uploaded once (`upload`) or borrowed from
    whoever built the graph on the GPU (`wrap`, `from_torch`).  `Solver.from_csr` builds the handle from it on the device; `bounds()`
    gives the bisection's bounds from a device count pass; `device_state()` is the `state` the solver classes take."""
    _destroy = "mmw_csr_destroy"

    @classmethod
    def _new(cls, device):
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.device = int(device)
        self._keep = None
        return self

    def _created(self):
        sz = (C.c_int64 * 4)()
        check(lib().mmw_csr_sizes(self._h, sz))
        self.K, self.nnzS, self.nnzQ = int(sz[0]), int(sz[2]), int(sz[3])
        return self

    @classmethod
    def upload(cls, state, device=0):
        """Device copies of a host state (S_gain, Q_asso, h_max), owned by the library; device = -1 keeps host copies (CPU tests)."""
        K, arrs = _state_arrays(state)
        return cls.upload_arrays(K, arrs, device)

    @classmethod
    def upload_arrays(cls, K, arrays, device=0):
        """`upload` for the seven arrays as they are (int32 / float64, not canonicalised: what the validation is tested with)."""
        sp, si, sx, qp, qi, qx, hm = [np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, _CSR_TYPES)]
        if sp.size != K + 1 or qp.size != K + 1 or hm.size != K or si.size != sx.size or qi.size != qx.size:
            raise MMWError("DeviceCSR: indptr arrays of K + 1 entries, h_max of K, indices and data of one length each")
        self = cls._new(device)
        ptr = [C.c_void_p(a.ctypes.data if a.size else None) for a in (sp, si, sx, qp, qi, qx, hm)]
        check(lib().mmw_csr_upload(C.byref(self._h), self.device, int(K), int(si.size), int(qi.size), *ptr))
        return self._created()

    @classmethod
    def wrap(cls, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max, K, device=0, nnzS=None, nnzQ=None):
        """Borrow seven device arrays (see `_device_array` for what an array may be).  nnzS / nnzQ: needed when the arrays are plain
        addresses, else taken from S_indices / Q_indices.  The arrays must stay alive and unchanged while this object lives (objects are
        kept referenced here; addresses are the caller's to keep) and be complete when a call that reads them is made."""
        arrs = (S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max)
        K = int(K)

        def count(a, given, name):
            if given is not None:
                return int(given)
            if hasattr(a, "numel"):
                return int(a.numel())
            if hasattr(a, "__cuda_array_interface__"):
                return int(np.prod(a.__cuda_array_interface__["shape"], dtype=np.int64))
            raise MMWError("DeviceCSR.wrap: %s is needed when the arrays are given as addresses" % name)
        ns, nq = count(S_indices, nnzS, "nnzS"), count(Q_indices, nnzQ, "nnzQ")
        lengths = (K + 1, ns, ns, K + 1, nq, nq, K)
        got = [_device_array(a, n, t, m) for a, n, t, m in zip(arrs, _CSR_NAMES, _CSR_TYPES, lengths)]
        self = cls._new(device)
        self._keep = [g[1] for g in got]
        check(lib().mmw_csr_wrap(C.byref(self._h), self.device, K, ns, nq, *[C.c_void_p(g[0] or None) for g in got]))
        return self._created()

    @classmethod
    def from_torch(cls, S, Q, h_max):
        """Borrow a state that torch holds on the ROCm device: S, Q sparse-CSR tensors (float64 values), h_max dense float64.  The index
        arrays are converted to int32 on the device (torch keeps int64); torch's current stream is synchronised, so the arrays are
        complete; the tensors stay referenced by this object.  (A torch build that ships its own HIP runtime has to touch the device
        before this library makes its first HIP call in the process -- bench.py's order -- or torch finds no device.)"""
        import torch  # (only here: the product imports without torch)
        if S.layout != torch.sparse_csr or Q.layout != torch.sparse_csr:
            raise MMWError("DeviceCSR.from_torch: S and Q must be sparse-CSR tensors")
        if not S.is_cuda or not Q.is_cuda or not h_max.is_cuda:
            raise MMWError("DeviceCSR.from_torch: the tensors must lie on the ROCm device")
        K = int(S.shape[0])
        parts = []
        for m in (S, Q):
            parts += [m.crow_indices().to(torch.int32).contiguous(), m.col_indices().to(torch.int32).contiguous(), m.values().to(torch.float64).contiguous()]
        parts.append(h_max.to(torch.float64).contiguous())
        torch.cuda.current_stream(S.device).synchronize()
        return cls.wrap(*parts, K=K, device=S.device.index or 0)

    def _closing(self):
        self._keep = None

    def state(self):
        """(S_gain csr, Q_asso csr, h_max): the host copy, made on request."""
        return _state_out(self.K, self.nnzS, self.nnzQ, lambda *a: check(lib().mmw_csr_state(self._h, *a)))

    def bounds(self):
        """(lower, upper) slot-count bounds of binary_search_relaxation.py:13-29 for this state, from a count pass on the device."""
        out = np.zeros(2, dtype=np.int32)
        check(lib().mmw_csr_bounds(self._h, _pi(out)))
        return int(out[0]), int(out[1])

    def pointers(self):
        """The seven device addresses in `wrap`'s order (0 for an empty array)."""
        out = (C.c_void_p * 7)()
        check(lib().mmw_csr_pointers(self._h, out))
        return [int(p or 0) for p in out]

    def solver(self, Z, nit, eta, rank_radio=2, dtype=F64):
        return Solver.from_csr(self, Z, nit, eta, rank_radio=rank_radio, dtype=dtype)

    def device_state(self):
        """The `state` to hand to the solver classes (see DeviceEnv.device_state): handles by Solver.from_csr, bounds from bounds()."""
        return DeviceState(self)


class DeviceState:
    """`state` of a DeviceEnv or a DeviceCSR (anything with K, state(), bounds() and solver(Z, nit, eta, rank_radio, dtype)): a lazy
    (S_gain, Q_asso, h_max) triple that remembers where it lives."""

    def __init__(self, env):
        self._env = env
        self.K = env.K
        self._host = None
        self.generation = getattr(env, "generation", 0)  # (a DeviceCSR never changes: one generation)

    def check(self):
        """A device-resident state is immutable -- identity is content (sdp_solver._same_state).  A DeviceEnv that has moved since
        holds another state under the same object: this one then refuses every use instead of reading the new arrays."""
        now = getattr(self._env, "generation", 0)
        if now != self.generation:
            raise MMWError("this DeviceState belongs to generation %d of its environment, which has moved since (generation %d): "
                           "take a new one from device_state()" % (self.generation, now))

    @property
    def env(self):
        """Where the state lives (its `solver` and `bounds` routes): checked on every access."""
        self.check()
        return self._env

    def host(self):
        if self._host is None:
            self._host = self.env.state()
        else:
            self.check()
        return self._host

    def __getitem__(self, i):
        return self.host()[i]

    def __iter__(self):
        return iter(self.host())

    def __len__(self):
        return 3


def csr_owner(state):
    """The `DeviceCSR` behind `state` -- a DeviceCSR itself or a DeviceState of one -- else None (host triples, a DeviceState of a
    DeviceEnv): what `BatchSolver.from_csr` takes and the batch workflows route by."""
    if isinstance(state, DeviceCSR):
        return state
    if isinstance(state, DeviceState) and isinstance(state._env, DeviceCSR):
        return state.env
    return None


class GreedyHandle(_Handle):
    """Owning wrapper of one `mmw_gm*`: the state of the greedy baselines of gm.py (mmw_gm_create), device = -1 for host C++."""
    _destroy = "mmw_gm_destroy"

    def __init__(self, state, device=0):
        self.K, (sp, si, sx, qp, qi, qx, hm) = _state_arrays(state)
        self.device = int(device)
        self._h = C.c_void_p()
        check(lib().mmw_gm_create(C.byref(self._h), self.device, self.K, _pi(sp), _pi(si), _pd(sx), _pi(qp), _pi(qi), _pd(qx), _pd(hm)))
        sz = (C.c_int64 * 4)()
        check(lib().mmw_gm_sizes(self._h, sz))
        self.groups = int(sz[1])  # -1: Q is not a union of cliques (general association check)

    @classmethod
    def from_env(cls, env):
        """The handle for the state a DeviceEnv holds now, its lists built on the device and its clique groups taken from the
        generator's association (mmw_gm_create_from_env): answers exactly what `GreedyHandle(env.state())` answers, and keeps
        answering for that state when the environment moves on."""
        self = cls.__new__(cls)
        self.K, self.device = env.K, env.device
        self._h = C.c_void_p()
        check(lib().mmw_gm_create_from_env(C.byref(self._h), env._h))
        self.groups = self.sizes()[1]
        return self

    def sizes(self):
        """mmw_gm_sizes: [K, clique groups (-1: general check), nnz of the S rows, nnz(Q)]."""
        sz = (C.c_int64 * 4)()
        check(lib().mmw_gm_sizes(self._h, sz))
        return [int(x) for x in sz]

    def key(self, kind):
        """MAX_GAIN's (kind 0) or MAX_ASSO's (kind 1) visiting key of the handle's state, float64 [K], bitwise the reference's
        scipy expression (mmw_gm_key); a handle built from an environment forms it on the device."""
        out = np.empty(self.K, dtype=np.float64)
        check(lib().mmw_gm_key(self._h, int(kind), _pd(out)))
        return out

    def pass_(self, order, nattempt=1):
        """One slot for the visiting order `order` (unassigned users): the accepted users, in acceptance order."""
        o = _i32(order)
        out = np.empty(max(o.size, 1), dtype=np.int32)
        n = C.c_int32(0)
        check(lib().mmw_gm_pass(self._h, _pi(o), int(o.size), int(nattempt), _pi(out), C.byref(n)))
        return out[:n.value]

    def run(self, key, Z, nattempt=1):
        """All slots under the stable order of -key: (slot int32[K] with -1 = unassigned, ZZ, remainder)."""
        k = _f64(key)
        if k.shape != (self.K,):
            raise MMWError("key must hold one value per user")
        z = np.empty(self.K, dtype=np.int32)
        zz, rem = C.c_int32(0), C.c_int32(0)
        check(lib().mmw_gm_run(self._h, _pd(k), int(Z), int(nattempt), _pi(z), C.byref(zz), C.byref(rem)))
        return z, zz.value, rem.value

    def assign(self, order, pref):
        """User-major greedy: order[K], pref (K, Z) slot preference per user; returns (slot int32[K] with -1, remainder)."""
        o = _i32(order)
        p = _i32(pref)
        if o.shape != (self.K,) or p.ndim != 2 or p.shape[0] != self.K:
            raise MMWError("assign: order must be (K,) and pref (K, Z)")
        z = np.empty(self.K, dtype=np.int32)
        rem = C.c_int32(0)
        check(lib().mmw_gm_assign(self._h, int(p.shape[1]), _pi(o), _pi(p), _pi(z), C.byref(rem)))
        return z, rem.value

    def rand(self, Z, nattempt=1, seed=0, pick="first"):
        """MAX_RAND with its draws made where the state lies (mmw_gm_rand): attempts 0 ... nattempt - 1 of the draw of `seed`
        (include/mmw_hip.h states it), one picked on the device.  pick: "first" (the first attempt that leaves nobody over, else the
        last) or "fewest" (the fewest users left over).  Returns (slot int32[K] with -1 = left over, rem int32[nattempt], picked)."""
        if pick not in ("first", "fewest"):
            raise ValueError("pick must be 'first' or 'fewest', got %r" % (pick,))
        z = np.empty(self.K, dtype=np.int32)
        rem = np.empty(max(1, int(nattempt)), dtype=np.int32)
        got = C.c_int32(0)
        check(lib().mmw_gm_rand(self._h, int(Z), int(nattempt), int(seed), 0 if pick == "first" else 1, _pi(z), _pi(rem), C.byref(got)))
        return z, rem, got.value

    def rand_draw(self, Z, seed, attempt):
        """The draw of one attempt copied out (mmw_gm_rand_draw): (pref_val float64 (K, Z), order_key float64 (K,))."""
        pv = np.empty((self.K, max(0, int(Z))), dtype=np.float64)
        key = np.empty(self.K, dtype=np.float64)
        check(lib().mmw_gm_rand_draw(self._h, int(Z), int(seed), int(attempt), _pd(pv), _pd(key)))
        return pv, key


def sym_eig(G, rel_tol=1e-13, max_sweeps=30, device=0):
    """Eigen-decomposition of a symmetric matrix by the device's block Jacobi; returns (theta unsorted, Q, block sweeps)."""
    G = _f64(G)
    b = G.shape[0]
    if G.shape != (b, b):
        raise ValueError("sym_eig: square matrix expected")
    theta = np.empty(b, dtype=np.float64)
    Q = np.empty((b, b), dtype=np.float64)
    sw = C.c_int32(0)
    check(lib().mmw_sym_eig(int(device), b, _pd(G), float(rel_tol), int(max_sweeps), _pd(theta), _pd(Q), C.byref(sw)))
    return theta, Q, sw.value


def dense_gram(V, W, b, sym, dtype=F64, device=0):
    """V[:, :b]^T W[:, :b] by the factor's Gram kernels (mmw_dense_gram); V, W are K x ld blocks, `sym` symmetrises."""
    V, W = _f64(V), _f64(W)
    if V.ndim != 2 or V.shape != W.shape:
        raise ValueError("dense_gram: two K x ld blocks expected")
    K, ld = V.shape
    G = np.empty((max(int(b), 0), max(int(b), 0)), dtype=np.float64)
    check(lib().mmw_dense_gram(int(device), int(dtype), K, int(b), ld, _pd(V), _pd(W), int(bool(sym)), _pd(G)))
    return G


def dense_gemm(V, Q, b, n, dtype=F64, device=0):
    """V[:, :b] Q[:b, :n] by the factor's tall GEMM (mmw_dense_gemm), as a K x ld block whose other columns are zero."""
    V, Q = _f64(V), _f64(Q)
    if V.ndim != 2 or Q.ndim != 2 or Q.shape[0] != b:
        raise ValueError("dense_gemm: a K x ld block and a b x ldq matrix expected")
    K, ld = V.shape
    out = np.empty((K, ld), dtype=np.float64)
    check(lib().mmw_dense_gemm(int(device), int(dtype), K, int(b), int(n), ld, _pd(V), Q.shape[1], _pd(Q), _pd(out)))
    return out


def dense_chol(G, device=0):
    """The Cholesky-QR's factorisation of a Gram matrix (mmw_dense_chol): (L of the unit-diagonal-scaled matrix, dscale, the
    inverses of L's 32 x 32 diagonal blocks [ceil(b / 32), 32, 32], ok)."""
    G = _f64(G)
    b = G.shape[0]
    if G.shape != (b, b):
        raise ValueError("dense_chol: square matrix expected")
    L = np.empty((b, b), dtype=np.float64)
    dscale = np.empty(b, dtype=np.float64)
    dinv = np.empty(((b + 31) // 32, 32, 32), dtype=np.float64)
    ok = C.c_int32(0)
    check(lib().mmw_dense_chol(int(device), b, _pd(G), _pd(L), _pd(dscale), _pd(dinv), C.byref(ok)))
    return L, dscale, dinv, bool(ok.value)


def dense_orth(V, b, dtype=F64, eps=1e-14, device=0):
    """The factor's orthonormalisation of a K x ld block (mmw_dense_orth): (Q as a K x ld block, [what pass 1 did, what pass 2
    did] with 0 Cholesky-QR, 1 Newton-Schulz, 2 eigen fallback)."""
    V = _f64(V)
    if V.ndim != 2:
        raise ValueError("dense_orth: a K x ld block expected")
    K, ld = V.shape
    out = np.empty((K, ld), dtype=np.float64)
    path = (C.c_int32 * 2)()
    check(lib().mmw_dense_orth(int(device), int(dtype), K, int(b), ld, _pd(V), float(eps), _pd(out), path))
    return out, [int(path[0]), int(path[1])]


def expm_apply(A_csr, B, dtype=F64, method=EXPM_LANCZOS, max_order=12, tol=1e-9, device=0, reps=1):
    """exp(A) B on the device for a symmetric scipy CSR matrix A; returns (out, info dict)."""
    ip, ci, vv = canonical_csr(A_csr)
    B = _f64(B)
    K, D = B.shape
    out = np.empty((K, D), dtype=np.float64)
    info = np.zeros(4, dtype=np.float64)
    us = C.c_double(0.0)
    check(lib().mmw_expm_apply(int(device), int(dtype), int(method), int(max_order), float(tol), K, D, _pi(ip), _pi(ci), _pd(vv),
                               _pd(B), _pd(out), _pd(info), int(reps), C.byref(us)))
    return out, {"one_norm": info[0], "order": int(info[1]), "substeps": int(info[2]), "shift": info[3], "kernel_us": us.value}
