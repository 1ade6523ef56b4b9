// The library's MMW_* environment switches: one table, one lifetime.
//
// A switch is read ONCE, when its handle is created (mmw_create / mmw_create_from_env, before the blocking thread starts), or at the
// entry of a handle-less call (mmw_expm_apply, mmw_sym_eig, mmw_dense_*); the Switches value travels down by const reference and nothing re-reads
// the environment afterwards.  The exceptions are the developer aids of `LiveSwitch` below, which act on a handle that already
// exists and are read at the call.  No other file of csrc/ touches the environment.  (INTEGRATION.md documents every name.)
#pragma once
#include <cmath>
#include <cstdlib>

namespace mmw {

struct Switches {
    // ---- the exponential's products (expm_engine.h)
    bool no_slice_spmm = false;    // MMW_NO_SLICE_SPMM: the generic SpMM never takes its small-K form (k_spmm_slice)
    int mf_gt = 0;                 // MMW_MF_GT=4|8|12: column tiles per workgroup of the matrix-core SpMM (0: by the grid's size)
    bool no_apost = false;         // MMW_NO_APOST: Lanczos runs to its a-priori order (no a-posteriori stop)
    // ---- the blockings (blocking.h, the handle's setup)
    bool no_blocking = false;      // MMW_BLOCKING=0: generic gather kernels only
    bool full_tile = false;        // MMW_FULL_TILE: the full-tile LDS kernels instead of the half-tile ones
    bool no_mfma = false;          // MMW_NO_MFMA: no matrix-core blocking (strictly fp32 operands)
    bool no_mfma_sddmm = false;    // MMW_NO_MFMA_SDDMM: X on the pattern stays on the LDS-staged SDDMM
    int mf_rows = 64;              // MMW_MF_ROWS: rows per block of the matrix-core blocking
    int mf_union_cap = 0;          // MMW_MF_UNION_CAP: cap on a matrix-core block's union (0: MF_UNION)
    bool env_rcm = false;          // MMW_ENV_RCM: a handle made from the generator takes the pattern-only row order of the CSR entry point
    bool check_blocking = false;   // MMW_CHECK_BLOCKING: a host-only handle builds the blockings and checks their invariants (CPU tests)
    // ---- the epilogue factor (factor.h)
    bool chol_lds = false;         // MMW_CHOL_LDS: the Cholesky panel's diagonal block factored through LDS
    bool bj_full = false;          // MMW_BJ_FULL: every meeting of the block Jacobi solves the whole 64 x 64 problem
    bool factor_no_ns = false;     // MMW_FACTOR_NO_NS: the second orthonormalisation pass is a Cholesky-QR too
    bool factor_no_mfma = false;   // MMW_FACTOR_NO_MFMA: the Chebyshev filter stays on the fp32 SpMM
    bool factor_full_rr = false;   // MMW_FACTOR_FULL_RR: a Rayleigh-Ritz step after every filter pass
    // ---- the loop (solver.h, solver_loop.h, chunk_policy.h)
    bool no_fused_dual = false;    // MMW_NO_FUSED_DUAL: the softmax in its two passes in every iteration
    double dual_gap = NAN;         // MMW_DUAL_GAP: how far e_accu's maximum may run ahead of the fused pass's shift (NaN: 60 / 600 by dtype)
    bool no_lagged_plan = false;   // MMW_NO_LAGGED_PLAN: an exact plan in front of every exponential
    bool no_first_order = false;   // MMW_NO_FIRST_ORDER: never the exponential as one first-order product
    bool no_first_a16 = false;     // MMW_NO_FIRST_A16: ... never with the matrix as one fp16 half
    double fv_du_scale = 1.0;      // MMW_FV_DU_SCALE: inflates the measured rounding of the fp16 plane (tests: a forced miss)
    bool fv_worstcase = false;     // MMW_FV_WORSTCASE: the certificate takes the format's worst-case rounding instead of the measured one
    bool fv_in_sddmm = true;       // MMW_FV_IN_SDDMM=0: the certificate's workgroups ride in the next DUAL pass instead of the SDDMM
    bool no_sddmm_rowsums = false; // MMW_NO_SDDMM_ROWSUMS: k_dual_rows takes the row sums of X in every iteration
    bool cautious_replay = true;   // MMW_CAUTIOUS_REPLAY=0: a discarded chunk is replayed synchronously at once
    bool sync_plan = false;        // MMW_SYNC_PLAN: every plan is read back (no chunks without readback)
    bool no_chunk_chain = false;   // MMW_NO_CHUNK_CHAIN: every chunk restarts its plan and softmax exactly
    bool fused_sketch = false;     // MMW_FUSED_SKETCH: the next sketch is drawn by extra workgroups of the half-tile SDDMM
    bool no_loss_sketch = false;   // MMW_NO_LOSS_SKETCH: the sketch is drawn by a launch of its own instead of the LOSS pass
    bool keep_xhalf = false;       // MMW_KEEP_XHALF: every iteration of a chunk leaves the fp32 copy of exp(L/2)R
    int sk_slabs = 256;            // MMW_SK_SLABS: cap on the sketch kernel's slabs
    bool kt_markers = false;       // MMW_KT_MARKERS: set_profile(2) brackets the matrix-core product with events of its own

    static Switches from_env() {
        Switches s;
        auto on = [](const char* name) { return getenv(name) != nullptr; };
        auto is0 = [](const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; };
        auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        auto real = [](const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; };
        s.no_slice_spmm = on("MMW_NO_SLICE_SPMM");
        s.mf_gt = num("MMW_MF_GT", 0);
        s.no_apost = on("MMW_NO_APOST");
        if (const char* e = getenv("MMW_BLOCKING")) s.no_blocking = e[0] == '0';
        s.full_tile = on("MMW_FULL_TILE");
        s.no_mfma = on("MMW_NO_MFMA");
        s.no_mfma_sddmm = on("MMW_NO_MFMA_SDDMM");
        s.mf_rows = num("MMW_MF_ROWS", 64);
        s.mf_union_cap = num("MMW_MF_UNION_CAP", 0);
        s.env_rcm = on("MMW_ENV_RCM");
        s.check_blocking = on("MMW_CHECK_BLOCKING");
        s.chol_lds = on("MMW_CHOL_LDS");
        s.bj_full = on("MMW_BJ_FULL");
        s.factor_no_ns = on("MMW_FACTOR_NO_NS");
        s.factor_no_mfma = on("MMW_FACTOR_NO_MFMA");
        s.factor_full_rr = on("MMW_FACTOR_FULL_RR");
        s.no_fused_dual = on("MMW_NO_FUSED_DUAL");
        s.dual_gap = real("MMW_DUAL_GAP", NAN);
        s.no_lagged_plan = on("MMW_NO_LAGGED_PLAN");
        s.no_first_order = on("MMW_NO_FIRST_ORDER");
        s.no_first_a16 = on("MMW_NO_FIRST_A16");
        s.fv_du_scale = real("MMW_FV_DU_SCALE", 1.0);
        s.fv_worstcase = on("MMW_FV_WORSTCASE");
        s.fv_in_sddmm = !is0("MMW_FV_IN_SDDMM");
        s.no_sddmm_rowsums = on("MMW_NO_SDDMM_ROWSUMS");
        s.cautious_replay = !is0("MMW_CAUTIOUS_REPLAY");
        s.sync_plan = on("MMW_SYNC_PLAN");
        s.no_chunk_chain = on("MMW_NO_CHUNK_CHAIN");
        s.fused_sketch = on("MMW_FUSED_SKETCH");
        s.no_loss_sketch = on("MMW_NO_LOSS_SKETCH");
        s.keep_xhalf = on("MMW_KEEP_XHALF");
        s.sk_slabs = num("MMW_SK_SLABS", 256);
        s.kt_markers = on("MMW_KT_MARKERS");
        return s;
    }
};

// Developer aids and reports that act on a handle that already exists (tests and bench.py set them around a call on a live
// handle): read at the call, through live_switch() only.
enum LiveSwitch {
    LIVE_VERBOSE,             // MMW_VERBOSE: creation, plan and replay reports on stderr
    LIVE_FACTOR_VERBOSE,      // MMW_FACTOR_VERBOSE: the factor's timeline on stderr
    LIVE_STAMPS,              // MMW_STAMPS: mmw_bench_spmm dumps the blocked kernel's phase stamps
    LIVE_SD_STAMPS,           // MMW_SD_STAMPS: ... the last iteration's SDDMM launch of a call
    LIVE_DUAL_STAMPS,         // MMW_DUAL_STAMPS: ... the last iteration's fused DUAL launch of a call
    LIVE_HOST_BLOCKING,       // MMW_HOST_BLOCKING: a host-only handle builds the blockings and prints their statistics
    LIVE_HOST_BLOCKING_HIST,  // MMW_HOST_BLOCKING_HIST: ... and the k-steps of every matrix-core block
    LIVE_BENCH_LANCZOS,       // MMW_BENCH_LANCZOS: mmw_bench_spmm times the Lanczos epilogue instead of the plain product
    LIVE_BENCH_FIRST,         // MMW_BENCH_FIRST: ... the first-order product as the loop launches it
    LIVE_DEVBUF_EXACT,        // MMW_DEVBUF_EXACT: process-wide (DevBuf has no handle): every DevBuf::alloc is an allocation of its own
};
inline bool live_switch(LiveSwitch w) {
    static const char* const name[] = {"MMW_VERBOSE",       "MMW_FACTOR_VERBOSE",     "MMW_STAMPS",        "MMW_SD_STAMPS",   "MMW_DUAL_STAMPS",
                                       "MMW_HOST_BLOCKING", "MMW_HOST_BLOCKING_HIST", "MMW_BENCH_LANCZOS", "MMW_BENCH_FIRST", "MMW_DEVBUF_EXACT"};
    return getenv(name[w]) != nullptr;
}

}  // namespace mmw
