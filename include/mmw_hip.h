/*
 * mmw_hip.h -- C ABI of the MI355X (gfx950) MMW SDP hot path.
 *
 * The reference (zhouyou-gu/sig-sdp-mmw) is pure Python and has no FFI; its boundary for this path
 * is the duck-typed solver protocol
 *
 *     f, gX          = alg.run_with_state(it, Z, state)   sim_src/alg/binary_search_relaxation.py:50
 *     z_vec, Z, rem  = alg.rounding(Z, gX, state)         sim_src/alg/binary_search_relaxation.py:53
 *
 * implemented by class mmw (sim_src/alg/mmw.py:12-229) and sdp_solver.rounding
 * (sim_src/alg/sdp_solver.py:18-107).  The entry points below are what a ctypes binding of that class
 * calls (see INTEGRATION.md for the stub); each one cites the reference lines it replaces.
 *
 * Conventions: C linkage, plain pointers + sizes, no exceptions cross the ABI.  Every function returns
 * 0 on success or a negative status; mmw_last_error() gives the message of the calling thread's last
 * failure.  Host buffers are caller-owned (NumPy arrays); device memory is library-owned.  One handle =
 * one device + one HIP stream.  A handle is not thread-safe; different handles may be used
 * concurrently (the library keeps no mutable global state besides the thread-local error string).
 * All host-side floating point crosses the ABI as float64 whatever the device compute type is.
 */
#ifndef MMW_HIP_H
#define MMW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmw_solver mmw_solver;

#define MMW_OK 0
#define MMW_ERR_ARG (-1)     /* bad argument / malformed state */
#define MMW_ERR_HIP (-2)     /* a HIP runtime call failed (no device, OOM, launch failure) */
#define MMW_ERR_STATE (-3)   /* call out of order (e.g. iterate past nit) */

enum mmw_dtype { MMW_F32 = 0, MMW_F64 = 1 };
enum mmw_expm_method {
    MMW_EXPM_LANCZOS = 0, /* per-column Lanczos, exp of the small tridiagonals on device */
    MMW_EXPM_TAYLOR = 1   /* shifted truncated Taylor (the scheme scipy's expm_multiply runs) */
};

/* selectors for mmw_read_f64 / mmw_read_i32 */
enum mmw_field {
    MMW_F_Y = 0,          /* [C]      dual weights Y (mmw.py:139)                       */
    MMW_F_E_ACCU = 1,     /* [C]      accumulated violations e_accu (mmw.py:137)        */
    MMW_F_E_THIS = 2,     /* [C]      last e_this (mmw.py:136)                          */
    MMW_F_LVAL = 3,       /* [nnzL]   L_accu on the fixed pattern (mmw.py:167)          */
    MMW_F_XVAL = 4,       /* [nnzL]   X on the pattern, diagonal included (mmw.py:183-194) */
    MMW_F_XAVG = 5,       /* [nnzL]   running sum of X (mmw.py:77), not yet divided     */
    MMW_F_YAVG = 6,       /* [C]      running sum of Y (mmw.py:78)                      */
    MMW_F_XHALF = 7,      /* [K*D]    last exp(L/2) R, row-major (mmw.py:180)           */
    MMW_F_SKETCH = 8,     /* [K*D]    last row-normalised sketch R (mmw.py:226-227)     */
    MMW_F_S_SUM = 9,      /* [K]      S_sum  (mmw.py:34)                                */
    MMW_F_NORM_H = 10,    /* [K]      norm_H (mmw.py:39)                                */
    MMW_F_ST_DATA = 11,   /* [nnzST]  values of S_T' in CSR order (mmw.py:28-33)        */
    MMW_F_PHASE_US = 12,  /* [4*iters] per-iteration device us: dual, loss, expm, total (mmw.py:141,169,196,199) */
    MMW_F_EXPM_INFO = 13, /* [4]      last plan: one-norm bound, Krylov order m, substeps, shift mu */
    MMW_F_FACTOR = 14,    /* [K*rank] last factor of the averaged X (mmw.py:213-216)    */
    MMW_F_BLOCKING = 16,  /* [4]      locality blocking: in use (0/1), row blocks, nnz per staged row (reuse); [3] = batches replayed
                             because the device-side Krylov order outgrew the launched stages */
    MMW_F_SPMM_KIND = 17, /* [2]      SpMM kernel of exp(L/2)R on this handle: 0 generic CSR gather, 1 LDS-staged full tiles, 2 half tiles,
                             3 matrix-core (bf16 hi/lo split); [1] = 1 while the last plan allowed the matrix-core kernel */
    MMW_F_E_MAX = 18,     /* [1]      max_c e_c(X) of the last iteration (the largest entry of MMW_F_E_THIS, reduced on the device) */
    MMW_F_DUAL_INFO = 19, /* [4]      iterations since mmw_create {whose DUAL phase took the row sums of X from the matrix-core SDDMM instead of a
                             pass of its own, whose softmax ran inside the violation pass, whose exponential was ONE first-order product,
                             ... with the matrix in one fp16 half} */
    MMW_F_FACTOR_INFO = 20, /* [5]    mmw_batch_factor's record of an instance: {Jacobi sweeps, largest |cos| of a row pair as met in the last sweep (<= 1e-15 when it ended without a rotation),
                             rank, sigma_rank, sigma_rank+1 (0 if rank = K)}; batches only */
    MMW_F_FACTOR_CALL = 21, /* [4]    the last mmw_batch_factor of a batch, kept on the host, the same for every instance: {path: 0 = one launch
                             (k_batch_factor), 1 = one launch per round (mmw_batch_set_factor_split); kernel launches enqueued; sweeps
                             the host loop ran (path 0: 0); workgroups of the largest launch}; zeros before the first call; batches only */
    MMW_F_SPLIT_CALL = 22,  /* [4]    the last mmw_batch_iterate of a batch, kept on the host, the same for every instance: {path: 0 = one launch
                             (k_mmw_batch), 1 = three launches per iteration (mmw_batch_set_split), 2 = one launch per Taylor term
                             (mmw_batch_set_row_split); kernel launches enqueued; of which idle: every workgroup past its instance's
                             schedule or with all its columns stopped (path 2 only); workgroups of the largest launch}; zeros before
                             the first call; batches only */
    MMW_F_FACTOR_ROWNORM = 23, /* [K] after mmw_batch_factor_spectral: every user's row norm of the K x Z eigenvector block BEFORE its rows
                             were normalised (0: the row is exactly zero and stayed so).  The top eigenvectors are localised: a user with
                             a tiny norm here has a row of amplified rounding noise in MMW_F_FACTOR.  MMW_ERR_STATE on any other factor.
                             A solver handle answers it the same way after mmw_factor_spectral (MMW_ERR_STATE after mmw_factor) */
    MMW_F_HEAD_CALL = 24,   /* [4]    the last mmw_batch_iterate of a batch, kept on the host, the same for every instance: {on: 1 while the
                             head split ran (mmw_batch_set_head_split), else 0; launches of the head path's own kernels (k_batch_head_*)
                             enqueued; workgroups of the widest of them; 0}; zeros before the first call and with the head split off;
                             batches only */
    MMW_F_PATTERN = 25,     /* [2*nnzL + 4*K] the pattern part of an instance's fp64 arena as the batch kernels read it: S_T'[row,col] and
                             S_T'[col,row] on the L pattern, h_max, S_sum, 1 / norm_H, cH; batches only, MMW_ERR_STATE on a host-only one */
    MMW_F_BUILD_INFO = 26,  /* [2]    live, per instance: {how the batch was built: 0 from host arrays (mmw_batch_create), 1 on the
                             device (mmw_batch_create_from_env, mmw_batch_create_from_csr); 1 while the instance's host lists are complete, 0 while a batch built on
                             the device has not fetched them yet}; batches only */
    MMW_F_LAPLACIAN = 27,   /* [nnzL] the Laplacian of S_gain + S_gain^T (diagonal zeroed; sdp_solver.py:173-176) on the L pattern, fp64:
                             -(S[r,c] + S[c,r]) off the diagonal (0 where the pattern holds the entry through Q alone), the sum of
                             S[r,c] + S[c,r] over the row's off-diagonal entries in ascending column order on it.  Built on the first
                             call that asks; a device -1 handle answers it too; solver handles only */
    MMW_F_SPECTRAL_INFO = 28, /* [8]  the last mmw_factor_spectral: {outer rounds completed before the Rayleigh-Ritz step that ended it, last
                             relative residual, Z, block width b, theta_Z, theta_Z+1 (0 when b = Z), filter passes that ran on the matrix
                             cores, 0}; zeros before the first call; solver handles only */
    MMW_F_SPECTRAL_EIG = 29,  /* [Z]  the Ritz values the last mmw_factor_spectral kept, ascending (the block's column order) */
    MMW_F_GAP_INFO = 30,  /* [6]      mmw_set_gap's record since mmw_create: {rows logged, rows continued at a settle, rows enqueued through the
                             cap (no slot of the ring was free, or no guess at hand: such a row is never continued), launches of the phase, largest |steps|, bytes of the phase's work space};
                             solver handles only */
    MMW_F_KERNEL_US = 15  /* [2*9]    per kernel class {total device us, launches} since mmw_set_profile(1):
                             spmm, sddmm, dual, loss, krylov vector ops, sketch, projection, greedy, factor */
};
enum mmw_ifield {
    MMW_I_L_INDPTR = 0,   /* [K+1]   */
    MMW_I_L_INDICES = 1,  /* [nnzL]  */
    MMW_I_ST_INDPTR = 2,  /* [K+1]   */
    MMW_I_ST_INDICES = 3, /* [nnzST] */
    MMW_I_GAIN_X = 4,     /* [E_gain] nz_idx_gain_x_ut (mmw.py:56) */
    MMW_I_GAIN_Y = 5,
    MMW_I_ASSO_X = 6,     /* [E_asso] nz_idx_asso_x_ut (mmw.py:57) */
    MMW_I_ASSO_Y = 7,
    MMW_I_DIAG_POS = 8,   /* [K] position of (k,k) in the L pattern */
    MMW_I_ASSO_POS = 9,   /* [E_asso] position of (x,y), x<y, in the L pattern */
    MMW_I_PATTERN = 10,   /* [2*K + 1 + 3*nnzL + E_asso] an instance's slice of the int32 arena as the batch kernels read it: indptr,
                             columns, rows, pair ids (-1: none), diagonal positions, pair positions; batches only, MMW_ERR_STATE on a
                             host-only one */
    MMW_I_ROUND_LIST_BUILDS = 11 /* [1] solver handles: how often mmw_round_env / mmw_round_env_attempts built the handle's second list set
                             (once per (environment, generation) they met in turn); 0 on a handle that never called them */
};

const char* mmw_last_error(void);
int mmw_version(void);
/* number of visible HIP devices; does not create a context */
int mmw_device_count(int* n);

/*
 * mmw_create: mmw._process_state + the prologue of mmw._run (mmw.py:26-41, 46-74).
 * Takes `state` exactly as the reference's caller hands it over: S_gain and Q_asso as canonical CSR
 * (sorted indices, no duplicates; int32 index arrays as scipy stores them), h_max[K].  Builds S_T',
 * S_sum, norm_H, the edge lists and the fixed CSR pattern of L/X in native host code, copies them to
 * `device` once and sets the iterate to the reference's initial point (Y = 1/C, X = I, L = 0).
 * The inputs are not modified (the reference copies them too, mmw.py:28).
 * device == -1 builds the host-side pattern only (no HIP call): such a handle answers mmw_sizes,
 * mmw_read_i32 and the host fields S_SUM / NORM_H / ST_DATA, everything else returns MMW_ERR_STATE.
 */
int mmw_create(mmw_solver** out, int device, int dtype, int32_t K, int32_t Z, int32_t rank_radio, double eta,
               int32_t nit, const int32_t* S_indptr, const int32_t* S_indices, const double* S_data,
               const int32_t* Q_indptr, const int32_t* Q_indices, const double* Q_data, const double* h_max);
int mmw_destroy(mmw_solver* s);

/* out[0..9] = K, Z, D, Dpad, nnzL, nnzST, E_gain, E_asso, C, iterations done */
int mmw_sizes(mmw_solver* s, int64_t out[10]);

/* Krylov scheme for exp(L/2)R, max order per substep (<= 16) and target relative accuracy. */
int mmw_set_expm(mmw_solver* s, int method, int max_order, double tol);
/* 1: record HIP events around every phase of every iteration (fills MMW_F_PHASE_US, the reference's per-iteration timers
 * mmw.py:142,170,197,200); 0: none, iterations run back to back; S > 1: events only in iteration 0 and in one iteration of every S
 * (four event records per iteration are four barrier packets in the chain of dependent launches): MMW_F_PHASE_US still has one row per
 * iteration, the rows of a group of S iterations repeat the group's sample -- the harness takes means (sim_mmw_time.py:48-52). */
int mmw_set_timing(mmw_solver* s, int enabled);

/* 1: bracket every kernel class with HIP events on the solver's stream (fills MMW_F_KERNEL_US), plans read back every iteration and
 * every class in launches of its own, so launch counts are exact; 2: the same brackets around the launches of the shipped path as they
 * are (chunks without readback, the sketch and the lagged plan riding in the LOSS launch); 0: off.  Clears the sums. */
int mmw_set_profile(mmw_solver* s, int enabled);

/* micro-benchmark of the dominant kernel on the handle's pattern and current L values: `reps` launches of the
 * CSR SpMM (blocked = 1: LDS-staged locality-blocked kernel, 0: generic gather kernel); mean device us per launch */
int mmw_bench_spmm(mmw_solver* s, int blocked, int reps, double* avg_us);

/* back to the initial point of mmw.py:62-73 for a fresh run of `nit` iterations on the same (state, Z) */
int mmw_reset(mmw_solver* s, int32_t nit);

/*
 * mmw_set_slots: rebind the handle to another slot count Z on the SAME state (the binary search probes
 * several Z per state, binary_search_relaxation.py:46-50): norm_H and the D = Z*rank_radio wide blocks are
 * rebuilt, the pattern, its locality blocking and the device copies of the state are reused; then mmw_reset(nit).
 * Z < 2, or a width D past what the kernels cover (1024 columns on an fp32 handle, 512 on an fp64 one), is refused with
 * MMW_ERR_ARG before anything changes: the handle stays on its slot count, with its iterate.
 */
int mmw_set_slots(mmw_solver* s, int32_t Z, int32_t nit);
/*
 * mmw_set_slots_warm: the same rebinding, but the next run CONTINUES from the previous probe's iterate instead of the
 * reference's initial point (opt-in warm start of the binary search, binary_search_relaxation.py:44-72 calls the solver
 * once per probed Z and the reference restarts each time, mmw.py:62-68): e_accu, L_accu and the last X / Y are kept, the
 * running sums of X and Y restart from them.  Falls back to mmw_set_slots when the handle has not iterated yet.
 */
int mmw_set_slots_warm(mmw_solver* s, int32_t Z, int32_t nit);
/*
 * mmw_carry: the warm start ACROSS states on the handle side (the stations have moved; a re-solve per time point of the online sweeps at
 * any K).  `src` is a handle that has iterated on the old state, `dst` a handle on the new state -- from mmw_create, mmw_create_from_env
 * or mmw_create_from_csr -- that has run no iteration.  The rule is mmw_batch_carry's: L and X entry (row, col) of `dst` take `src`'s
 * value at (row, col) where `src`'s pattern stores it, else 0; e_accu and Y [D-part K | F-part E_asso | H-part K] carry by user and, the
 * F-part, by pair (asso_x, asso_y), 0 for a pair `src` lacks -- also where `src` stores the pair's entry as a gain entry.  Y is not
 * renormalised.  The running sums follow the handle's warm convention, as mmw_set_slots_warm leaves them: xavg = xval, yavg = Y.
 * e_this, the K x D blocks, the iteration count 0 and nit stay as creation left them.  No index map is made on the host: the two
 * patterns are matched on the device.  `dst` also takes over the run history mmw_set_slots_warm would have kept on `src` (its first
 * chunk is short and planned on `src`'s last plan).  `src` is only read: it is settled and its stream waited for.  Ordering: the call
 * returns after the work on `dst`'s stream has finished, so `src` may be iterated, reset or destroyed as soon as it is back.
 * A `src` that has run no iteration leaves `dst` cold (MMW_OK).  Refused before anything is written: dst == src (MMW_ERR_ARG), a handle
 * made with device -1 (MMW_ERR_STATE), different devices, dtypes or K (MMW_ERR_ARG), a `dst` that has iterated (MMW_ERR_STATE).  Z and
 * rank_radio may differ.
 * mmw_carry_map: the two maps that rule defines, computed on the host by merging the two patterns -- lmap[nl = nnzL of dst] the position
 * in `src`'s L / X arrays, cmap[nc = C of dst] the position in `src`'s constraint vector, -1 where `src` holds none.  Needs no device:
 * handles made with device -1 answer, handles built on the device fetch their lists first.  What the tests hold the device matching to.
 */
int mmw_carry(mmw_solver* dst, mmw_solver* src);
int mmw_carry_map(mmw_solver* dst, mmw_solver* src, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc);
/* step size for the iterations that follow (the reference reads self.eta on every run, mmw.py:137,167) */
int mmw_set_eta(mmw_solver* s, double eta);

/*
 * mmw_iterate: `n` passes of the loop body mmw.py:75-200 (averaging, DUAL, LOSS, EXPM), device resident.
 * randv: NULL -> the sketch of every iteration is generated on the device (Philox4x32-10 normals, key = the seed's
 * low and high word, counter = (row, column group, iteration, tag): see mmw_sketch; rows normalised); otherwise n*K*D float64, iteration-major,
 * each block the row-normalised (K,D) sketch the reference would draw at mmw.py:226-227 (parity mode).
 * Returns after the work is enqueued; any read or mmw_sync waits for it.
 */
int mmw_iterate(mmw_solver* s, int32_t n, const double* randv, uint64_t seed);
int mmw_sync(mmw_solver* s);
/*
 * mmw_sketch: the row-normalised (K, D) sketch the device generator draws for `iteration` of a run with `seed` (what
 * np.random.randn + the row normalisation of mmw.py:226-227 are to the reference).  The generator is counter-based: Philox4x32-10
 * with key (seed & 0xffffffff, seed >> 32) and counter (row, column group, iteration, 0x4d4d5753); a group is the 16 bytes one draw
 * fills -- columns 2p, 2p+1 from a 53-bit / 64-bit uniform pair on an fp64 handle, columns 4p ... 4p+3 from four 24-bit uniforms on an
 * fp32 one (Box-Muller) -- columns >= D are zero and do not count in the row's norm (DESIGN.md section 2 states the whole contract,
 * tests/helpers/philox_ref.py restates it in NumPy).  So the block is exactly the one mmw_iterate(n, NULL, seed) multiplied in that
 * iteration, in whatever chunk and whichever launch it was drawn: parity tests hand it to the oracle to follow a device-RNG run.
 * out: K*D float64, row-major.  Waits for enqueued work; does not touch the iterate.
 */
int mmw_sketch(mmw_solver* s, uint64_t seed, int32_t iteration, double* out, int64_t n);

int mmw_read_f64(mmw_solver* s, int which, double* out, int64_t n);
int mmw_read_i32(mmw_solver* s, int which, int32_t* out, int64_t n);

/*
 * mmw_gap: the LOG_GAP branch mmw.py:79-117 at the current averages (call before iteration i with
 * i+1 terms accumulated): out = { max_c e_c(Xbar), K*lambda_min(L(Ybar)), difference }.
 */
int mmw_gap(mmw_solver* s, double out[3]);

/*
 * The duality gap inside the loop of a solver handle, at any K: the LOG_GAP branch mmw.py:79-117 as launches of the handle's own
 * stream between the iterations (csrc/kernels_gap.h), so a logged run stays on the chunked path mmw_iterate(n) takes without it.
 *
 * mmw_set_gap: from the next mmw_iterate on, iteration i logs one row when it starts, from the i + 1 terms of the running sums
 * (Xbar = (xavg + the X still waiting for its LOSS pass) / (i + 1), Ybar = yavg / (i + 1); mmw.py:77-81): {e_max by the DUAL
 * formulas, K * theta with theta = lambda_min(L(Ybar)), e_max - K * theta, steps} -- LOGGED_NP_DATA["gap"][:, 3:6] of the reference
 * and the Lanczos steps taken -- by mmw_batch_set_gap's definitions: L(Ybar) by the LOSS formulas with coefficient +1, plain Lanczos
 * from the Philox start vector keyed by (row, K, nnzL), theta_min(T_m) and the last eigenvector component solved at the checks
 * mmw_gap_checks lists, stop at |beta_m s_m| <= 1e-11 * scale, on beta_m <= 1e-11 * scale, or at m = min(K, m_cap); `steps` is
 * NEGATIVE when the cap cut a Krylov space short.  m_cap <= 0 takes 600, m_cap > 1024 is MMW_ERR_ARG.  The phase works in float64 on
 * both dtypes (an fp32 handle's sums are widened as they are read, the pattern's constants are the host's doubles; an fp32 handle
 * built on the device holds its gains as floats only and widens those) and only reads the iterate: with the same sequence of calls every
 * field, counter and plan of the handle is bitwise what it is with the gap off, and the chunk lengths are the same.  A row is a
 * function of the sums it reads and of m_cap only: not of first_steps, of the split of the iterations into calls, or of where a chunk
 * ended.  first_steps: how far a row is enqueued while no earlier row of the run has been read back (<= 0: the cap); later rows go
 * through the first check at or after the largest |steps| read back so far.  Rows are read back where the loop synchronises anyway;
 * one that is not done by then is continued from its slot of a ring (at most 33 slots under a byte limit, MMW_F_GAP_INFO).  A
 * discarded chunk's rows are rewritten by its replay.  Rows of iterations that ran with the gap off are NaN (steps 0); mmw_reset,
 * mmw_set_slots and mmw_set_slots_warm clear the log and keep the setting; mmw_carry leaves the destination's log alone; mmw_gap is
 * unchanged.  MMW_ERR_STATE on a device -1 handle.
 * mmw_read_gap: 4 doubles per iteration done (n must be 4 x that count, else MMW_ERR_ARG); MMW_ERR_STATE if the gap was never
 * enabled.
 * mmw_gap_checks: the steps at which a row of (K, m_cap) is checked -- 10, 20, ... with the interval growing by a quarter, the last
 * at min(K, m_cap): for K >= 600 and the default cap 10 20 30 40 50 62 77 96 120 150 187 233 291 363 453 566 600.  *n gets their
 * count; `out` (room entries, or NULL to ask for the count) gets them.  A host function: no device is needed.
 */
int mmw_set_gap(mmw_solver* s, int enabled, int32_t m_cap, int32_t first_steps);
int mmw_read_gap(mmw_solver* s, double* out, int64_t n);
int mmw_gap_checks(int32_t K, int32_t m_cap, int32_t* out, int32_t room, int32_t* n);

/*
 * mmw_factor: the epilogue mmw.py:202-216.  Xbar = (sum of X)/nit on the pattern, top-`rank`
 * (by |eigenvalue|) invariant subspace by block Krylov iteration on the device,
 * X_half[K,rank] = V sqrt(|lambda|), columns in ascending |lambda| like svds.  out: K*rank float64, or NULL: the factor stays on
 * the device (mmw_round takes it from there with gX == NULL; mmw_read_f64(MMW_F_FACTOR) copies it out when asked) -- the caller
 * binary_search_relaxation.py:50-53 only hands it from run_with_state to rounding.
 */
int mmw_factor(mmw_solver* s, int32_t rank, double* out, uint64_t seed);

/*
 * mmw_factor_spectral: sdp_solver.spectral_sdp_solver.run_with_state (sdp_solver.py:165-185) on a handle, any K.  The Z eigenvectors
 * of largest eigenvalue of the Laplacian of S_gain + S_gain^T (MMW_F_LAPLACIAN) by mmw_factor's own iteration -- the Laplacian is
 * positive semidefinite, so largest |lambda| is largest lambda -- as a K x Z block, columns in ascending eigenvalue like eigsh
 * (signs arbitrary), every row divided by its norm; a row whose norm is exactly 0 (an isolated user) stays 0 where the reference
 * divides by zero.  index_order = 1: row k is then multiplied by 1 - k 2^-32 (rand_sdp_solver.index_ordered, bit for bit), so that the
 * rounding visits the unit rows in index order.  out: K*Z float64, or NULL: the block stays on the device for mmw_round(gX == NULL)
 * and MMW_F_FACTOR, as after mmw_factor.  MMW_F_FACTOR_ROWNORM hands out the norms before the division, MMW_F_SPECTRAL_INFO and
 * MMW_F_SPECTRAL_EIG the call's record.  Stops at mmw_factor's tolerance (relative residual 1e-9 in fp64, 2e-5 in fp32; the
 * reference asks eigsh for 1e-5); MMW_ERR_STATE when the iteration does not converge.  The handle's slot count, its iterate and its
 * sums play no part and do not move.  Z outside [1, K] or index_order outside {0, 1}: MMW_ERR_ARG before anything else; a device -1
 * handle: MMW_ERR_STATE.
 */
int mmw_factor_spectral(mmw_solver* s, int32_t Z, int32_t index_order, double* out, uint64_t seed);

#define MMW_FACTOR_RANDOM_MAX_COLS 2147483583 /* 2^31 - 1 - 64: the widest block mmw_factor_random draws (see there) */
/*
 * mmw_factor_random: rand_sdp_solver.run_with_state (sim_src/alg/sdp_solver.py:109-114) on a handle, any K: a K x cols block of
 * standard normals with its rows normalised, as the handle's RESIDENT FACTOR -- what mmw_batch_factor_random is for a batch.  The
 * block is float64 whatever the handle's dtype and lies where mmw_factor and mmw_factor_spectral leave theirs: mmw_round,
 * mmw_round_env, mmw_round_attempts and mmw_round_env_attempts take it with gX == NULL and Dp = cols, MMW_F_FACTOR copies it out.
 * out: K*cols float64, or NULL: the block stays on the device.
 * The draw is the sketch's: row r, column pair p (columns 2p and 2p + 1) from Philox4x32-10 with counter (r, p, 0, 0x4d4d5753) under
 * the key (seed & 0xffffffff, seed >> 32), Box-Muller in float64; a column >= cols does not count towards the norm; lane l of the
 * row's wavefront adds the squares of the pairs l + 64 i in ascending i and the 64 sums meet in the sketch's wave reduction.  So the
 * block is the float64 sketch of (seed, iteration 0): for cols <= 512 bitwise what mmw_sketch(seed, 0) returns on a float64 handle
 * whose D is cols, and bitwise what mmw_batch_factor_random leaves for seeds[b] = seed; wider blocks continue the same rule (i = 4,
 * 5, ...).  A float32 and a float64 handle give the same bits.
 * index_order = 1: row k is then multiplied by 1 - k 2^-32 (rand_sdp_solver.index_ordered of the index_order = 0 block, bit for bit),
 * so that the rounding visits the unit rows in index order, as for mmw_factor_spectral.
 * Nothing else moves: the iterate, its sums, a chunk in flight, the run history and MMW_F_EXPM_INFO stay as they are (the draw queues
 * behind the chunk; no iteration needs to have run), and a held mmw_factor / mmw_factor_spectral result is replaced as those replace
 * each other.  MMW_F_FACTOR_ROWNORM answers MMW_ERR_STATE afterwards.
 * Refused before anything is written, each with a message that names the value: cols < 1, index_order outside {0, 1}, cols >
 * MMW_FACTOR_RANDOM_MAX_COLS (MMW_ERR_ARG; mmw_round itself asks nothing of D' but D' >= 1 -- this is the widest D' for which the 64-column slab
 * counter of its projection, an int, does not wrap); a device -1 handle (MMW_ERR_STATE); a block of K x cols doubles that does not fit
 * on the device (MMW_ERR_HIP; the last factor stands).
 */
int mmw_factor_random(mmw_solver* s, int32_t cols, int32_t index_order, double* out, uint64_t seed);

/*
 * mmw_expm_apply: the stand-alone seam mmw.expm_half_randsk (mmw.py:224-229) minus the draw:
 * out[K,D] = exp(A) B for a symmetric CSR matrix A (pattern arbitrary) and a dense block B.
 * info (may be NULL): one-norm bound, order m, substeps, shift.  `reps` > 1 repeats the device work
 * (benchmarking); kernel_us (may be NULL) receives the mean device time of one application.
 */
int mmw_expm_apply(int device, int dtype, int method, int max_order, double tol, int32_t K, int32_t D,
                   const int32_t* indptr, const int32_t* indices, const double* data, const double* B,
                   double* out, double info[4], int32_t reps, double* kernel_us);

/*
 * mmw_sym_eig: the dense symmetric eigensolve inside mmw_factor's Rayleigh-Ritz step, stand-alone (the reference gets it from
 * LAPACK inside scipy.sparse.linalg.eigsh / svds, mmw.py:206-212): G = Q diag(theta) Q^T for a symmetric b x b matrix (row-major
 * float64) by block Jacobi on the device.  Stops when the off-diagonal Frobenius norm is below rel_tol * max|diag| * sqrt(b)
 * or after max_sweeps block sweeps (*sweeps, may be NULL, receives the count).  theta is not sorted.
 */
int mmw_sym_eig(int device, int32_t b, const double* G, double rel_tol, int32_t max_sweeps, double* theta, double* Q, int32_t* sweeps);

/*
 * The factor's dense building blocks, each as the one operation it is (csrc/kernels_dense.h through DenseWork / Factorizer of
 * csrc/factor.h), handle-less like mmw_sym_eig.  Blocks are K x ld row-major float64 host arrays, ld >= b their row stride; dtype
 * (MMW_F32 / MMW_F64) is the type T the block is stored in on the device -- the call rounds to T on the host before the upload and
 * widens what it reads back.  The caller fills the padding columns [b, ld) of an input; they influence no result.  MMW_CHOL_LDS and
 * MMW_FACTOR_NO_NS are read at the call.  MMW_ERR_ARG before the device is touched: a null pointer, K < 1, b < 1, b > 2048,
 * ld < b, n < 1, ldq < n, n > ld, an unknown dtype.
 *
 * mmw_dense_gram: G_out[b x b] = V[:, :b]^T W[:, :b] (k_gram_tiles + k_gram_reduce), sym != 0: (G + G^T) / 2.
 * mmw_dense_gemm: C_out[K x ld], columns < n = V[:, :b] Q[:b, :n] (k_gemm_tall; Q float64 with row stride ldq), the other columns 0.
 * mmw_dense_chol: the Cholesky-QR's factorisation of a b x b Gram matrix G: dscale_out[b] = 1 / sqrt(diag G) (0 where the diagonal
 *   is not positive), L_out[b x b] the lower-triangular factor of G' = diag(dscale) G diag(dscale) with zeros above the diagonal,
 *   dinv_out[ceil(b / 32)][32 x 32] the inverses of L's 32 x 32 diagonal blocks (identity-padded in the last one), *ok = 0 when a
 *   pivot was not positive (L_out and dinv_out then hold no result).
 * mmw_dense_orth: Q_out[K x ld] = Factorizer::orthonormalise of V (two passes; eps is the eigen fallback's relative floor, 1e-14 in
 *   the factor); path_out[pass] = 0 Cholesky-QR, 1 Newton-Schulz step, 2 eigen fallback.  Columns [b, ld) of Q_out are 0.
 */
int mmw_dense_gram(int device, int dtype, int32_t K, int32_t b, int32_t ld, const double* V, const double* W, int sym, double* G_out);
int mmw_dense_gemm(int device, int dtype, int32_t K, int32_t b, int32_t n, int32_t ld, const double* V, int32_t ldq, const double* Q, double* C_out);
int mmw_dense_chol(int device, int32_t b, const double* G, double* L_out, double* dscale_out, double* dinv_out, int32_t* ok);
int mmw_dense_orth(int device, int dtype, int32_t K, int32_t b, int32_t ld, const double* V, double eps, double* Q_out, int32_t path_out[2]);

/*
 * mmw_round: one sdp_solver.rounding_one_attempt (sdp_solver.py:27-107) per projection batch entry.
 * gX[K,Dp] and randv[nbatch,Z,Dp] (row-normalised, sdp_solver.py:48-49) in float64.  For every batch
 * entry: inprod = randv gX^T on the fp64 matrix cores, per-user slot preference order, the greedy
 * feasibility assignment in descending ||gX_k|| order.  z_out[nbatch,K] gets the slot or -1 for a user
 * left unassigned (the caller draws those, sdp_solver.py:104-105); rem_out[nbatch] the count.
 * gX == NULL: the K x Dp factor mmw_factor (or the block mmw_factor_spectral or mmw_factor_random) computed last on this handle, read where it lies on the device.
 * Ties: equal norms are visited by lower user index, equal inner products prefer the lower slot.  Zr > 4800 (32 Zr bytes
 * of flags beyond the greedy kernel's LDS) is refused with MMW_ERR_ARG before anything is allocated, copied, launched or timed.
 */
int mmw_round(mmw_solver* s, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv,
              int32_t* z_out, int32_t* rem_out);

/*
 * The producer and the consumer either side of the path, on the device.
 *
 * mmw_env_create: env._compute_txp / _compute_state / generate_S_Q_hmax (sim_src/env/env.py:136-196) for K stations at
 * sta_xy[K][2] and A access points at ap_xy[A][2] (the caller draws the station drop, env.py:59): path loss
 * 20 log10(f/1e6) - 12 + 28 log10(d + 1) dB, transmit power so that the strongest AP receives txp_offset * min_sinr over the
 * noise floor, receive powers below min_s_n_ratio dropped, association = strongest AP; S_gain = rx[:, asso] without explicit
 * zeros, Q_asso = same-AP relation without diagonal, h_max = diag(S_gain) / min_sinr - 1, all as CSR built on the device.
 * mmw_env_sizes: out = {K, A, nnz(S_gain), nnz(Q_asso)}; mmw_env_state copies the CSR arrays (caller-sized from mmw_env_sizes)
 * and h_max[K] to the host -- exactly the `state` mmw_create takes.
 * mmw_env_evaluate: env.evaluate_sinr / evaluate_bler (env.py:198-233) for the colouring z_vec[K] (float64 slot numbers as
 * rounding returns them) with Z slots: sinr_out[K] after the one-survivor rule for users of one AP sharing a slot, and, when
 * bler_out is not NULL, the finite-blocklength block error rate (env.py:107-111) per user.
 */
typedef struct mmw_env mmw_env;
int mmw_env_create(mmw_env** out, int device, int32_t K, int32_t A, const double* sta_xy, const double* ap_xy, double fre_Hz,
                   double txp_offset, double min_s_n_ratio, double min_sinr, double noise_floor_dbm);
int mmw_env_destroy(mmw_env* e);
int mmw_env_sizes(mmw_env* e, int64_t out[4]);
int mmw_env_state(mmw_env* e, int32_t* S_indptr, int32_t* S_indices, double* S_data, int32_t* Q_indptr, int32_t* Q_indices,
                  double* Q_data, double* h_max);
int mmw_env_evaluate(mmw_env* e, const double* z_vec, int32_t Z, double packet_bit, double bandwidth, double slot_time,
                     double* sinr_out, double* bler_out);
/*
 * mmw_create_from_env: mmw_create for the state this generator holds, WITHOUT the host round trip (env.generate_S_Q_hmax ->
 * mmw._process_state, sim_src/env/env.py:168-196 -> sim_src/alg/mmw.py:26-57): the transpose S_T', the association mask, the symmetric
 * pattern of L / X with its per-entry weights, mirrors and pair ids, the edge lists and the row statistics are built by device
 * kernels straight from the generator's receive powers (csrc/pattern_device.h; rows come out sorted, no sort and no atomic), and the
 * rounding's view of the state from its CSR of S_gain.  The handle is the one mmw_create makes from mmw_env_state's arrays: same
 * pattern, same lists (every mmw_read_i32 field equal), S_sum / norm_H / ST_DATA bit-identical.  Only the traversal order of the
 * locality blocking differs: the generator knows the stations' coordinates, so the row blocks are runs of a spatial order instead
 * of patches grown along an RCM order of the pattern (products agree to rounding, not bit for bit; MMW_ENV_RCM=1 forces the latter).
 * The handle does not keep a reference to `env` after the call returns.
 * mmw_env_bounds: the bisection's bounds of binary_search_relaxation.py:13-29 for this state, out = {lower, upper}, from the same
 * count pass (no host matrices).
 */
int mmw_create_from_env(mmw_solver** out, mmw_env* env, int dtype, int32_t Z, int32_t rank_radio, double eta, int32_t nit);
int mmw_env_bounds(mmw_env* e, int32_t out[2]);
/*
 * The online sweeps on one instance of any K (sim_script/journal_version/sim_mmw_online.py:34-88: solve once, then let the stations
 * walk and round the same factor against the state at every time point; ton_major_rv/sim_mmw_online_cmp_methods.py for the arms).
 *
 * mmw_env_move: mob_env.step_time's effect on the state (sim_src/env/env.py:74-87 -> generate_S_Q_hmax, :136-196): the K stations of
 * an existing environment at sta_xy[K][2]; K, A, the access points and the radio parameters stay.  Receive powers, transmit
 * powers, association, AP member lists and S_gain / Q_asso / h_max as CSR are computed again on the device by mmw_env_create's own
 * kernels; the buffers grow when nnz grows.  Afterwards mmw_env_sizes, mmw_env_state, mmw_env_bounds and mmw_env_evaluate answer
 * bitwise what a fresh mmw_env_create at those coordinates answers.  A handle made earlier by mmw_create_from_env or
 * mmw_gm_create_from_env is untouched (neither keeps a reference to `env`).  A coordinate that is not finite: MMW_ERR_ARG, nothing moves.
 *
 * mmw_round_env: mmw_round (sdp_solver.rounding_one_attempt, sdp_solver.py:27-107, as sim_mmw_online.py:60 calls it on the moved
 * state) of gX -- or, with gX == NULL, of the handle's resident factor or spectral block -- against the state `env` holds NOW.  The
 * rounding's view of that state (S_gain's off-diagonal out-lists, the Q lists, h_max) is built on the device from the environment's
 * CSR into a second list set the handle owns, kept for the (environment, generation) it was built from; no host copy of the state.
 * Same kernels, same tie rules, same Zr > 4800 refusal and same outputs as mmw_round.  Nothing of the handle's own state, iterate
 * or factor changes.  Refused with MMW_ERR_ARG before anything is allocated or launched: an environment whose K differs from the
 * handle's, an environment on another device.  A device -1 handle: MMW_ERR_STATE.
 */
int mmw_env_move(mmw_env* e, const double* sta_xy);
int mmw_round_env(mmw_solver* s, mmw_env* e, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv,
                  int32_t* z_out, int32_t* rem_out);
/*
 * All attempts of one sdp_solver.rounding call (sim_src/alg/sdp_solver.py:18-25) in one chain of launches, with the directions drawn
 * and the winner chosen on the device: what mmw_batch_round does for small instances, on the solver handle at any K.
 *
 * mmw_round_attempts: nattempt attempts of mmw_round (sdp_solver.rounding_one_attempt, sdp_solver.py:27-107) on the handle's own
 * state.  The Zr x Dp directions of attempt a (sdp_solver.py:48-49) are Philox4x32-10 normals with counter (row, column pair, a,
 * 0x524e4456) under the key (seed & 0xffffffff, seed >> 32), rows normalised: bitwise mmw_batch_round_randv's for the same
 * (Zr, Dp, seed, a), whatever nattempt is.  The attempts run side by side; then the rule of sdp_solver.py:18-25 picks one on the
 * device.  pick_rule 0, the reference's: the lowest attempt that leaves nobody over, else the last one -- exactly what the loop over
 * single attempts that stops at the first feasible one returns.  pick_rule 1 (not the reference's): the attempt with the fewest users
 * left over, ties to the lower attempt.  z_out[K]: the picked attempt's slots, -1 for a user left over (the caller draws those,
 * sdp_solver.py:104-105); rem_out[nattempt]: every attempt's count of users left over; *pick_out: the picked attempt; z_all
 * [nattempt*K], or NULL: every attempt's slots.  gX as for mmw_round (NULL: the resident factor or spectral block).  What crosses to
 * the host is K + nattempt + 2 integers (and z_all when asked); gX crosses to the device only when the caller hands one.
 * Refused before anything is allocated, copied or launched, MMW_ERR_ARG: Zr or Dp < 1, nattempt outside [1, 256], pick_rule outside
 * {0, 1}, a null output, Zr > 4800 (mmw_round's bound); MMW_ERR_STATE: a device -1 handle, gX == NULL with no resident K x Dp factor.
 *
 * mmw_round_env_attempts: the same against the state `env` holds NOW (sim_script/journal_version/sim_mmw_online.py:60 calls
 * rounding on the moved state), with mmw_round_env's cached second list set and its refusals (another K, another device).
 *
 * mmw_round_randv: the directions of ONE attempt by the same kernel, out[Zr*Dp] row-major (sdp_solver.py:48-49): the seam through
 * which tests compare the draw with tests/helpers/philox_ref.py and with mmw_batch_round_randv.  attempt >= 0; n must be Zr*Dp.
 */
int mmw_round_attempts(mmw_solver* s, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule,
                       int32_t* z_out, int32_t* rem_out, int32_t* pick_out, int32_t* z_all);
int mmw_round_env_attempts(mmw_solver* s, mmw_env* e, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule,
                           int32_t* z_out, int32_t* rem_out, int32_t* pick_out, int32_t* z_all);
int mmw_round_randv(mmw_solver* s, int32_t Zr, int32_t Dp, uint64_t seed, int32_t attempt, double* out, int64_t n);

/*
 * A state that lives on the device as its seven CSR arrays, and the solver handle built from it there: the way in for a graph
 * that is not the generator's (csrc/csr_device.h, csrc/pattern_csr_device.h).  S_gain and Q_asso are (indptr int32 [K+1], indices
 * int32 [nnz], data float64 [nnz]), h_max float64 [K].  nnzS and nnzQ are announced by the caller: the library never learns an
 * array's length from the array.  K >= 1 and 0 <= nnz < 2^31 here; the solver's own limits come with the handle.
 *
 * mmw_csr_upload: the library makes and owns device copies of seven host arrays (device == -1: host copies, no HIP call).
 * mmw_csr_wrap: seven DEVICE pointers are borrowed: the caller keeps them alive and unchanged while the mmw_csr lives, the arrays
 * must be complete when any call that reads them is made, and every call has finished reading when it returns.  A null pointer
 * is allowed exactly where its length is 0 (indices / data of a matrix without stored entries).
 * mmw_csr_sizes: out = {K, 0, nnzS, nnzQ}.  mmw_csr_pointers: the seven device pointers in the argument order of wrap (null for
 * an empty array, all null with device -1).  mmw_csr_state: the host copy of the state, made on request into caller-sized arrays.
 * mmw_csr_bounds: the bisection's bounds of binary_search_relaxation.py:13-29, out = {lower, upper}, from a count pass on the
 * device: lower = longest row of Q + 1, upper = max over rows a of #{j != a : S[a][j] != 0 or S[j][a] != 0} + 2 (for a
 * non-negative S what the host expression on S + S^T gives).  It validates the arrays first, as the creator below does.
 *
 * mmw_create_from_csr: mmw_create for the state `csr` holds, built by kernels: validation, the filtered S and the rounding's lists,
 * S_T' by column counts, placement and a per-row ranking, the L / X pattern by a count pass, host prefix sums and a fill pass in
 * which every entry finds its own place, pair ids, edge lists, mirrors, row statistics.  The handle is bit for bit the one
 * mmw_create makes from the same arrays -- same lists, same values, the same locality blocking (built on the host from the column
 * indices, as there) -- and the lists only the read entries hand out stay on the device until asked for.
 * Validation comes first and refuses with MMW_ERR_ARG and build_pattern's words, the first error being the lowest (kind, row) in
 * this order: indptr[0] != 0; indptr decreasing; indptr[K] != the nnz announced; column out of range; row unsorted or
 * duplicated; stored zero in Q; diagonal in Q; Q asymmetric; then K < 2; Z < 2; a zero norm_H; nnz(L) beyond int32.  The indptr
 * arrays are checked before anything reads indices, the column ranges before any column is used as an address.
 * The handle keeps no reference to `csr` after the call returns.  With a host-only `csr` the handle is mmw_create's with device -1.
 */
typedef struct mmw_csr mmw_csr;
int mmw_csr_upload(mmw_csr** out, int device, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* S_indptr,
                   const int32_t* S_indices, const double* S_data, const int32_t* Q_indptr, const int32_t* Q_indices,
                   const double* Q_data, const double* h_max);
int mmw_csr_wrap(mmw_csr** out, int device, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* S_indptr,
                 const int32_t* S_indices, const double* S_data, const int32_t* Q_indptr, const int32_t* Q_indices,
                 const double* Q_data, const double* h_max);
int mmw_csr_destroy(mmw_csr* c);
int mmw_csr_sizes(mmw_csr* c, int64_t out[4]);
int mmw_csr_pointers(mmw_csr* c, void* out[7]);
int mmw_csr_state(mmw_csr* c, int32_t* S_indptr, int32_t* S_indices, double* S_data, int32_t* Q_indptr, int32_t* Q_indices,
                  double* Q_data, double* h_max);
int mmw_csr_bounds(mmw_csr* c, int32_t out[2]);
int mmw_create_from_csr(mmw_solver** out, mmw_csr* csr, int dtype, int32_t Z, int32_t rank_radio, double eta, int32_t nit);

/*
 * The greedy baselines of sim_src/alg/gm.py on a light handle (csrc/kernels_gm.h): no MMW pattern, no blocking.
 *
 * mmw_gm_create: the per-call preparation of MAX_GAIN.run / MAX_ASSO.run / MAX_RAND.run (gm.py:11-18, 74-80, 136-142), once per state:
 * the rows of S_gain with the diagonal zeroed (setdiag(0), explicit zeros dropped: they add nothing and fail nothing), the rows of
 * Q_asso, h_max, and whether Q is a union of cliques with weights >= 1 (env.py:182-189), in which case the association check is one
 * owner per access point and slot.  S and Q as canonical int32 CSR (sorted, no duplicates), Q without diagonal.
 * device == -1: the same procedures as plain host C++ (no HIP call).
 * mmw_gm_sizes: out = {K, clique groups (-1: Q is not a union of cliques, the general check runs), nnz of the S rows, nnz(Q)}.
 */
typedef struct mmw_gm mmw_gm;
int mmw_gm_create(mmw_gm** out, int device, int32_t K, const int32_t* S_indptr, const int32_t* S_indices, const double* S_data,
                  const int32_t* Q_indptr, const int32_t* Q_indices, const double* Q_data, const double* h_max);
/*
 * mmw_gm_create_from_env: mmw_gm_create for the state `env` holds now (the greedy arm of the online comparison,
 * ton_major_rv/sim_mmw_online_cmp_methods.py:79-88), WITHOUT the host round trip: the S rows, the Q rows and h_max are built on the
 * device from the environment's CSR, and the clique groups come straight from its association (its Q is the same-AP relation,
 * env.py:181-189).  mmw_gm_sizes, mmw_gm_pass, mmw_gm_run and mmw_gm_assign answer exactly what they answer on
 * mmw_gm_create(mmw_env_state(...)).  The handle keeps no reference to `env`: it is a snapshot of the generation it was built from.
 */
int mmw_gm_create_from_env(mmw_gm** out, mmw_env* e);
/*
 * mmw_gm_key: the visiting keys of MAX_GAIN (kind 0, gm.py:11-18: the column sums of S_gain with the diagonal zeroed) and MAX_ASSO
 * (kind 1, gm.py:81: the row sums of Q_asso) for the handle's state, key_out[K], in scipy's summation orders: bitwise the
 * reference's expressions.  A handle built by mmw_gm_create_from_env forms them on the device from its own lists -- there is no host
 * matrix to take them from --; a handle made from host arrays forms them on the host.
 */
int mmw_gm_key(mmw_gm* g, int kind, double* key_out);
int mmw_gm_destroy(mmw_gm* g);
int mmw_gm_sizes(mmw_gm* g, int64_t out[4]);
/*
 * mmw_gm_pass: one slot of MAX_GAIN / MAX_ASSO (the body of `for z in range(Z)`, gm.py:25-56 / 86-113) for the visiting order
 * order[0..n) the caller formed (kindx[np.argsort(-key[not_assigned])], :31-32 / :88-89; distinct users, all unassigned): `nattempt`
 * attempts on sums set to zero once per call and carried from attempt to attempt (:26-27), the first longest list wins (:53-54).
 * list_out[0..*nlist) receives it in acceptance order (caller-sized n).
 */
int mmw_gm_pass(mmw_gm* g, const int32_t* order, int32_t n, int32_t nattempt, int32_t* list_out, int32_t* nlist);
/*
 * mmw_gm_run: the whole slot loop of MAX_GAIN / MAX_ASSO (gm.py:24-58 / 85-115) in one device call, with the visiting order
 * argsort(-key, kind="stable") ranked on the device (ties to the lower user index; the order restricted to the unassigned users is
 * then the same for every slot).  Z: slot bound (K for not_Z_bound, :22-23).  z_out[K]: slot or -1 for a user left unassigned (the
 * caller draws those, :60-64); *zz_out: ZZ, the slots entered (a slot that accepts nobody ends the loop early: every later slot
 * would accept nobody either, ZZ = Z); *rem_out: users left over.
 */
int mmw_gm_run(mmw_gm* g, const double* key, int32_t Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out, int32_t* rem_out);
/*
 * mmw_gm_assign: MAX_RAND's user-major greedy (gm.py:152-193, the same procedure as sdp_solver.rounding_one_attempt) for the user
 * order order[K] (`rank`, :150) and the per-user slot preference pref[K*Z] (row k = sorted_indices[:, k], :149), on the rounding's
 * greedy kernels.  z_out[K]: slot or -1 (the caller draws those, :197-198); *rem_out: users left over.
 */
int mmw_gm_assign(mmw_gm* g, int32_t Z, const int32_t* order, const int32_t* pref, int32_t* z_out, int32_t* rem_out);
/*
 * MAX_RAND.run (gm.py:131-200) with its random part made where the state lies (csrc/kernels_gm_rand.h): nothing is drawn, sorted or
 * uploaded by the host.
 *
 * The draw, stated once.  For (seed, attempt) and the sizes (K, Z):
 *   pref_val[k][z]  a standard normal per user k and slot z -- the reference's inprod[z, k] (gm.py:148) --, a K x Z block, user-major;
 *   order_key[k]    a standard normal per user -- the argument of argsort(randn(K)) (gm.py:150) --, a K x 1 block.
 * Both are Philox4x32-10 under the key (seed & 0xffffffff, seed >> 32) with the counter (row, column pair, attempt, TAG): row = k, a
 * pair of pref_val holds the slots 2p and 2p + 1 (an odd Z discards the second normal of the last pair), order_key is the first
 * normal of pair 0; TAG = 0x47525046 ("GRPF") for pref_val and 0x47524b59 ("GRKY") for order_key, apart from the sketch's 0x4d4d5753
 * and the rounding's 0x524e4456.  The four words give the sketch's two uniforms u1 = ((w0 << 21 ^ w1 >> 11) + 1) 2^-53 in (0, 1] and
 * u2 = (w2 + w3 2^-32) 2^-32 in [0, 1) and Box-Muller's pair sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2).  Because these normals decide
 * integers that a device -1 handle has to give too, ln, cos and sin are not a math library's but one fixed sequence of IEEE double
 * additions, multiplications, one division and one square root, without contraction (gmr_normals, csrc/kernels_gm_rand.h): the same
 * bits on the device and on the host, some 2 ulp from the exact functions.  A value depends on (seed, attempt, K, Z, k, z) and on
 * nothing else: not on launch geometry, not on the batch's composition, not on `take`.
 *   User order: ascending order_key, ties to the lower user index.
 *   Preference of user k: descending pref_val[k][.], ties to the lower slot (the rule of the rounding's preference rows).
 *
 * mmw_gm_rand: attempts 0 ... nattempt - 1 of that draw, each through mmw_gm_assign's greedy (gm.py:152-193) for its own order and
 * preference table, formed on the device by the rounding's rank and preference kernels; then one of them is picked on the device by
 * mmw_round_attempts' two rules.  pick_rule 0: the first attempt that leaves nobody over, else the last.  pick_rule 1: the attempt
 * with the fewest users left over, ties to the lower attempt.  z_out[K]: the picked attempt's slots, -1 for a user left over (the
 * caller draws those, gm.py:196-198); rem_out[nattempt]: every attempt's count; *pick_out: the picked attempt.  The reference runs a
 * single attempt: nattempt = 1 is the drop-in case.  K + nattempt + 1 integers cross to the host, nothing crosses to the device.
 * Refused with MMW_ERR_ARG before anything is allocated or launched, each naming the value: Z < 1, nattempt outside [1, 256],
 * pick_rule outside {0, 1}, a null output, Z > 4800 (mmw_round's bound: 32 Z bytes of LDS in the greedy kernel).
 * device == -1: the same procedure as plain host C++, the draw through the host form of the same functions -- equal bit for bit.
 * A handle built by mmw_gm_create_from_env answers exactly like one built from the host state.
 *
 * mmw_gm_rand_draw: the draw of ONE attempt copied out, pref_val_out[K*Z] (user-major) and order_key_out[K], either may be NULL: the
 * seam for tests and for a host comparator, the counterpart of mmw_round_randv.  attempt >= 0; Z as above.
 */
int mmw_gm_rand(mmw_gm* g, int32_t Z, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out, int32_t* rem_out, int32_t* pick_out);
int mmw_gm_rand_draw(mmw_gm* g, int32_t Z, uint64_t seed, int32_t attempt, double* pref_val_out, double* order_key_out);

/*
 * Batched solver: B small independent fp64 instances, ONE workgroup per instance and `n` MMW iterations per launch
 * (csrc/kernels_batch.h).  For the sweeps of the reference (many seeds x cell sizes, K = 75 ... 675 users per instance), where a
 * handle's iteration is a chain of ~20 launches of a few us each.  Nothing waits across workgroups and every reduction runs in a
 * fixed order inside the instance's workgroup: an instance's results are bitwise independent of its batch neighbours and of how
 * its iterations are split into calls.  Limits (refused with MMW_ERR_ARG and a message; such instances stay on handles):
 * K <= 4096, D = Z * rank_radio <= 512, nnzL <= 2^22, 96 MiB of device memory per instance.
 *
 * mmw_batch_create: mmw_create's state processing (csrc/pattern.h) per instance -- K[b], Z[b], nit[b] and the CSR arrays of
 * instance b behind the b-th pointer of each array -- then all of them packed into one device arena at the initial point.
 * device == -1 builds the host side only (mmw_batch_read_i32 and the host fields S_SUM / NORM_H / ST_DATA answer).
 * mmw_batch_sizes: out as mmw_sizes for instance `inst` (Dpad = D: the batch keeps K x D blocks unpadded).
 */
typedef struct mmw_batch mmw_batch;
int mmw_batch_create(mmw_batch** out, int device, int32_t B, const int32_t* K, const int32_t* Z, int32_t rank_radio, double eta,
                     const int32_t* nit, const int32_t* const* S_indptr, const int32_t* const* S_indices, const double* const* S_data,
                     const int32_t* const* Q_indptr, const int32_t* const* Q_indices, const double* const* Q_data, const double* const* h_max);
int mmw_batch_destroy(mmw_batch* b);
int mmw_batch_sizes(mmw_batch* b, int32_t inst, int64_t out[10]);
/* per-instance slot counts for the next probes (norm_H and D rebuilt, every instance reset to the initial point with `nit`);
 * Z[b] <= 0 takes instance b out of the runs until a later call gives it a slot count */
int mmw_batch_set_slots(mmw_batch* b, const int32_t* Z, int32_t nit);
/*
 * mmw_batch_set_slots_warm: the same rebinding, but every instance that has iterated CONTINUES from its previous probe's iterate
 * instead of the reference's initial point (opt-in warm start of the bisection as mmw_set_slots_warm: binary_search_relaxation.py:44-72
 * calls the solver once per probed Z and the reference restarts each time, mmw.py:62-68): e_accu, L_accu and the last X / Y are
 * kept, the running sums of X and Y restart (the batch adds X_i / Y_i when iteration i starts, so after n iterations they hold the
 * kept X / Y and n - 1 new terms), the iterations done read 0 and `nit` more are announced.  An instance that has not iterated
 * falls back to mmw_batch_set_slots.  Z[b] <= 0 takes instance b out of the runs WITH its iterate and its counters carried over,
 * so a later warm call with a slot count picks it up where it stopped.  Both entries move the arena on the device
 * (csrc/kernels_batch_relayout.h: one small upload and one launch, into a second arena that then trades places with the first).
 * MMW_ERR_STATE on a host-only batch.
 */
int mmw_batch_set_slots_warm(mmw_batch* b, const int32_t* Z, int32_t nit);
/*
 * mmw_batch_carry: the warm start ACROSS states (the stations have moved; a re-solve per time point of the online sweeps).  `src` is
 * a batch on the old states that has iterated, `dst` a batch on the new states as mmw_batch_create made it, at any slot counts, that
 * has not.  For every instance `take` flags (NULL: all) the iterate (e_accu, L_accu, X, Y) of `src` is re-indexed onto `dst`'s
 * pattern and constraints: entry (row, col) of L and X receives src's value at (row, col) where src's pattern stores it, else 0 (the
 * diagonal is in both, so X's diagonal always carries); e_accu and Y, laid out [D-part K | F-part E_asso | H-part K], carry the D-
 * and the H-part by user index and the F-part by pair (asso_x, asso_y), 0 for a pair src does not have.  Y is NOT renormalised: the
 * first iteration's softmax rewrites it, and before that only the first term of the running sum of Y and the first row of the gap
 * log read it.  Everything else of `dst` stays as creation left it: sums, e_this, the K x D blocks and the info record zero, the
 * iterations done 0 and `nit` unchanged -- so a later mmw_batch_set_slots_warm on `dst`, whose rule is unchanged, still treats a
 * carried instance that has not iterated as cold.  A taking instance whose `src` counterpart has run no iteration is left cold (not
 * an error: mmw_batch_set_slots_warm's fallback).  The index maps are merged on the host from the two batches' patterns and go up in
 * one copy; one launch (csrc/kernels_batch_carry.h) on dst's stream does the rest, after src's stream has been synchronised.
 * Refused before anything is written, both batches untouched: dst == src, a host-only batch (MMW_ERR_STATE), different devices,
 * different B, K[b] of a taking instance different in the two, a taking dst instance that has iterated (MMW_ERR_STATE).
 * mmw_batch_carry_map: the two maps of instance `inst` as mmw_batch_carry computes them -- lmap[nl = nnzL of dst] the position in
 * src's L / X values, cmap[nc = C of dst] the position in src's constraint vector, -1 where src has none.  Host patterns only:
 * device == -1 batches answer too.
 */
int mmw_batch_carry(mmw_batch* dst, mmw_batch* src, const int32_t* take);
int mmw_batch_carry_map(mmw_batch* dst, mmw_batch* src, int32_t inst, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc);
int mmw_batch_reset(mmw_batch* b, int32_t nit);
/* one step size per instance (eta[B]) for the iterations that follow */
int mmw_batch_set_eta(mmw_batch* b, const double* eta);
/* Taylor degree cap per substep (<= 16) and target relative accuracy of exp(L/2)R, per column (default 16, 1e-9) */
int mmw_batch_set_expm(mmw_batch* b, int max_order, double tol);
/*
 * mmw_batch_iterate: every instance runs min(n, nit - iterations done) iterations of mmw.py:75-200 in one launch; returns when done.
 * randv: NULL -> Philox sketches on the device, instance b keyed by seeds[b] with the counter layout of mmw_iterate(..., NULL, seed)
 * (a block is bitwise mmw_sketch's); otherwise the row-normalised K x D blocks of every instance that runs, instance after instance,
 * iteration-major within an instance (parity mode).
 */
int mmw_batch_iterate(mmw_batch* b, int32_t n, const double* randv, const uint64_t* seeds);
/*
 * The duality gap inside the batch: the LOG_GAP branch mmw.py:79-117 as a phase of the instance's own workgroup, so a whole
 * convergence sweep (every instance, every iteration, every gap row) stays ONE launch per mmw_batch_iterate.
 *
 * mmw_batch_set_gap: from the next mmw_batch_iterate on, every iteration i of every active instance logs one row when it starts,
 * from the i + 1 terms X_0 .. X_i / Y_0 .. Y_i of the running sums (mmw.py:77-81): {e_max = the largest constraint violation at
 * Xbar, K * theta with theta = lambda_min(L(Ybar)) by plain Lanczos, e_max - K * theta, steps} -- LOGGED_NP_DATA["gap"][:, 3:6] of
 * the reference and the Lanczos steps taken.  The recurrence stops at |beta_m s_m| <= 1e-11 * scale (mmw_gap's fp64 criterion), on
 * an invariant subspace, or at m = min(K, m_cap); `steps` is NEGATIVE when m_cap was reached without meeting the criterion (theta
 * is then a Ritz value, an upper bound of lambda_min).  m_cap <= 0 takes the default 600, m_cap > 1024 is refused.  The phase only
 * reads the iterate: with the gap on every other field is bitwise what it is with the gap off, and a row is bitwise independent of
 * the batch neighbours and of how the iterations are split into calls.  The log and the phase's work space (nnzL + 5 K doubles
 * per instance) live in a buffer of their own, allocated when the gap is first enabled.  Rows of iterations that ran while the gap
 * was off are NaN; mmw_batch_reset / mmw_batch_set_slots clear the log and keep the setting.  MMW_ERR_STATE on a host-only batch.
 * mmw_batch_read_gap: the rows of instance `inst`, 4 doubles per iteration done (n must be 4 x that count); MMW_ERR_STATE if the
 * gap was never enabled.
 */
int mmw_batch_set_gap(mmw_batch* b, int enabled, int32_t m_cap);
int mmw_batch_read_gap(mmw_batch* b, int32_t inst, double* out, int64_t n);
/*
 * Several workgroups for a large instance (csrc/kernels_batch_split.h).  A batch launch lasts as long as its largest instance runs
 * on its one workgroup; mmw_batch_set_split gives instance b parts[b] workgroups, 1 ... MMW_BATCH_MAX_PARTS (a value outside is
 * refused by instance with MMW_ERR_ARG and leaves the setting as it was).  While any instance that runs has parts > 1,
 * mmw_batch_iterate enqueues every iteration as three launches for all instances together -- head (gap row, averaging, DUAL, softmax,
 * LOSS: one workgroup per instance), exp(L/2)R (one workgroup per column slice of the sketch: width 8 ceil(ceil(D / parts) / 8)
 * columns, ceil(D / width) slices, so D < 8 has one) and X on the pattern (one workgroup per range of nnzL / parts stored entries)
 * -- on the batch's stream, kernel boundaries being the only synchronisation, and returns when all are done.  Every column and every
 * entry is computed by the same sums in the same order as in the single launch: all fields, the gap log and EXPM_INFO are bitwise
 * what they are without the split, whatever the parts, the batch neighbours and the split of the iterations into calls.  NULL or all
 * ones selects the single launch (the default).  The setting survives mmw_batch_reset and mmw_batch_set_slots; the slices follow
 * the current D at every mmw_batch_iterate.  The work tables live in buffers of their own: the arenas do not move.  MMW_ERR_STATE on
 * a host-only batch.
 */
#define MMW_BATCH_MAX_PARTS 32
int mmw_batch_set_split(mmw_batch* b, const int32_t* parts);
/*
 * The rows of a Taylor term over workgroups (csrc/kernels_batch_rows.h).  mmw_batch_set_split cuts exp(L/2)R by sketch column only, at
 * most ceil(D / 8) workgroups per instance; mmw_batch_set_row_split gives instance b rows[b] row parts, 1 ... MMW_BATCH_MAX_ROW_PARTS (a
 * value outside is refused by instance with MMW_ERR_ARG and leaves the setting as it was), multiplied with its column slices.  While
 * any instance that runs has rows > 1, mmw_batch_iterate enqueues every iteration for all instances together as: the head of the
 * column split; a plan launch whose records (mu, rho, substeps, order per instance) the host reads -- one synchronisation per
 * iteration, after which the host knows the length nsub (1 + order) of every schedule; per launch of the longest schedule one
 * workgroup per (instance, column slice, row part), which starts a substep or adds one Taylor term on its own rows and columns and
 * returns at once when it is past its instance's schedule or all its columns have stopped; X on the pattern with slices x rows entry
 * ranges.  Kernel boundaries are the only synchronisation.  The row ranges are contiguous, cover [0, K) and are balanced by stored
 * entries of L: boundary p is the first row at which the prefix of L's indptr reaches p nnzL / rows, so a range may be empty
 * (mmw_batch_row_ranges writes the rows + 1 boundaries of instance `inst`; it also answers on a host-only batch).  A row's sum runs
 * over its entries in CSR order whichever workgroup owns it and the stop rule is built from maxima only: all fields, the gap log and
 * EXPM_INFO are bitwise what the single launch gives.  NULL or all ones selects what runs without it (the default).  The setting
 * survives mmw_batch_reset and mmw_batch_set_slots.  Tables, records and slabs live in buffers of their own: the arenas do not move.
 * MMW_F_SPLIT_CALL says which path the last mmw_batch_iterate took.  MMW_ERR_STATE on a host-only batch.
 */
#define MMW_BATCH_MAX_ROW_PARTS 64
int mmw_batch_set_row_split(mmw_batch* b, const int32_t* rows);
int mmw_batch_row_ranges(mmw_batch* b, int32_t inst, int32_t rows, int32_t* out);
/*
 * The head and the plan over workgroups (csrc/kernels_batch_head.h).  Both splits above leave everything in front of the exponential --
 * averaging, both DUAL passes, the softmax, the LOSS update and the plan's pass over L, all O(nnzL) -- on one workgroup per instance,
 * and let every entry range of X recompute all K row sums of X_half X_half^T.  mmw_batch_set_head_split gives instance b parts[b] row
 * parts for that work, 1 ... MMW_BATCH_MAX_HEAD_PARTS (a value outside is refused by instance with MMW_ERR_ARG and leaves the setting
 * as it was).  While any instance that runs has parts > 1, every iteration goes through the split paths -- with neither
 * mmw_batch_set_split nor mmw_batch_set_row_split that is the column split's path with one slice per instance -- and its head is the
 * launches [gap row] averaging, DUAL, fold, LOSS: one workgroup per (instance, row part), except the gap row and the fold (e_accu,
 * softmax, the LOSS constant: O(C)), which stay on one workgroup per instance.  On the row split's path the plan becomes an O(K)
 * launch over per-row values the LOSS launch left; the host's one synchronisation per iteration stays where it is.  Behind the
 * exponential a launch forms the row sums of X_half X_half^T once, by row part, and X on the pattern reads them.  Kernel boundaries
 * are the only synchronisation.  The row ranges are those of mmw_batch_row_ranges' rule (mmw_batch_head_ranges writes the parts + 1
 * boundaries of instance `inst`; it also answers on a host-only batch); part p also owns the pairs [p E_asso / parts, (p + 1) E_asso
 * / parts).  Per-entry and per-row statements do not depend on their owner, a row's sum runs over its entries in CSR order, and every
 * sum across threads stays on one workgroup with the single launch's thread map: all fields, the gap log and EXPM_INFO are bitwise
 * what the single launch gives.  NULL or all ones turns it off (the default): every launch is then what it is without this entry.
 * The setting survives mmw_batch_reset and mmw_batch_set_slots.  Tables, records and scratch live in buffers of their own: the arenas
 * do not move.  MMW_F_HEAD_CALL says whether the last mmw_batch_iterate took the head path; MMW_F_SPLIT_CALL keeps its meaning and
 * counts the head path's launches among its own.  MMW_ERR_STATE on a host-only batch.
 */
#define MMW_BATCH_MAX_HEAD_PARTS 64
int mmw_batch_set_head_split(mmw_batch* b, const int32_t* parts);
int mmw_batch_head_ranges(mmw_batch* b, int32_t inst, int32_t parts, int32_t* out);
/* the fields of instance `inst` by the MMW_F_* / MMW_I_* ids: Y, E_ACCU, E_THIS, LVAL, XVAL, XAVG, YAVG, XHALF, SKETCH, S_SUM, NORM_H,
 * ST_DATA, EXPM_INFO ({rho, Taylor steps taken, substeps, mu}) and every pattern array; MMW_F_PATTERN / MMW_I_PATTERN (the pattern
 * part of the instance's two arenas as the kernels read it) and MMW_F_BUILD_INFO (how the batch was built, mmw_batch_create_from_env);
 * other ids are refused */
int mmw_batch_read_f64(mmw_batch* b, int32_t inst, int which, double* out, int64_t n);
int mmw_batch_read_i32(mmw_batch* b, int32_t inst, int which, int32_t* out, int64_t n);
/* the block the device generator draws for instance `inst` in `iteration` of a run with `seed` (mmw_sketch's semantics) */
int mmw_batch_sketch(mmw_batch* b, int32_t inst, uint64_t seed, int32_t iteration, double* out, int64_t n);
/*
 * mmw_batch_export: device-to-device copy of the instance's iterate (L, X, Xbar sum, Y, Ybar sum, e_accu, e_this, iteration count,
 * nit) into an fp64 handle that mmw_create made from the same (state, Z): the handle is reset first (plans, chains, timers), its
 * derived copies of L are rebuilt, and it then behaves as if it had run those iterations itself -- mmw_factor, mmw_round and mmw_gap
 * run on it unchanged, and further mmw_iterate calls continue the run.  The batch's MMW_F_XAVG / MMW_F_YAVG hold X_0 + ... + X_{i-1}
 * after i iterations; a handle's hold X_0 + ... + X_i while iterations remain (mmw_gap reads i + 1 terms), so before the last
 * iteration the export adds the current X and Y to the sums it hands over.  Refuses fp32 handles and a handle whose K / Z / pattern
 * differ.
 */
int mmw_batch_export(mmw_batch* b, int32_t inst, mmw_solver* h);
/*
 * The epilogue of a probe inside the batch (csrc/kernels_batch_epilogue.h): X_half and the rounding of every instance in ONE launch
 * each, one workgroup per instance, instead of one mmw_batch_export + mmw_factor + mmw_round trip per instance.  Opt-in: nothing
 * else changes, the arenas and every field mmw_batch_read_f64 hands out stay bitwise as they were (the work space is a buffer of
 * its own, made on first use and sized for the taking instances), and an instance's factor and slots are bitwise independent of its
 * batch neighbours.  Limits: K <= MMW_BATCH_EPILOGUE_MAX_K and the batch's own D <= 512; a taking instance over the limit is refused
 * by name with MMW_ERR_ARG before anything runs (it stays on the handle path), a host-only batch answers MMW_ERR_STATE.
 *
 * mmw_batch_factor: X_half = U sqrt(S) of the top-`rank` singular triplets of Xbar = (sum of X) / nit (mmw.py:201, 213-216) for every
 * taking instance, by a dense one-sided Jacobi on the rows of the symmetric Xbar: the row norms at convergence are |lambda|, the
 * singular values svds ranks by, so a kept set that is mostly negative eigenvalues comes out as svds gives it.  Columns are in
 * ascending sigma (svds' order); a kept singular value of exactly 0 gives a zero column.  take[B]: non-zero = the instance takes
 * part, NULL = every active instance.  rank[B]: NULL = min(K - 1, (Z - 1) * rank_radio) (mmw.py:214); 1 <= rank <= K.  An instance
 * that has not run its `nit` iterations gets MMW_ERR_STATE -- unless xavg[b] is non-NULL (parity mode): then instance b's Xbar is
 * the nnzL values xavg[b] on its pattern, in MMW_F_XAVG's order (taken as given, not divided; symmetric), instead of the run's.
 * The factor stays on the device for mmw_batch_round; mmw_batch_read_f64(MMW_F_FACTOR) copies it out ([K*rank], row-major) and
 * MMW_F_FACTOR_INFO its record.  An instance still rotating at the cap of 30 sweeps keeps its factor and is named on stderr.  The factors of a call stand until the next mmw_batch_factor, mmw_batch_set_slots or mmw_batch_reset.
 *
 * mmw_batch_round: sdp_solver.rounding (sdp_solver.py:18-107) of the resident factor of every taking instance (take as above; a
 * taking instance without a factor gets MMW_ERR_STATE).  Attempt a of instance b draws randv[Z, rank] from Philox keyed by
 * (seeds[b], a), row-normalised (:48-49); users are visited by descending ||gX_k|| (:51) and take the first slot of their descending
 * inprod order (:56-57, ties to the lower slot) that passes the three checks of :78-92, as mmw_round.  Attempts run one after
 * another; stop_at_first != 0 ends an instance after its first attempt that leaves nobody over (:23-24).  z_out: nattempt * K slots
 * per TAKING instance, instance after instance, attempt-major; -1 = the user was left unassigned (the caller draws those,
 * :104-105), -2 = the attempt was not run.  rem_out[B * nattempt]: users left over per attempt (-1: not run, or the instance did
 * not take part); used_out[B]: attempts run.
 *
 * mmw_batch_round_randv: the randv[Z * rank] that attempt `attempt` of instance `inst` draws with `seed`, bitwise (n must be
 * Z * rank of the instance's resident factor).
 */
#define MMW_BATCH_EPILOGUE_MAX_K 1024
/*
 * Several workgroups for the factor of a large instance (csrc/kernels_batch_factor_split.h).  mmw_batch_factor lasts as long as the
 * dense Jacobi of its largest instance runs on its one workgroup; mmw_batch_set_factor_split gives instance b parts[b] workgroups per
 * tournament round, 1 ... MMW_BATCH_MAX_PARTS (a value outside is refused by instance with MMW_ERR_ARG and leaves the setting as it
 * was).  While any TAKING instance of a call has parts > 1, mmw_batch_factor enqueues the factors of all taking instances together as
 * head (Xbar into the dense work matrix: one workgroup per instance), one launch per round of the tournament (one workgroup per item:
 * a contiguous range of ceil(P / parts) of the instance's P = ceil(K / 2) row pairs, ceil(P / that) <= parts items, none empty; an
 * instance with parts = 1 has one), one small launch per sweep that sums the items' rotation counts and largest |cos|, and tail (row
 * norms, the rank cut, X_half, the record) -- on the batch's stream, kernel boundaries being the only synchronisation, with one host
 * synchronisation per sweep to drop the instances that have ended from the later launches.  A row pair is reduced and rotated by one
 * wave whichever workgroup takes it, and a sweep's rotation count and largest |cos| are exact in any order: MMW_F_FACTOR,
 * MMW_F_FACTOR_INFO and everything mmw_batch_round makes of them are bitwise what the single launch gives, whatever the parts, the
 * batch neighbours and `take`.  Argument checks, parity mode (xavg) and the stderr line at the sweep cap are those of the single
 * launch.  NULL or all ones selects the single launch (the default).  The setting survives mmw_batch_reset and mmw_batch_set_slots; the
 * items follow the instances' K at every mmw_batch_factor.  The item table, the slab of per-item sums and the sweep records live in
 * buffers of their own: the epilogue's work space keeps its layout.  MMW_F_FACTOR_CALL says which path the last call took.
 * MMW_ERR_STATE on a host-only batch.
 */
int mmw_batch_set_factor_split(mmw_batch* b, const int32_t* parts);
int mmw_batch_factor(mmw_batch* b, const int32_t* take, const int32_t* rank, const double* const* xavg);
int mmw_batch_round(mmw_batch* b, const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out,
                    int32_t* rem_out, int32_t* used_out);
int mmw_batch_round_randv(mmw_batch* b, int32_t inst, uint64_t seed, int32_t attempt, double* out, int64_t n);
/*
 * The baselines the reference's sweep scripts run beside the MMW search on every instance (sim_script/journal_version/
 * sim_all_bler.py:30-72: rand_sdp_solver, MAX_GAIN.run and MAX_ASSO.run at Z_fin; ton_major_rv/sim_mmw_online_cmp_methods.py:79-88:
 * MAX_GAIN.run(-1, not_Z_bound=True) once per drop), inside the batch: one launch per call, one workgroup per taking instance
 * (csrc/kernels_batch_gm.h), instead of one mmw_gm_create, one host-made key and one single-wave mmw_gm_run per instance.  Opt-in:
 * the arenas, the resident MMW fields and (for mmw_batch_gm) the resident factors stay bitwise as they were; an instance's result is
 * bitwise independent of its batch neighbours and of `take`.
 *
 * mmw_batch_gm: gm.MAX_GAIN.run (kind 0, sim_src/alg/gm.py:9-66) or gm.MAX_ASSO.run (kind 1, gm.py:69-127) of every taking instance on
 * the state the batch was built from, in the stable visiting order (argsort(-key, kind="stable"): ties to the lower user index, the
 * rule of mmw_gm_run).  The key is formed on the device and is bitwise the reference's expression: kind 0, the column sums of S_gain
 * with the diagonal zeroed accumulated in ascending row (gm.py:11-18: scipy's CSC matvec behind S.transpose().sum(axis=1)); kind 1,
 * the row sums of Q_asso in stored order (gm.py:81).  The slot loop is gm.py:24-58 / 85-115 as mmw_gm_run runs it: the sums zeroed
 * once per slot, `nattempt` attempts on them, the first longest list wins, a slot that accepts nobody ends the loop with ZZ = Z, and
 * the loop ends early when everybody is assigned.  take[B]: as in mmw_batch_round.  Z[B]: the slot bound per instance; Z[b] <= 0 is
 * not_Z_bound (gm.py:22-23): the bound is K and the caller's fill range is ZZ (gm.py:60-64).  z_out: K entries per TAKING instance,
 * instance after instance, the slot or -1 for a user left over (the caller draws those, gm.py:60-64); zz_out[B] / rem_out[B]: ZZ and
 * the users left over, -1 for an instance that did not take part; key_out: NULL, or the key of every taking instance laid out as
 * z_out.  One copy of the descriptors in, one launch, one copy of the results back.
 * Refused by name with MMW_ERR_ARG before anything runs (the outputs stay untouched): a taking instance with
 * K > MMW_BATCH_EPILOGUE_MAX_K, or whose Q_asso is not a union of cliques with weights >= 1 -- every state env.generate_S_Q_hmax
 * makes is one (env.py:182-189), mmw_batch_create decides it; such an instance stays on a GreedyHandle (mmw_gm_create) --, kind
 * outside {0, 1}, nattempt < 1, and a call in which no instance takes part.  A host-only batch (device -1) answers with the same
 * procedure as plain host C++, key and order included.
 *
 * mmw_batch_env_gm (declared with the environment below): the same on the state the environment holds after its last move
 * (MAX_GAIN.run on e.generate_S_Q_hmax(), sim_mmw_online_cmp_methods.py:79-81); the association is the group id.  take: non-zero =
 * the instance takes part, NULL = every instance.  MMW_ERR_STATE before the first move.
 *
 * mmw_batch_factor_random: rand_sdp_solver.run_with_state (sim_src/alg/sdp_solver.py:109-114), a K x (Z * rank_radio) block of
 * normals with its rows normalised, as the RESIDENT FACTOR of every taking instance, rank = D = Z * rank_radio (D may exceed K).  The
 * block of instance b with seeds[b] is bitwise mmw_batch_sketch(b, inst, seeds[b], 0).  No iteration needs to have run.  As with
 * mmw_batch_factor the work buffers are laid out anew (earlier factors are gone) and a host-only batch answers MMW_ERR_STATE;
 * mmw_batch_round, mmw_batch_round_env, mmw_batch_round_randv and MMW_F_FACTOR / MMW_F_FACTOR_INFO ({0, 0, D, 0, 0}) then work on it,
 * with one rule of its own: every row has norm 1, so the rounding's visiting order (descending norm, sdp_solver.py:51) is one tie
 * over all users, and the rounding visits such a block in index order (ties to the lower index) without forming the norms, whose
 * last bits would decide the order otherwise.  A factor of mmw_batch_factor is rounded exactly as before.
 *
 * mmw_batch_factor_spectral: spectral_sdp_solver.run_with_state (sim_src/alg/sdp_solver.py:165-185) as the RESIDENT FACTOR of every
 * taking instance (csrc/kernels_batch_spectral.h): the Laplacian L = D - W of the state the batch was built from, W = S_gain +
 * S_gain^T with the diagonal zeroed (the state's CSR is taken as canonical: no entry stored twice) and D_ii = sum_j W_ij, its Z[b]
 * eigenvectors of largest eigenvalue as a K x Z block, columns in ascending eigenvalue (eigsh's order), every row of the block divided
 * by its norm (:182).  The reference takes eigsh(k = Z, which = 'LM', tol = 1e-5); here the eigenvectors come from mmw_batch_factor's
 * dense one-sided Jacobi on the rows of L, to rounding error: L is positive semidefinite, so the row norms at convergence are the
 * eigenvalues.  L is built without atomics and exactly symmetric, every sum in a fixed order: an instance's block is bitwise
 * independent of its batch neighbours and of `take`, and the single launch and the chain of mmw_batch_set_factor_split give the same
 * bits.  The sign of a column is arbitrary but deterministic (comparisons belong on the projector V V^T).  take[B]: as in mmw_batch_factor.  Z[B]: NULL = each instance's own slot count; otherwise
 * 1 <= Z[b] <= K (eigsh itself refuses k >= K; the Jacobi does not, and the one-AP shape K = 2, Z = 2 rounds).  The eigenvector of
 * eigenvalue 0 is the one a row norm cannot carry: its row ends as rounding noise or as exact zeros (a zero-norm row gives a zero
 * column); it ranks last and enters the block only at Z = K.  A user whose row of the K x Z block is exactly zero keeps a zero row
 * -- an isolated user is one; the reference divides by zero there.  Users whose row is tiny before the division (the top eigenvectors
 * of these Laplacians are localised: norms down to 1e-14) carry amplified rounding noise, here as in the reference.  No iteration
 * needs to have run.  As with mmw_batch_factor_random the work buffers are laid out anew (earlier factors are gone).  Refused by name
 * with MMW_ERR_ARG before anything runs: a taking instance with K > MMW_BATCH_EPILOGUE_MAX_K, or Z[b] outside [1, K]; a host-only
 * batch answers MMW_ERR_STATE.  An instance still rotating at the cap of 30 sweeps keeps its block and is named on stderr as by
 * mmw_batch_factor.  mmw_batch_round, mmw_batch_round_env, mmw_batch_round_randv, MMW_F_FACTOR ([K * Z], row-major),
 * MMW_F_FACTOR_INFO ({sweeps, largest |cos| of a row pair met in the last sweep, Z, lambda_Z, lambda_Z+1 (0 at Z = K)}) and
 * MMW_F_FACTOR_CALL then work on it, and MMW_F_FACTOR_ROWNORM hands out the users' row norms before the division; the rows being unit (or zero), the rounding visits the users in index order as for
 * mmw_batch_factor_random.
 */
int mmw_batch_gm(mmw_batch* b, int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out,
                 int32_t* rem_out, double* key_out);
int mmw_batch_factor_random(mmw_batch* b, const int32_t* take, const uint64_t* seeds);
int mmw_batch_factor_spectral(mmw_batch* b, const int32_t* take, const int32_t* Z);
/*
 * mmw_batch_gm_rand: gm.MAX_RAND.run (gm.py:131-200) of every taking instance on the state the batch was built from, one launch, one
 * workgroup per instance (csrc/kernels_batch_gm.h, k_batch_gm_rand).  Attempt a of instance b is the draw of mmw_gm_rand for
 * (seeds[b], a) with the instance's (K, Z[b]) -- order keys, preference values, ascending order, descending preference, ties as stated
 * there -- followed by the greedy pass mmw_batch_round runs (the same three checks, the same accumulation order): the slots and counts
 * are bitwise those of mmw_gm_rand(seed = seeds[b]) on a handle of the same state, alone, among neighbours and under any `take`.
 * take[B]: as in mmw_batch_round.  Z[B]: the slot count per instance; an instance with Z[b] <= 0 is left out like one with take[b] = 0
 * (MAX_RAND has no not_Z_bound).  Attempts run one after another; stop_at_first != 0 ends an instance after its first attempt that
 * leaves nobody over.  Outputs in mmw_batch_round's shapes: z_out, nattempt * K slots per instance that ran, instance after instance,
 * attempt-major, -1 = left over (the caller draws those, gm.py:196-198), -2 = attempt not run; rem_out[B * nattempt] (-1: not run or
 * left out); used_out[B]: attempts run.  The greedy pass reads the columns of Q_asso themselves, so mmw_batch_gm's
 * clique condition is NOT needed here; the limits are K <= MMW_BATCH_EPILOGUE_MAX_K and Z[b] <= MMW_BATCH_EPILOGUE_MAX_K (one flag per
 * slot in LDS).
 * Refused by name with MMW_ERR_ARG before anything runs (outputs untouched): a null Z, seeds or output, nattempt outside [1, 4096],
 * a running instance over either limit, a call in which no instance runs.  The arenas, the resident MMW fields and the resident
 * factors stay bitwise as they were.  A host-only batch (device -1) answers with the same procedure as plain host C++.
 * mmw_batch_env_gm_rand (declared with the environment below): the same on the state of the environment's last move.
 */
int mmw_batch_gm_rand(mmw_batch* b, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds,
                      int32_t* z_out, int32_t* rem_out, int32_t* used_out);

/*
 * The generator and the scorer for many small instances (csrc/kernels_batch_env.h), one workgroup per instance: the state of
 * every time point of the reference's online sweeps (sim_script/journal_version/sim_mmw_online.py:34-78 -- per seed and variant,
 * at 11 time points, alg.rounding(Z_fin, gX, e.generate_S_Q_hmax()) on the stations as they have moved, e.evaluate_bler(z_vec, Z_fin),
 * e.step_time(...)) without one mmw_env_create, one solver handle and one mmw_env_evaluate per instance and point.  No atomics,
 * nothing waits across workgroups, every reduction runs in a fixed order: an instance's results are bitwise independent of its
 * batch neighbours, and its state is bitwise the one mmw_env_create builds at the same positions.
 * Limits: K <= MMW_BATCH_EPILOGUE_MAX_K, A <= 1024; an instance over the limit is refused by name with MMW_ERR_ARG before anything
 * runs, and so is device == -1 (there is no host form).
 *
 * mmw_batch_env_create: env.__init__'s parameters (sim_src/env/env.py:12-37) for B instances with K[b] stations and the A[b] access
 * points ap_xy[b][A][2].  It holds no positions yet: every other entry answers MMW_ERR_STATE until the first move.
 * mmw_batch_env_move: env.generate_S_Q_hmax (env.py:136-196) of every instance for the stations at sta_xy[b][K][2] -- where
 * mob_env.step_time (sim_src/env/mob_env.py:20-21, env.py:74-87; the caller's, graphs.mobile_drop) has taken them: all positions go
 * up in one copy, a count pass, one readback of the B totals, the fill pass.  The lists live in a grow-only arena.
 * mmw_batch_env_sizes / mmw_batch_env_state: mmw_env_sizes / mmw_env_state for instance `inst`.
 * mmw_batch_env_evaluate: env.evaluate_sinr / evaluate_bler (env.py:198-233) of one colouring z_vec[b][K] with Z[b] slots per
 * instance, ONE launch for all: interference summed member by member in ascending user order, the one-survivor rule per (AP, slot),
 * users with z outside [0, Z) keep 1e-3; sinr_out[b][K], and bler_out[b][K] unless bler_out is NULL.
 *
 * mmw_batch_round_env: mmw_batch_round (sdp_solver.py:18-107) of the batch's resident factors against the state the environment
 * holds instead of the one the batch was built from -- the reference's alg.rounding(Z_fin, gX, e.generate_S_Q_hmax()) after
 * e.step_time (sim_mmw_online.py:43-47).  The factor, the Philox draws (mmw_batch_round_randv stays valid) and the greedy pass are
 * mmw_batch_round's; take / seeds / z_out / rem_out / used_out as there.  The environment must hold as many instances as the batch,
 * on the same device; a taking instance whose K differs between the two is refused by name with MMW_ERR_ARG.  Nothing of the
 * batch changes: the arenas, the resident factors and every mmw_batch_read_* field stay bitwise as they were.
 */
typedef struct mmw_batch_env mmw_batch_env;
int mmw_batch_env_create(mmw_batch_env** out, int device, int32_t B, const int32_t* K, const int32_t* A, const double* const* ap_xy,
                         double fre_Hz, double txp_offset, double min_s_n_ratio, double min_sinr, double noise_floor_dbm);
int mmw_batch_env_destroy(mmw_batch_env* e);
int mmw_batch_env_move(mmw_batch_env* e, const double* const* sta_xy);
int mmw_batch_env_sizes(mmw_batch_env* e, int32_t inst, int64_t out[4]);
int mmw_batch_env_state(mmw_batch_env* e, int32_t inst, int32_t* S_indptr, int32_t* S_indices, double* S_data, int32_t* Q_indptr,
                        int32_t* Q_indices, double* Q_data, double* h_max);
int mmw_batch_env_evaluate(mmw_batch_env* e, const double* const* z_vec, const int32_t* Z, double packet_bit, double bandwidth,
                           double slot_time, double* const* sinr_out, double* const* bler_out);
int mmw_batch_round_env(mmw_batch* b, mmw_batch_env* e, const int32_t* take, int32_t nattempt, int stop_at_first,
                        const uint64_t* seeds, int32_t* z_out, int32_t* rem_out, int32_t* used_out);
/* The batch for the states an environment holds, built on the device (csrc/kernels_batch_pattern.h, csrc/batch_from_env.h): B = the
 * environment's instances, on its device, on the state of its last move.  It is the batch mmw_batch_create makes from the arrays
 * mmw_batch_env_state hands out for every instance at the same Z[b], rank_radio, eta and nit[b]: mmw_batch_sizes, every
 * mmw_batch_read_i32 list and every mmw_batch_read_f64 field are equal bit for bit, and so is everything computed from them.
 * Creation is a count pass, ONE readback for all instances (the sizes, l_indptr, S_sum, the squared row sums, h_max), norm_H and cH
 * on the host (they depend on Z), one upload, the fill pass and one launch for the initial point: no per-instance copy and no host
 * pass over stored entries.  The batch copies the state's lists device to device and keeps no reference to the environment, which
 * may move or be destroyed at once.  The host lists behind mmw_batch_read_i32 (but MMW_I_L_INDPTR), MMW_F_ST_DATA, mmw_batch_export
 * and mmw_batch_carry(_map) are fetched per instance the first time an entry needs them, from that copy (MMW_F_BUILD_INFO says
 * whether that has happened); the first mmw_batch_gm fetches Q of every instance for its clique decision and completes no list.
 * Refused by instance, *out untouched: an environment that has not moved (MMW_ERR_STATE); nit[b] < 1, K < 2, a Z[b] that
 * mmw_batch_set_slots refuses and the batch limits of mmw_batch_create, in its words (MMW_ERR_ARG).  Z, D and K are checked before
 * anything is allocated; nnzL, the arena size and norm_H after the count pass, before the arenas are made.  There is no host-only
 * form. */
int mmw_batch_create_from_env(mmw_batch** out, mmw_batch_env* env, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit);
/* The batch for B CSR states that lie on the device (mmw_csr), built there, one workgroup per instance
 * (csrc/kernels_batch_csr_pattern.h, csrc/batch_from_csr.h): mmw._process_state and the prologue of mmw._run
 * (sim_src/alg/mmw.py:26-60) per instance, without a host copy of any state.  All csr[b] lie on one device and the batch is made
 * there; the same mmw_csr may appear more than once.  It is the batch mmw_batch_create makes from the arrays mmw_csr_state hands out
 * for every csr[b] at the same Z[b], rank_radio, eta and nit[b]: mmw_batch_sizes, every mmw_batch_read_i32 list and every
 * mmw_batch_read_f64 field are equal bit for bit, and so is everything computed from them.
 * Round trips, none of which depends on B: one upload (the per-instance table of the seven pointers and sizes), the count launch,
 * which validates every instance itself, ONE readback for all instances (the verdicts, the sizes, l_indptr, S_sum, the squared row
 * sums, h_max), norm_H and cH on the host (they depend on Z), one upload, the fill launch and one launch for the initial point.
 * The batch copies the state's lists device to device and keeps no reference to any mmw_csr: each may be destroyed as soon as the
 * call returns, and the arrays behind a wrapped one may be freed.  The host lists behind mmw_batch_read_i32 (but MMW_I_L_INDPTR),
 * MMW_F_ST_DATA, mmw_batch_export and mmw_batch_carry(_map) are fetched per instance the first time an entry needs them, from that
 * copy (MMW_F_BUILD_INFO: {1, 0 then 1}); the first mmw_batch_gm fetches Q of every instance for its clique decision.
 * If every csr[b] is host-only (device -1) the result is the host-only batch mmw_batch_create(device = -1) makes from the same
 * arrays, after the same per-row checks.
 * Refused, *out untouched:
 *   before anything is allocated or launched, MMW_ERR_ARG: B < 1, a NULL csr[b], host-only states mixed with states on a device,
 *     states on different devices, nit[b] < 1, K < 2, Z[b] < 2, K or D over the batch limits of mmw_batch_create, in its words;
 *   a malformed state, MMW_ERR_ARG "mmw_batch_create_from_csr: instance b: " and mmw_create's words for it (the checks are
 *     mmw_create_from_csr's, run inside the count launch: an instance whose check failed writes nothing that depends on its
 *     columns); the lowest failing instance is the one reported;
 *   after the count pass, before the arenas are made, MMW_ERR_ARG: nnzL or the arena size over the limits, a zero norm_H. */
int mmw_batch_create_from_csr(mmw_batch** out, int32_t B, mmw_csr* const* csr, const int32_t* Z, int32_t rank_radio, double eta,
                              const int32_t* nit);
/* mmw_batch_gm on the state of the environment's last move: see there */
int mmw_batch_env_gm(mmw_batch_env* e, int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out,
                     int32_t* zz_out, int32_t* rem_out, double* key_out);
/* mmw_batch_gm_rand on the state of the environment's last move: see there (MMW_ERR_STATE before the first move) */
int mmw_batch_env_gm_rand(mmw_batch_env* e, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first,
                          const uint64_t* seeds, int32_t* z_out, int32_t* rem_out, int32_t* used_out);

#ifdef __cplusplus
}
#endif
#endif /* MMW_HIP_H */
