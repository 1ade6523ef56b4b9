// The device-resident MMW solver behind the C ABI: `mmw_solver` is the opaque handle, `Solver<T>` its fp32 / fp64 body (unnamed namespace: mmw_api.hip includes this once).
#pragma once
#include <cstring>
#include <memory>
#include <atomic>
#include <thread>

#include "block_tables.h"
#include "chunk_policy.h"
#include "dev_reports.h"
#include "env_device.h"
#include "kernels_gm.h"
#include "pattern_device.h"
#include "solver_extras.h"

using namespace mmw;

struct mmw_env {
    mmw::EnvDevice e;
};
struct mmw_solver {
    virtual ~mmw_solver() {}
    virtual int sizes(int64_t out[10]) = 0;
    virtual int set_expm(int method, int max_order, double tol) = 0;
    virtual int set_timing(int enabled) = 0;
    virtual int set_profile(int enabled) = 0;
    virtual int bench_spmm(int blocked, int reps, double* avg_us) = 0;
    virtual int reset(int32_t nit) = 0;
    virtual int set_slots(int32_t Z, int32_t nit, int warm) = 0;
    virtual int set_eta(double eta) = 0;
    virtual int iterate(int32_t n, const double* randv, uint64_t seed) = 0;
    virtual int sync() = 0;
    virtual int sketch(uint64_t seed, int32_t iteration, double* out, int64_t n) = 0;
    virtual int read_f64(int which, double* out, int64_t n) = 0;
    virtual int read_i32(int which, int32_t* out, int64_t n) = 0;
    virtual int gap(double out[3]) = 0;
    virtual int factor(int32_t rank, double* out, uint64_t seed) = 0;
    virtual int round(int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out,
                      int32_t* rem_out) = 0;
};
namespace {
// the two refusals of a handle made with device -1
inline int host_only_handle() { return fail(MMW_ERR_STATE, "host-only handle"); }
inline int host_only_pattern() { return fail(MMW_ERR_STATE, "this handle was created with device -1 (host pattern only)"); }
template <typename T> struct Solver final : mmw_solver {
    const Switches sw;  // read once by mmw_create / mmw_create_from_env (switches.h); everything below this handle gets a reference
    explicit Solver(const Switches& s) : sw(s), eng(sw), extras(sw) {}
    int device = 0;
    bool host_only = false;
    hipStream_t st = nullptr;
    HostPattern H;
    int K = 0, Z = 0, D = 0, rank_radio = 2, nit = 0, iter = 0;
    double eta = 0.1;
    bool kt_shipped = false;  // set_profile(2)
    bool kt_exact() const { return kt.on && !kt_shipped; }  // set_profile(1): synchronous plans, every kernel class in launches of its own
    // pattern on the device
    DevBuf<int> d_indptr, d_col, d_pid, d_mirror, d_diag, d_apos, d_lrow;
    DevBuf<T> d_sab, d_sba, d_h, d_ssum, d_invn, d_cH;
    // iterate state
    DevBuf<T> lval, xval, xavg, Y, yavg, e_accu, e_this, rsum, Xh, drow;
    DevBuf<double> max_part, sum_part, scal, tr_part, stage64, out64;
    DevBuf<T> wH;  // Y_H / norm_H
    DevBuf<T> yun;  // the fused DUAL pass's unnormalised exponentials (see iterate_impl)
    // how far e_accu's maximum may run ahead of the fused pass's shift before its exponentials are distrusted (exp overflows T
    // near 88 / 709); MMW_DUAL_GAP is for the tests, which force the replay with it
    const double dual_gap = std::isnan(sw.dual_gap) ? (sizeof(T) == 4 ? 60.0 : 600.0) : sw.dual_gap;
    static constexpr int LOSS_GRID_MAX = 4096;
    BlockTables<T> bt;  // the locality blockings: host tables, device tables, kernel argument structs (block_tables.h)
    int64_t sketch_done_for = -1;  // iteration whose sketch the last SDDMM launch already drew into the start block
    uint64_t sketch_done_seed = 0;
    int sketch_done_slabs = 0;
    bool lblk_stale = false;         // bt.lval_blk lags lval (the matrix-core kernel ran the last products)
    DevBuf<ExpmPlan> sn_plan;        // plan (with its history) at the start of the pending chunk
    // X in the matrix-core SDDMM's tile order (kernels_mfma.h): xs_val / xs_avg hold X and its running sum while x_tiles is set, the
    // CSR-ordered xval / xavg otherwise (bt.b_e2w maps a CSR entry to its slot)
    DevBuf<T> xs_val, xs_avg;
    bool x_tiles = false;   // which pair of buffers holds the iterate's X
    bool sn_tiles = false;  // ... and which the pending chunk's snapshot was taken from
    DevBuf<unsigned short> xh_planes;
    DevBuf<long long> rsfx;  // [2K] 2^-40 fixed-point totals: [0, K) row sums of the off-diagonal X, left by the matrix-core SDDMM; [K, 2K) row norms of
                             // y = exp(L/2)R from the first-order product (kernels_mfma.h).  Zeroed by every LOSS pass.
    DevBuf<double> tr1_part; // trace shares of the first-order product's workgroups (zero where none works)
    // the rounding of the first-order product's fp16 plane: measured by the sketch kernel (default), or the format's worst case
    const bool fv_measure = !sw.fv_worstcase;
    double plane_rounding() const { return fv_measure ? F16_PLANE_EXPECT : 1.02 * F16_UNIT; }
    long long n_first16_iters = 0;
    ChunkPolicy pol;  // the run's planning history and the next chunk's guesses (chunk_policy.h)
    long long n_first_iters = 0;
    bool rs_last = false;    // the last iteration enqueued left rsfx for the X the next one starts from
    const bool rs_enabled = !sw.no_sddmm_rowsums;
    long long n_rs_iters = 0, n_fused_iters = 0;  // MMW_F_DUAL_INFO
    int blocking_mode = 1;  // 1: use when profitable, 0: never
    // optimistic (no per-iteration readback) batches: snapshot for the rare replay
    DevBuf<T> sn_lval, sn_xval, sn_xavg, sn_Y, sn_yavg, sn_eaccu;
    bool pending = false;
    int pend_iter0 = 0, pend_n = 0;
    size_t pend_events0 = 0;  // phase-timer events recorded before the pending chunk (PhaseTimers::mark)
    uint64_t pend_seed = 0;
    DevBuf<double> emax_d;
    double emax_h = 0.0;
    int emax_enq_iter = -1, emax_iter = -1;  // iteration count the enqueued / fetched maximum violation belongs to
    ExpmEngine<T> eng;
    Extras<T> extras;
    KernelTimers kt;
    PhaseTimers pt;
    uint64_t last_seed = 0;
    bool last_was_rng = false;
    ~Solver() override {
        bt.join();  // the build thread works on this handle's members
        if (host_only) return;
        (void)hipSetDevice(device);
        if (st) (void)hipStreamDestroy(st);
    }
    int upload_slot_scalars() {  // the two row vectors that follow the slot count: 1 / norm_H and cH
        std::vector<double> invn(K);
        for (int k = 0; k < K; ++k) invn[k] = 1.0 / H.norm_H[k];
        MMW_TRY(d_invn.upload_cast(invn, st));
        return d_cH.upload_cast(H.cH, st);
    }
    PatternDev<T> pat() const {
        PatternDev<T> P;
        P.K = K; P.Z = Z; P.E_asso = (int)H.E_asso(); P.C = (int)H.C(); P.nnzL = (int)H.nnzL();
        P.indptr = d_indptr.p; P.col = d_col.p; P.pid = d_pid.p; P.mirror = d_mirror.p; P.diag_pos = d_diag.p;
        P.asso_pos = d_apos.p; P.sab = d_sab.p; P.sba = d_sba.p; P.h_max = d_h.p; P.S_sum = d_ssum.p;
        P.inv_norm_H = d_invn.p; P.cH = d_cH.p;
        if (x_tiles) { P.e2w = bt.b_e2w.p; P.xasso = bt.b_xasso.p; P.xdiag_base = (int)bt.HB.m_nedges; }
        return P;
    }
    int init(int dev, int32_t K_, int32_t Z_, int32_t rr, double eta_, int32_t nit_, const int32_t* Sp, const int32_t* Si,
             const double* Sx, const int32_t* Qp, const int32_t* Qi, const double* Qx, const double* h) {
        device = dev;
        const double t_0 = tnow();
        // The first kernel launch of a process loads the library's code object (~0.15 s): start it on a helper thread now, under
        // the host-side pattern build.
        static std::atomic<bool> module_loading{false};
        std::thread warm_thread;
        if (!host_only && !module_loading.exchange(true))
            warm_thread = std::thread([dev]() {
                if (hipSetDevice(dev) != hipSuccess) return;
                float* p = nullptr;
                if (hipMalloc((void**)&p, 256 * sizeof(float)) != hipSuccess) return;
                hipLaunchKernelGGL((k_fill<float>), dim3(1), dim3(BLOCK), 0, (hipStream_t) nullptr, (size_t)256, p, 0.0f);
                (void)hipDeviceSynchronize();
                (void)hipFree(p);
            });
        struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{warm_thread};
        bt.want_mfma(K_, Z_ * rr, sw);
        const bool start_blk = !host_only && !sw.no_blocking;
        double t_struct = 0.0;
        std::string err = build_pattern(H, K_, Z_, Sp, Si, Sx, Qp, Qi, Qx, h, [&]() {
            t_struct = tnow();
            if (start_blk) bt.build_thread = std::thread([this]() { bt.host_blockings(H, sw); });
        });
        if (!err.empty()) bt.join();
        const double t_1 = tnow();
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_create: " + err);
        K = K_; Z = Z_; rank_radio = rr; eta = eta_; nit = nit_;
        D = Z * rank_radio;
        if (host_only) {  // device == -1: pattern inspection only (CPU tests of the host logic)
            std::string lerr;
            if (make_layout(D, V16<T>::N, eng.lay, lerr) != MMW_OK) return fail(MMW_ERR_ARG, lerr);
            if (live_switch(LIVE_HOST_BLOCKING)) {  // developer aid: build the locality blocking on the host and print its statistics
                report_host_blocking(bt.HB, H, K, blocking_limits<T>(), sw);
            }
            if (sw.check_blocking) {  // CPU tests: build the blocking and check its invariants
                const BlockingLimits lim = blocking_limits<T>();
                if (bt.HB.order.empty()) build_blocking(bt.HB, K, H.l_indptr, H.l_indices, lim);
                build_sd_tables(bt.HB, K, H.l_indptr, H.l_indices);
                if (!bt.HB.order.empty() && !bt.HB.blk_rowptr.empty() && bt.HB.blk_rowptr.back() == K) {
                    const std::string berr = verify_blocking(bt.HB, K, H.l_indptr, H.l_indices, lim);
                    if (!berr.empty()) return fail(MMW_ERR_STATE, "blocking invariant violated: " + berr);
                    for (int mrows : {64, 32, 7}) {
                        build_mfma_blocking(bt.HB, K, H.l_indptr, H.l_indices, mrows, sw.mf_union_cap);
                        const std::string merr = verify_mfma_blocking(bt.HB, K, H.l_indptr, H.l_indices);
                        if (!merr.empty()) return fail(MMW_ERR_STATE, "blocking invariant violated: " + merr);
                    }
                }
            }
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        MMW_TRY(d_indptr.upload(H.l_indptr, st));
        MMW_TRY(d_col.upload(H.l_indices, st));
        MMW_TRY(d_pid.upload(H.pid, st));
        MMW_TRY(d_mirror.upload(H.mirror, st));
        MMW_TRY(d_diag.upload(H.diag_pos, st));
        MMW_TRY(d_apos.upload(H.asso_pos, st));
        {
            std::vector<int32_t> lrow((size_t)H.nnzL());
            for (int k = 0; k < K; ++k)
                for (int e = H.l_indptr[k]; e < H.l_indptr[k + 1]; ++e) lrow[e] = k;
            MMW_TRY(d_lrow.upload(lrow, st));
        }
        MMW_TRY(d_sab.upload_cast(H.sab, st));
        MMW_TRY(d_sba.upload_cast(H.sba, st));
        MMW_TRY(d_h.upload_cast(H.h_max, st));
        MMW_TRY(d_ssum.upload_cast(H.S_sum, st));
        MMW_TRY(upload_slot_scalars());
        return init_common(t_0, t_1, t_struct, /*env=*/nullptr);
    }
    // ---- mmw_create_from_env: the state never leaves the device.  The generator's receive powers are turned into the pattern, its
    // per-entry arrays, the edge lists and the row statistics by the kernels of pattern_device.h; the host gets the row pointers (from
    // the count pass's prefix sums), the column indices (the blockings read them) and three K-vectors.  The lists that only the
    // API's read fields hand out stay on the device until asked for (ensure_host_lists).
    struct EnvLists {  // device copies kept for ensure_host_lists
        DevBuf<int> st_ptr, st_idx, gain_x, gain_y, asso_x, asso_y, gu_ptr, qu_ptr, so_ptr;
        DevBuf<double> st_val, s_sum, sq_sum;
        bool host_done = true;  // false: H's list vectors are still empty
    } envl;
    int ensure_host_lists() {
        if (envl.host_done) return MMW_OK;
        MMW_HIP(hipSetDevice(device));
        const size_t nst = (size_t)H.n_st, ng = (size_t)H.n_gain, na = (size_t)H.n_asso;
        H.st_indices.resize(nst); H.st_data.resize(nst);
        H.gain_x.resize(ng); H.gain_y.resize(ng); H.asso_x.resize(na); H.asso_y.resize(na);
        H.diag_pos.resize(K); H.asso_pos.resize(na);
        MMW_TRY(copy_d2h(H.st_indices.data(), envl.st_idx.p, nst * sizeof(int32_t), st));
        MMW_TRY(copy_d2h(H.st_data.data(), envl.st_val.p, nst * sizeof(double), st));
        MMW_TRY(copy_d2h(H.gain_x.data(), envl.gain_x.p, ng * sizeof(int32_t), st));
        MMW_TRY(copy_d2h(H.gain_y.data(), envl.gain_y.p, ng * sizeof(int32_t), st));
        MMW_TRY(copy_d2h(H.asso_x.data(), envl.asso_x.p, na * sizeof(int32_t), st));
        MMW_TRY(copy_d2h(H.asso_y.data(), envl.asso_y.p, na * sizeof(int32_t), st));
        MMW_TRY(copy_d2h(H.diag_pos.data(), d_diag.p, (size_t)K * sizeof(int32_t), st));
        MMW_TRY(copy_d2h(H.asso_pos.data(), d_apos.p, na * sizeof(int32_t), st));
        envl.host_done = true;
        return MMW_OK;
    }
    // Row order of a geometric instance: boustrophedon strips about one block wide (blocking.h: consecutive runs of it are compact patches)
    static std::vector<int32_t> spatial_order(int K, const std::vector<double>& xy, int rows_per_block) {
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
        for (int k = 0; k < K; ++k) {
            x0 = std::min(x0, xy[2 * k]); x1 = std::max(x1, xy[2 * k]);
            y0 = std::min(y0, xy[2 * k + 1]); y1 = std::max(y1, xy[2 * k + 1]);
        }
        const double area = std::max((x1 - x0) * (y1 - y0), 1e-300);
        const double w = std::max(std::sqrt(area * (double)rows_per_block / (double)std::max(K, 1)) * 0.9, 1e-300);  // a block is ~ w x w
        std::vector<std::pair<std::pair<int64_t, double>, int32_t>> key(K);
        for (int k = 0; k < K; ++k) {
            const int64_t strip = (int64_t)((xy[2 * k] - x0) / w);
            key[k] = {{strip, (strip & 1) ? -xy[2 * k + 1] : xy[2 * k + 1]}, k};
        }
        std::sort(key.begin(), key.end());
        std::vector<int32_t> ord(K);
        for (int k = 0; k < K; ++k) ord[k] = key[k].second;
        return ord;
    }
    EnvDevice* env_src = nullptr;  // during init_env only
    int init_env(int dev, EnvDevice& E, int32_t Z_, int32_t rr, double eta_, int32_t nit_) {
        device = dev;
        const double t_0 = tnow();
        if (Z_ < 2) return fail(MMW_ERR_ARG, "mmw_create_from_env: Z must be >= 2 (the constraints divide by Z-1)");
        if (E.K < 2) return fail(MMW_ERR_ARG, "mmw_create_from_env: K must be >= 2");
        MMW_HIP(hipSetDevice(device));
        MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        MMW_TRY(E.pattern_inputs());  // (cached in the generator: rxT, positions in the AP lists, the count pass)
        K = E.K; Z = Z_; rank_radio = rr; eta = eta_; nit = nit_;
        D = Z * rank_radio;
        H.K = K; H.Z = Z;
        const int A = E.A;
        const int32_t* c6 = E.h_cnt6.data();
        // prefix sums of the count pass
        std::vector<int32_t> st_ptr(K + 1, 0), gu_ptr(K + 1, 0), qu_ptr(K + 1, 0), so_ptr(K + 1, 0);
        H.l_indptr.assign(K + 1, 0);
        for (int k = 0; k < K; ++k) {
            H.l_indptr[k + 1] = H.l_indptr[k] + c6[k];
            st_ptr[k + 1] = st_ptr[k] + c6[(size_t)K + k];
            gu_ptr[k + 1] = gu_ptr[k] + c6[(size_t)2 * K + k];
            qu_ptr[k + 1] = qu_ptr[k] + c6[(size_t)3 * K + k];
            so_ptr[k + 1] = so_ptr[k] + (E.h_sptr[k + 1] - E.h_sptr[k]) - c6[(size_t)4 * K + k];
            if ((int64_t)H.l_indptr[k] + c6[k] > (int64_t)INT32_MAX) return fail(MMW_ERR_ARG, "mmw_create_from_env: pattern too large for int32 indexing");
        }
        const size_t nnz = (size_t)H.l_indptr[K], nst = (size_t)st_ptr[K], ng = (size_t)gu_ptr[K], na = (size_t)qu_ptr[K];
        H.n_st = (int64_t)nst; H.n_gain = (int64_t)ng; H.n_asso = (int64_t)na;
        H.st_indptr = st_ptr;
        MMW_TRY(d_indptr.upload(H.l_indptr, st));
        MMW_TRY(envl.st_ptr.upload(st_ptr, st)); MMW_TRY(envl.gu_ptr.upload(gu_ptr, st)); MMW_TRY(envl.qu_ptr.upload(qu_ptr, st)); MMW_TRY(envl.so_ptr.upload(so_ptr, st));
        MMW_TRY(d_col.alloc(nnz)); MMW_TRY(d_lrow.alloc(nnz)); MMW_TRY(d_sab.alloc(nnz)); MMW_TRY(d_sba.alloc(nnz)); MMW_TRY(d_pid.alloc(nnz)); MMW_TRY(d_mirror.alloc(nnz));
        MMW_TRY(d_diag.alloc(K)); MMW_TRY(d_apos.alloc(na));
        MMW_TRY(envl.st_idx.alloc(nst)); MMW_TRY(envl.st_val.alloc(nst));
        MMW_TRY(envl.gain_x.alloc(ng)); MMW_TRY(envl.gain_y.alloc(ng)); MMW_TRY(envl.asso_x.alloc(na)); MMW_TRY(envl.asso_y.alloc(na));
        MMW_TRY(envl.s_sum.alloc(K)); MMW_TRY(envl.sq_sum.alloc(K));
        PatOut<T> O;
        O.l_ptr = d_indptr.p; O.st_ptr = envl.st_ptr.p; O.gu_ptr = envl.gu_ptr.p; O.qu_ptr = envl.qu_ptr.p; O.appos = E.appos.p;
        O.l_idx = d_col.p; O.lrow = d_lrow.p; O.sab = d_sab.p; O.sba = d_sba.p; O.pid = d_pid.p; O.diag_pos = d_diag.p;
        O.st_idx = envl.st_idx.p; O.st_val = envl.st_val.p;
        O.gain_x = envl.gain_x.p; O.gain_y = envl.gain_y.p; O.asso_x = envl.asso_x.p; O.asso_y = envl.asso_y.p; O.asso_pos = d_apos.p;
        hipLaunchKernelGGL((k_pat_fill<T>), dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, A, E.P.thr, E.rx.p, E.rxT.p, E.asso.p, O);
        MMW_HIP(hipGetLastError());
        // the column indices first: the host-side blockings start on them while the device finishes the rest
        H.l_indices.resize(nnz);
        MMW_TRY(copy_d2h(H.l_indices.data(), d_col.p, nnz * sizeof(int32_t), st));
        const double t_struct = tnow();
        bt.want_mfma(K, Z_ * rr, sw);
        if (!sw.no_blocking) {
            if (!sw.env_rcm) {  // (MMW_ENV_RCM=1: the pattern-only order of the CSR entry point, for comparisons)
                bt.HB.rcm_cache = spatial_order(K, E.h_sta, 64);
                bt.HB.grow = false;
            }
            bt.build_thread = std::thread([this]() { bt.host_blockings(H, sw); });
        }
        hipLaunchKernelGGL(k_pat_mirror, dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, d_indptr.p, d_col.p, d_lrow.p, d_mirror.p);
        hipLaunchKernelGGL(k_pat_rowstats, dim3(grid_elems((size_t)K)), dim3(BLOCK), 0, st, K, envl.st_ptr.p, envl.st_val.p, envl.s_sum.p, envl.sq_sum.p);
        MMW_HIP(hipGetLastError());
        H.S_sum.resize(K); H.sq_sum.resize(K); H.h_max.resize(K);
        MMW_TRY(copy_d2h(H.S_sum.data(), envl.s_sum.p, (size_t)K * sizeof(double), st));
        MMW_TRY(copy_d2h(H.sq_sum.data(), envl.sq_sum.p, (size_t)K * sizeof(double), st));
        MMW_TRY(copy_d2h(H.h_max.data(), E.h_max.p, (size_t)K * sizeof(double), st));
        H.norm_H.assign(K, 0.0);
        H.cH.assign(K, 0.0);
        {
            const std::string err = update_slots(H, Z);
            if (!err.empty()) {
                bt.join();
                return fail(MMW_ERR_ARG, "mmw_create_from_env: " + err);
            }
        }
        MMW_TRY(d_h.upload_cast(H.h_max, st));
        MMW_TRY(d_ssum.upload_cast(H.S_sum, st));
        MMW_TRY(upload_slot_scalars());
        envl.host_done = false;
        const double t_1 = tnow();
        env_src = &E;
        const int rc = init_common(t_0, t_1, t_struct, &E);
        env_src = nullptr;
        return rc;
    }
    // the rounding's view of the state, from the generator's own CSR of S_gain (diagonal dropped) and Q
    int init_extras_env(EnvDevice& E) {
        MMW_TRY(extras.init_device(st, K, &kt));
        std::vector<int32_t> so_ptr_h((size_t)K + 1);
        MMW_TRY(copy_d2h(so_ptr_h.data(), envl.so_ptr.p, so_ptr_h.size() * sizeof(int32_t), st));
        const size_t nso = (size_t)so_ptr_h[K];
        MMW_TRY(extras.so_indptr.upload(so_ptr_h, st));
        MMW_TRY(extras.so_indices.alloc(nso)); MMW_TRY(extras.so_data.alloc(nso)); MMW_TRY(extras.so_hmax.alloc(nso));
        MMW_TRY(extras.q_indptr.alloc((size_t)K + 1)); MMW_TRY(extras.q_indices.alloc((size_t)E.nnzQ)); MMW_TRY(extras.h_max.alloc(K));
        hipLaunchKernelGGL(k_pat_so_fill, dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, (const int*)E.s_ptr.p, (const int*)E.s_idx.p, (const double*)E.s_val.p,
                           (const int*)extras.so_indptr.p, (const double*)E.h_max.p, extras.so_indices.p, extras.so_data.p, extras.so_hmax.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipMemcpyAsync(extras.q_indptr.p, E.q_ptr.p, ((size_t)K + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
        MMW_HIP(hipMemcpyAsync(extras.q_indices.p, E.q_idx.p, (size_t)E.nnzQ * sizeof(int), hipMemcpyDeviceToDevice, st));
        MMW_HIP(hipMemcpyAsync(extras.h_max.p, E.h_max.p, (size_t)K * sizeof(double), hipMemcpyDeviceToDevice, st));
        MMW_HIP(hipStreamSynchronize(st));
        return MMW_OK;
    }
    // ---- everything after the pattern is on the device: the iterate's buffers, the engine, the blockings, the rounding side
    int init_common(double t_0, double t_1, double t_struct, EnvDevice* env) {
        const bool verbose = live_switch(LIVE_VERBOSE);
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        MMW_TRY(lval.alloc(nnz)); MMW_TRY(xval.alloc(nnz)); MMW_TRY(xavg.alloc(nnz));
        MMW_TRY(Y.alloc(C)); MMW_TRY(yavg.alloc(C)); MMW_TRY(e_accu.alloc(C)); MMW_TRY(e_this.alloc(C));
        MMW_TRY(rsum.alloc(K)); MMW_TRY(drow.alloc(K));
        MMW_TRY(max_part.alloc(ROW_GRID_MAX)); MMW_TRY(sum_part.alloc(4 * (size_t)std::max(2048, ROW_GRID_MAX))); MMW_TRY(scal.alloc(8));
        MMW_TRY(tr_part.alloc(ROW_GRID_MAX)); MMW_TRY(wH.alloc(K));
        MMW_TRY(eng.init(st, K, D, d_indptr.p, d_col.p, lval.p));
        kt.st = st;
        eng.kt = &kt;
        eng.max_order = 12;
        eng.tol = sizeof(T) == 4 ? 1e-6 : 1e-9;
        MMW_TRY(Xh.alloc(eng.bs));
        MMW_TRY(prealloc());
        const double t_2 = tnow();
        MMW_TRY(setup_blocking());
        const double t_3 = tnow();
        if (verbose) fprintf(stderr, "[create] pattern %.1f ms (structure after %.1f), uploads+alloc %.1f ms, blocking %.1f ms\n", (t_1 - t_0) * 1e3, (t_struct - t_0) * 1e3, (t_2 - t_1) * 1e3, (t_3 - t_2) * 1e3);
        size_t big = std::max(std::max(nnz, C), eng.bs);
        MMW_TRY(out64.alloc(big));
        MMW_TRY(stage64.alloc((size_t)K * D));
        MMW_HIP(hipStreamSynchronize(st));
        if (env) MMW_TRY(init_extras_env(*env));
        else MMW_TRY(extras.init(this->st, &H, K, &kt));
        return reset(nit);
    }
    BlkDev blkdev() const { return bt.blkdev(K, eng.lay.Dpad, sw.full_tile); }
    // Buffers the loop, the factor and the rounding would otherwise allocate on first use (hipMalloc is a synchronous driver call
    // of 0.1 - 3 ms, and the first probe of a search pays all of them inside its timed phases): reserved here, while the
    // blocking thread is still at work and this thread would only wait for it.
    int prealloc() {
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        for (DevBuf<T>* b : {&sn_lval, &sn_xval, &sn_xavg}) MMW_TRY(b->alloc(nnz));
        for (DevBuf<T>* b : {&sn_Y, &sn_yavg, &sn_eaccu, &yun}) MMW_TRY(b->alloc(C));
        MMW_TRY(sn_plan.alloc(1));
        // Krylov basis: the first iterations of a run ask for 2 - 3 steps before the a-posteriori estimate settles on fewer; growing
        // the basis there costs an allocation, a copy and two device synchronisations each time
        if ((double)eng.bs * sizeof(T) * 4.0 < 8.0e9) MMW_TRY(eng.ensure_blocks(std::min(4, eng.max_order + 1)));
        if (bt.blk_want_mf && (eng.lay.Dpad % 32) == 0) {
            MMW_TRY(xh_planes.alloc(2 * eng.bs));
            MMW_TRY(eng.reserve_planes());
        }
        const int rank = std::min(K - 1, (Z - 1) * rank_radio);  // what the host class asks mmw_factor for (mmw.py:206)
        if (rank >= 1) {
            MMW_TRY(extras.fac_reserve(st, K, rank, bt.blk_want_mf));
            if ((size_t)10 * K * Z * sizeof(double) <= ((size_t)2 << 30)) MMW_TRY(extras.round_reserve(K, Z, rank, 10));  // sdp_solver.rounding's 10 attempts
        }
        return MMW_OK;
    }
    int setup_blocking() {
        if (sw.no_blocking) blocking_mode = 0;
        if (!blocking_mode) return MMW_OK;
        if (bt.build_thread.joinable()) bt.build_thread.join();  // started under the pattern build (init)
        else bt.host_blockings(H, sw);
        if (bt.blk_want_mf && live_switch(LIVE_VERBOSE))
            fprintf(stderr, "[mmw] matrix-core blocking: ok %d blocks %d rows/block %.1f reuse %.2f row tiles %d k-steps %d\n", (int)bt.HB.fits_mfma, bt.HB.nbm(),
                    (double)K / std::max(1, bt.HB.nbm()), bt.HB.m_reuse, bt.HB.mfma_mt, bt.HB.kbase.empty() ? 0 : bt.HB.kbase.back());
        if (live_switch(LIVE_VERBOSE))
            fprintf(stderr, "[mmw] blocking: usable %d half-tile %d blocks %d rows/block %.1f union/block %.1f entries %lld (nnz %lld, +%.1f%% padding) sd_max %d\n",
                    (int)bt.HB.usable, (int)bt.HB.fits_half_tile, bt.HB.nb(), (double)K / std::max(1, bt.HB.nb()), (double)bt.HB.un_cols.size() / std::max(1, bt.HB.nb()),
                    (long long)bt.HB.nent, (long long)H.nnzL(), 100.0 * ((double)bt.HB.nent / (double)H.nnzL() - 1.0), bt.HB.sd_max);
        if (!bt.HB.usable) return MMW_OK;
        MMW_TRY(bt.upload(st, H, K, sw, d_apos.p));
        if (sizeof(T) == 4 && bt.HB.fits_mfma) {
            eng.use_mfma = true;
            eng.mf.nb = bt.HB.nbm();
            eng.mf.desc = bt.b_mdesc.p;
            eng.mf.un_fixed = bt.b_munfixed.p;
            eng.mf.order = bt.b_morder.p;
            eng.mf.kbase = bt.b_kbase.p;
            eng.mf.afrag = bt.afrag.p;
            eng.mf_mt = bt.HB.mfma_mt;
            if (bt.sddmm_mfma) {  // X in tile order and the fixed-point row totals, for the matrix-core SDDMM
                MMW_TRY(xs_val.alloc(bt.n_xs));
                MMW_TRY(xs_avg.alloc(bt.n_xs));
                MMW_TRY(rsfx.alloc((size_t)2 * K));
            }
            if ((size_t)bt.HB.nbm() > (size_t)MAX_PART && bt.HB.nbm() > bt.HB.nb()) {
                MMW_TRY(eng.partial.alloc((size_t)bt.HB.nbm() * eng.lay.Dpad));
                MMW_TRY(eng.partial_o2.alloc((size_t)bt.HB.nbm() * eng.lay.Dpad));
            }
        }
        if (!bt.sddmm_mfma) MMW_TRY(bt.ensure_sd(st, H, K, eng.lay.Dpad, sw.full_tile));
        MMW_HIP(hipStreamSynchronize(st));
        extras.fac.set_blocking(blkdev(), bt.b_bepos.p, bt.HB.nent);
        if (eng.use_mfma) extras.fac.set_mfma(eng.mf, bt.HB.mfma_mt, bt.b_fpos.p, bt.afrag_n, (int64_t)H.nnzL());
        eng.blk_stale = &lblk_stale;
        eng.blk_refresh = [this]() -> int {
            hipLaunchKernelGGL((k_gather_blocked<T>), dim3(grid_elems((size_t)bt.HB.nent)), dim3(BLOCK), 0, st, (size_t)bt.HB.nent, bt.b_bepos.p, lval.p, bt.lval_blk.p);
            MMW_HIP(hipGetLastError());
            return MMW_OK;
        };
        return eng.enable_blocking(blkdev(), bt.lval_blk.p);
    }
    int sizes(int64_t out[10]) override {
        out[0] = K; out[1] = Z; out[2] = D; out[3] = eng.lay.Dpad; out[4] = H.nnzL(); out[5] = H.nnzST();
        out[6] = H.E_gain(); out[7] = H.E_asso(); out[8] = H.C(); out[9] = iter;
        return MMW_OK;
    }
    int set_expm(int method, int max_order, double tol) override {
        if (method != MMW_EXPM_LANCZOS && method != MMW_EXPM_TAYLOR) return fail(MMW_ERR_ARG, "unknown expm method");
        if (max_order < 1 || max_order > MAX_ORDER) return fail(MMW_ERR_ARG, "max_order must be in [1,16]");
        if (!(tol > 0)) return fail(MMW_ERR_ARG, "tol must be positive");
        eng.method = method; eng.max_order = max_order; eng.tol = tol;
        return MMW_OK;
    }
    int set_timing(int enabled) override {
        pt.timing = enabled != 0;
        pt.timing_stride = enabled > 1 ? enabled : 1;
        return MMW_OK;
    }
    // SpMM micro-benchmark on the current L values: Tm = 0.5 * L * start_block, `reps` launches
    int bench_spmm(int blocked, int reps, double* avg_us) override {
        if (host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(device));
        if (blocked && !bt.HB.usable) return fail(MMW_ERR_STATE, "no locality blocking for this pattern");
        MMW_TRY(sync());
        hipLaunchKernelGGL((k_sketch_rng<T>), dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, 99ull, 0u, eng.start_block(), (double*)nullptr);
        const bool keep = eng.use_blk, keep_mf = eng.use_mfma;
        eng.use_blk = blocked != 0;
        if (blocked == 2 && !eng.use_mfma) return fail(MMW_ERR_STATE, "no matrix-core SpMM for this handle (fp32, blocks of <= 32 rows)");
        eng.use_mfma = blocked == 2;
        StampBuf stamps;
        const bool want_stamps = blocked && live_switch(LIVE_STAMPS);
        MMW_TRY(stamps.request(want_stamps, (size_t)16 * 8192, st));
        hipEvent_t e0, e1;
        MMW_HIP(hipEventCreate(&e0));
        MMW_HIP(hipEventCreate(&e1));
        const bool lz = live_switch(LIVE_BENCH_LANCZOS);  // time the Lanczos epilogue (alpha partials) instead of the plain product
        const unsigned short* pl = nullptr;
        if (blocked == 2) {  // the planes are the producer's job: outside the timed launches
            eng.planes_ready[0] = false;
            MMW_TRY(eng.make_planes(0));
            pl = eng.planes_of(0);
        }
        // MMW_BENCH_FIRST: the first-order product as the loop launches it (fp16 operands and its whole epilogue; the operands are whatever the
        // last iteration left -- only the time is of interest)
        const bool fo = blocked == 2 && live_switch(LIVE_BENCH_FIRST) && sizeof(T) == 4 && rsfx.p != nullptr;
        int ntr1 = 0;
        if (fo) {
            if (xh_planes.n < 2 * eng.bs) MMW_TRY(xh_planes.alloc(2 * eng.bs));
            const size_t need = (size_t)eng.first_grid_max();
            if (tr1_part.n < need) {
                MMW_TRY(tr1_part.alloc(need));
                MMW_HIP(hipMemsetAsync(tr1_part.p, 0, need * sizeof(double), st));
            }
            hipLaunchKernelGGL(k_plane_f16, dim3(grid_elems(eng.bs / 4)), dim3(BLOCK), 0, st, eng.bs / 4, reinterpret_cast<const float4*>(eng.start_block()),
                               reinterpret_cast<uint2*>(eng.planes_of(0)));
        }
        auto one = [&]() {
            if (fo) {
                eng.planes_ready[0] = true;
                eng.planes0_f16 = true;
                return eng.apply_first((T*)nullptr, 0.5, 1, true, xh_planes.p, rsfx.p + K, tr1_part.p, &ntr1);
            }
            return lz ? eng.template launch_spmm<SPMM_LANCZOS>(eng.start_block(), eng.Tm.p, nullptr, 0.5, 0.0, 1.0, nullptr, 0, pl)
                      : eng.template launch_spmm<SPMM_PLAIN>(eng.start_block(), eng.Tm.p, nullptr, 0.5, 0.0, 1.0, nullptr, 0, pl);
        };
        int rc = one();  // warm
        MMW_HIP(hipEventRecord(e0, st));
        for (int r = 0; r < reps && rc == MMW_OK; ++r) rc = one();
        MMW_HIP(hipEventRecord(e1, st));
        MMW_HIP(hipStreamSynchronize(st));
        if (want_stamps) {  // one more launch that leaves its stamps (matrix-core kernel: per-wave phase clocks)
            unsigned long long*& slot = blocked == 2 ? g_mf_stamps : g_blk_stamps;
            slot = stamps.p();
            rc = one();
            slot = nullptr;
            MMW_TRY(blocked == 2 ? dump_mf_stamps(st, stamps.p()) : dump_stamps(st, stamps.p()));
        }
        eng.use_blk = keep;
        eng.use_mfma = keep_mf;
        float ms = 0;
        MMW_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (avg_us) *avg_us = ms * 1e3 / (reps > 0 ? reps : 1);
        return rc;
    }
    int set_profile(int enabled) override {
        if (host_only) return host_only_handle();
        MMW_TRY(sync());
        kt.on = enabled != 0;
        kt_shipped = enabled == 2;  // 2: time the launches of the shipped path (chunks without readback, riding workgroups) as they are
        kt.attach = kt_shipped && !sw.kt_markers;  // ... the matrix-core product by the events its launch carries itself
        eng.kt_exact = kt.on && !kt_shipped;
        kt.clear();
        return MMW_OK;
    }
    // same state, new slot count: only the Z-dependent scalars and the D-wide blocks change
    int set_eta(double eta_) override {
        if (!(eta_ >= 0.0)) return fail(MMW_ERR_ARG, "eta must be non-negative");
        if (!host_only) {
            MMW_HIP(hipSetDevice(device));
            MMW_TRY(settle());  // a pending chunk was enqueued with the old step size; a replay must use it too
        }
        eta = eta_;
        return MMW_OK;
    }
    int set_slots(int32_t Z_, int32_t nit_, int warm) override {
        if (host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(settle());
        MMW_HIP(hipStreamSynchronize(st));
        if (warm && iter == 0) warm = 0;  // nothing to continue from
        std::string err = update_slots(H, Z_);
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_set_slots: " + err);
        Z = Z_;
        D = Z * rank_radio;
        MMW_TRY(upload_slot_scalars());
        MMW_TRY(eng.resize(D));
        MMW_TRY(Xh.alloc(eng.bs));
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        MMW_TRY(out64.alloc(std::max(std::max(nnz, C), eng.bs)));
        MMW_TRY(stage64.alloc((size_t)K * D));
        return warm ? restart_warm(nit_) : reset(nit_);
    }
    // what a cold and a warm start of a run share: the counters, the policy's history (chunk_policy.h says what each kind keeps), the plans
    int begin_run(int32_t nit_, bool warm) {
        if (nit_ < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        nit = nit_;
        if (warm) pol.on_warm_restart(iter);
        else pol.on_reset();
        iter = 0;
        emax_enq_iter = emax_iter = -1;
        pending = false;
        if (eng.viol_d.p) MMW_TRY(eng.clear_violation());
        return eng.reset_plan_history(warm);
    }
    // Warm start of the next probe of the binary search (opt-in; the reference restarts every probe from Y = 1/C, X = I,
    // mmw.py:62-68): the accumulated violations e_accu, the accumulated loss L_accu and the last X / Y are kept, the
    // running sums restart from that X / Y, the iteration counter from zero.
    int restart_warm(int32_t nit_) {
        MMW_TRY(begin_run(nit_, true));
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        if (x_tiles) MMW_HIP(hipMemcpyAsync(xs_avg.p, xs_val.p, bt.n_xs * sizeof(T), hipMemcpyDeviceToDevice, st));
        else MMW_HIP(hipMemcpyAsync(xavg.p, xval.p, nnz * sizeof(T), hipMemcpyDeviceToDevice, st));
        MMW_HIP(hipMemcpyAsync(yavg.p, Y.p, C * sizeof(T), hipMemcpyDeviceToDevice, st));
        pt.clear_samples();
        return MMW_OK;
    }
    int reset(int32_t nit_) override {
        if (host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(begin_run(nit_, false));
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        MMW_HIP(hipMemsetAsync(lval.p, 0, nnz * sizeof(T), st));
        if (bt.lval_blk.p) MMW_HIP(hipMemsetAsync(bt.lval_blk.p, 0, (size_t)bt.HB.nent * sizeof(T), st));
        if (bt.afrag.p) MMW_HIP(hipMemsetAsync(bt.afrag.p, 0, bt.afrag_n * sizeof(unsigned), st));
        if (bt.afrag16.p) MMW_HIP(hipMemsetAsync(bt.afrag16.p, 0, bt.afrag_n * sizeof(unsigned short), st));
        eng.last_mfma_ok = true;
        lblk_stale = false;
        x_tiles = false;  // the initial point is written in CSR order; the first matrix-core SDDMM call moves it
        MMW_HIP(hipMemsetAsync(xval.p, 0, nnz * sizeof(T), st));
        MMW_HIP(hipMemsetAsync(xavg.p, 0, nnz * sizeof(T), st));
        MMW_HIP(hipMemsetAsync(e_accu.p, 0, C * sizeof(T), st));
        MMW_HIP(hipMemsetAsync(e_this.p, 0, C * sizeof(T), st));
        hipLaunchKernelGGL((k_set_identity<T>), dim3(grid_elems(K)), dim3(BLOCK), 0, st, K, d_diag.p, xval.p, xavg.p);
        const T y0 = (T)(1.0 / (double)C);
        hipLaunchKernelGGL((k_fill<T>), dim3(grid_elems(C)), dim3(BLOCK), 0, st, C, Y.p, y0);
        hipLaunchKernelGGL((k_fill<T>), dim3(grid_elems(C)), dim3(BLOCK), 0, st, C, yavg.p, y0);
        MMW_HIP(hipGetLastError());
        pt.clear_samples();
        return MMW_OK;
    }
    // CSR-ordered copies of X and its running sum for whoever needs them (API reads, the factor, the gap, the kernels of the other SDDMM
    // forms) while the iterate keeps them in tile order; the tile buffers stay the iterate's
    int x_csr_view() {
        if (!x_tiles) return MMW_OK;
        const size_t nnz = (size_t)H.nnzL();
        hipLaunchKernelGGL((k_x_tiles_to_csr<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, bt.b_e2w.p, xs_val.p, xval.p, xs_avg.p, xavg.p);
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    int x_to_csr() {
        MMW_TRY(x_csr_view());
        x_tiles = false;
        return MMW_OK;
    }
    int x_to_tiles() {
        if (x_tiles) return MMW_OK;
        if (!bt.b_e2w.p || bt.n_xs == 0) return fail(MMW_ERR_STATE, "internal: no tile order on this handle");
        const size_t nnz = (size_t)H.nnzL();
        hipLaunchKernelGGL((k_x_csr_to_tiles<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, bt.b_e2w.p, xval.p, xs_val.p, xavg.p, xs_avg.p);
        MMW_HIP(hipGetLastError());
        x_tiles = true;
        return MMW_OK;
    }
    int copy_state(bool save) {
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        if (save) sn_tiles = x_tiles;
        else x_tiles = sn_tiles;  // the snapshot goes back into the buffers it was taken from
        DevBuf<T>* snap[6] = {&sn_lval, &sn_xval, &sn_xavg, &sn_Y, &sn_yavg, &sn_eaccu};
        DevBuf<T>* live[6] = {&lval, x_tiles ? &xs_val : &xval, x_tiles ? &xs_avg : &xavg, &Y, &yavg, &e_accu};
        const size_t nx = x_tiles ? bt.n_xs : nnz;
        const size_t len[6] = {nnz, nx, nx, C, C, C};
        CopySet<T> cs;
        for (int i = 0; i < 6; ++i) {
            if (snap[i]->n < len[i]) MMW_TRY(snap[i]->alloc(len[i]));
            cs.dst[i] = save ? snap[i]->p : live[i]->p;
            cs.src[i] = save ? live[i]->p : snap[i]->p;
            cs.n[i] = len[i];
        }
        if (sn_plan.n < 1) MMW_TRY(sn_plan.alloc(1));
        cs.plan_dst = save ? sn_plan.p : eng.plan_d.p;
        cs.plan_src = save ? eng.plan_d.p : sn_plan.p;
        hipLaunchKernelGGL((k_copy_state<T>), dim3(256, 6), dim3(BLOCK), 0, st, cs);  // one launch instead of seven copies
        MMW_HIP(hipGetLastError());
        if (!save && bt.lval_blk.p) lblk_stale = true;  // rebuilt from the restored values when the fp32 kernel next needs it
        if (!save && bt.afrag.p) {  // the fragment image follows the restored values
            hipLaunchKernelGGL((k_refrag<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, lval.p, bt.b_fpos.p, bt.afrag.p);
            MMW_HIP(hipGetLastError());
        }
        return MMW_OK;
    }
    // a batch enqueued without plan readbacks is verified here; a violated batch is replayed synchronously
    // A chunk that ends with a violation is discarded and run again from its snapshot.  The second attempt is still a chunk without
    // readbacks, but a cautious one: Lanczos steps (no first-order form) at the a-priori order plus one, an exact plan in front of every
    // exponential (no extrapolated ones), the softmax in its two passes for the first iteration.  Only if that one is refused as well --
    // or the matrix has outgrown the 16-bit split of the matrix-core product, which only the per-iteration readback steps around --
    // do the iterations run synchronously (~2.5x the time per iteration).  Hard probes of a bisection (slot counts at the edge of
    // feasibility: the matrix grows faster than any history predicts) took 3 replays per 150 iterations, 29 ms instead of 13.
    int restore_pending() {
        pol.on_discard();
        emax_enq_iter = emax_iter = -1;  // (the reduction enqueued behind the discarded chunk saw its e_this)
        MMW_TRY(eng.clear_violation());
        MMW_TRY(copy_state(false));
        iter = pend_iter0;
        return pt.drop_since(pend_events0, st);  // the timers of the discarded chunk (earlier chunks keep theirs)
    }
    void say_replay(int viol, const char* how) const {
        if (!live_switch(LIVE_VERBOSE)) return;
        const ExpmPlan& p = eng.last;
        fprintf(stderr, "[replay] iterations %d..%d (Z %d) %s: reason bits %d (1 order, 2 lagged plan, 4 plan, 8 softmax, 16 operands, 32 first-order certificate); launched m %d, first-order %d, one-half %d; "
                        "plan m %d m_eff %d apriori %d rho %.3g absn %.3g est %.2e first_est %.2e tol %.1e\n",
                pend_iter0, pend_iter0 + pend_n - 1, (int)H.Z, how, viol, pol.m_guess, (int)pol.first_guess, (int)pol.first_a16_guess, p.m, p.m_eff, p.m_apriori, p.rho, p.absn,
                plan_estimate(p.conv[std::max(0, std::min(p.m_eff, MAX_ORDER))]), plan_estimate(p.first_est), p.tol);
    }
    void accept_plan() {  // a chunk was settled without a violation: eng.last is its last plan
        pol.plan_seen = true;
        pol.note_plan(eng.last, iter);
        pol.m_guess = pol.next_launch_order(eng.last, eng.max_order, iter);
    }
    int settle() {
        if (!pending) return MMW_OK;
        pending = false;
        int viol = 0;
        MMW_TRY(eng.fetch_plan(&viol));
        if (!viol) {
            accept_plan();
            return MMW_OK;
        }
        ++pol.replays;
        const bool operands_only = (viol & VIOL_OPERANDS) && !pol.first_guess;  // the bf16 split's gate: the fp32 kernel has to take over
        if (viol & VIOL_LAGGED) pol.lagged_missed = true;  // (er-50k: a second chunk missed the same way 32 iterations later)
        say_replay(viol, "discarded");
        MMW_TRY(restore_pending());
        if (sw.cautious_replay && !operands_only && eng.method == MMW_EXPM_LANCZOS && pend_n > 1) {
            pol.plan_cautious(eng.last, eng.max_order);
            pol.exact_plans_only = true;
            const int rc = iterate_impl(pend_n, nullptr, pend_seed, true);
            pol.exact_plans_only = false;
            MMW_TRY(rc);
            viol = 0;
            MMW_TRY(eng.fetch_plan(&viol));
            if (!viol) {
                accept_plan();
                say_replay(0, "cautious attempt accepted");
                return MMW_OK;
            }
            ++pol.replays;
            say_replay(viol, "cautious attempt discarded");
            MMW_TRY(restore_pending());
        }
        say_replay(0, "replayed synchronously");
        return iterate_impl(pend_n, nullptr, pend_seed, false);
    }
    int iterate(int32_t n, const double* randv, uint64_t seed) override {
        if (host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(device));
        if (n < 0) return fail(MMW_ERR_ARG, "n must be >= 0");
        MMW_TRY(settle());
        if (iter + n > nit) return fail(MMW_ERR_STATE, "mmw_iterate: more iterations than announced to mmw_create/mmw_reset");
        const bool optimistic = randv == nullptr && n > 1 && !kt_exact() && !sw.sync_plan;  // profiling mode 1 counts exact launches
        if (!optimistic) {
            pol.chain_ok = false;
            MMW_TRY(iterate_impl(n, randv, seed, false));
            return enqueue_emax();
        }
        // Chunks enqueued without plan readbacks.  Each chunk starts from a device snapshot; before the next one starts the
        // plan of the previous is looked at (one sync): a chunk that needed more steps than were launched is restored and
        // replayed with per-iteration readback, and the launch order follows the device.  The last chunk is settled by the
        // next call.  How long a chunk is and what it is launched with: ChunkPolicy::chunk_length / plan_chunk.
        int left = n;
        while (left > 0) {
            MMW_TRY(settle());
            const int chunk = pol.chunk_length(eng.last, sw, iter, left);
            pol.plan_chunk(eng.last, sw, eng.max_order, iter, chunk, sizeof(T) == 4, bt.afrag16.p != nullptr, plane_rounding());
            MMW_TRY(copy_state(true));
            pend_iter0 = iter; pend_n = chunk; pend_seed = seed; pend_events0 = pt.mark();
            MMW_TRY(iterate_impl(chunk, nullptr, seed, chunk > 1));
            pol.warm_fresh = false;
            pending = chunk > 1;
            left -= chunk;
        }
        return enqueue_emax();
    }
    // The objective record's one number -- the largest violation of the last iteration (MMW_F_E_MAX) -- is reduced right behind the call's
    // work and copied out by the mmw_sync that waits for it anyway: reading it afterwards is free (its launch + copy + wait were a third
    // of what a 20-step timed region spends on its record).  A replay of the last chunk changes `iter` back and forth but ends at the same
    // e_this only after re-running, so the value is tied to the iteration count AND dropped whenever a chunk is discarded.
    int enqueue_emax() {
        if (iter <= 0) return MMW_OK;
        if (!emax_d.p) MMW_TRY(emax_d.alloc(1));
        hipLaunchKernelGGL((k_max_of<T>), dim3(1), dim3(1024), 0, st, (size_t)H.C(), e_this.p, emax_d.p);
        MMW_HIP(hipGetLastError());
        emax_enq_iter = iter;
        emax_iter = -1;
        return MMW_OK;
    }
    int sketch_slabs() const { return std::min(grid_rows(K), sw.sk_slabs); }  // few slabs for the start-norm reduction
    int launch_sketch(hipStream_t s, uint64_t seed, uint32_t it, bool planes_f16 = false) {
        const bool lz = eng.method == MMW_EXPM_LANCZOS;
        unsigned short* pl = eng.start_planes();
        hipLaunchKernelGGL((k_sketch_rng<T>), dim3(sketch_slabs()), dim3(BLOCK), lz ? (size_t)(WAVES_PER_BLOCK + 1) * eng.lay.Dpad * sizeof(double) : 0, s, K, D, eng.lay.Dpad,
                           seed, it, eng.start_block(), lz ? eng.partial_sq.p : (double*)nullptr, pl, planes_f16 ? 1 : 0,
                           planes_f16 && lz && fv_measure ? eng.partial_du.p : (double*)nullptr);
        eng.planes_ready[0] = pl != nullptr;
        eng.planes0_f16 = planes_f16 && pl != nullptr;
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    // One call of iterate_impl: what is fixed for its `n` iterations, then what one iteration leaves for the next.
    struct ChunkRun {
        int n; const double* randv; uint64_t seed; bool optimistic;
        bool lanczos;     // eng.method == MMW_EXPM_LANCZOS
        // X on the pattern comes from the matrix-core SDDMM in this call: it writes -- and the DUAL phase then reads -- X in tile order;
        // every other SDDMM form works on the CSR order
        bool sd_mf_call;
        PatternDev<T> P;
        const T* xcur;    // the X the DUAL phase reads (the layout does not change inside a call)
        int gr, gd, gc, gl, Dpad;  // grids of the row kernels, the DUAL pass, the softmax passes and the LOSS pass
        int m_launch;     // Lanczos steps launched per exponential (0: as the plan read back says)
        bool lag_chunk, chain, chain_plan, fuse_sketch;
        // carried from one iteration to the next
        bool xavg_deferred = false;  // the X just made is added to its running sum by the next iteration's LOSS pass
        bool rs_ok = false;          // rsfx holds the row sums of the X the next DUAL phase starts from
        FirstVerify fv_pending;      // the first-order exponential of the previous iteration of this call still waits for its check
    };
    // what the phases of ONE iteration hand each other
    struct IterRun {
        int it, acc;  // index within the call; 1: X / Y of this iteration go into the running sums
        bool lagged_it = false, fused_dual = false, rs_zeroed = false, first_it = false;
        PlanArgs pa;
        int ntr1 = 0;
    };
    // the sketch of the iteration about to run is already in the start block (drawn by a LOSS pass or by the previous SDDMM launch)
    bool sketch_drawn(const ChunkRun& c) const { return !c.randv && sketch_done_for == (int64_t)iter && sketch_done_seed == c.seed; }
    template <int NCH> void launch_sddmm(const ChunkRun& c, int acc) {
        hipLaunchKernelGGL((k_sddmm<T, NCH>), dim3(c.gr), dim3(BLOCK), 0, st, c.P, c.Dpad, eng.lay.LPR, eng.lay.G, Xh.p, drow.p, tr_part.p, c.gr, xval.p, xavg.p, acc);
    }
    template <int MT, int NB>
    int launch_sddmm_mfma(const ChunkRun& c, dim3 grid, const SdMfmaDev& SM, const double* trp, int ntr, int acc, long long* rs_out, const long long* dfx,
                          unsigned long long* stamps, const FirstVerify& fv) {
        MMW_TRY(set_max_lds(reinterpret_cast<const void*>(&k_sddmm_mfma<MT, NB>), sdm_lds_bytes<MT, NB>()));
        hipLaunchKernelGGL((k_sddmm_mfma<MT, NB>), grid, dim3(256 * MT), (sdm_lds_bytes<MT, NB>()), st, eng.mf, SM, K, c.Dpad,
                           reinterpret_cast<const char*>(xh_planes.p), drow.p, trp, ntr, xs_val.p, xs_avg.p, acc, rs_out, dfx, stamps, fv);
        return MMW_OK;
    }
    int iterate_impl(int32_t n, const double* randv, uint64_t seed, bool optimistic) {
        ChunkRun c{n, randv, seed, optimistic, eng.method == MMW_EXPM_LANCZOS};
        c.sd_mf_call = sizeof(T) == 4 && bt.sddmm_mfma && eng.use_blk && c.lanczos && (eng.lay.Dpad % 32) == 0 && bt.b_e2w.p != nullptr;
        if (n > 0) MMW_TRY(c.sd_mf_call ? x_to_tiles() : x_to_csr());
        c.P = pat();
        c.xcur = x_tiles ? xs_val.p : xval.p;
        c.gr = grid_rows(K);
        // the DUAL pass's grid: its workgroups stride over the row pairs, and the slabs it leaves (maxima, softmax sums, |L| row sums) are
        // folded by one workgroup afterwards.  One resident round of workgroups (five per CU at the pass's 86 registers) instead of one per
        // eight rows: half the slabs to fold and no second round's tail -- DUAL 21.0 -> 20.0 us per step at the benchmark (640: 22.3; 1920: 20.2)
        c.gd = std::min(c.gr, 5 * device_cus());
        c.gc = grid_elems((size_t)H.C());
        c.gl = (int)std::min<size_t>(((size_t)H.nnzL() + BLOCK - 1) / BLOCK, (size_t)LOSS_GRID_MAX);  // LOSS: one thread per stored entry, grid-stride
        c.Dpad = eng.lay.Dpad;
        c.m_launch = optimistic ? pol.m_guess : 0;
        // from the plan the last settled chunk ended on; not in the first chunk after a warm restart: with another slot count the matrix grows
        // at another rate than the history the extrapolation rests on (its bound was missed and the chunk replayed, measured)
        c.lag_chunk = optimistic && pol.lagged_ok(eng.last, sw) && !pol.warm_fresh && !pol.exact_plans_only;
        c.chain = optimistic && pol.chain_ok;      // this chunk continues the previous one (see ChunkPolicy::chain_ok)
        pol.chain_ok = false;
        // the plan is chained only while a single step is accepted with a factor 8 to spare: near a change of order an exact plan at
        // the start of every chunk keeps the a-priori order down (er-1pct: 5 127 it/s with it, 4 495 without)
        c.chain_plan = c.chain && pol.plan_has_room(eng.last);
        // the row sums of X the DUAL phase starts from: left by the last matrix-core SDDMM (this call's previous iteration, or the chunk
        // this one continues), otherwise taken by k_dual_rows
        c.rs_ok = c.chain && rs_last && rs_enabled && rsfx.p != nullptr;
        rs_last = false;
        // drawing the next sketch in extra workgroups of the SDDMM launch paid off with 8-wave SDDMM workgroups (+3.7 %); with
        // 16-wave ones (two per CU, every wave slot taken) it costs 1.5 %, so it is opt-in
        c.fuse_sketch = !kt_exact() && !pt.timing && sw.fused_sketch;
        sketch_done_for = -1;  // whatever an earlier batch left in the start block is not trusted
        for (int it = 0; it < n; ++it) {
            IterRun s;
            s.it = it;
            s.acc = (iter + 1 < nit) ? 1 : 0;  // the last X / Y are not averaged (mmw.py:77-78,203)
            MMW_TRY(pt.record(0, iter, st));
            MMW_TRY(phase_dual(c, s));
            MMW_TRY(phase_loss(c, s));
            MMW_TRY(phase_expm(c, s));
            MMW_TRY(phase_x(c, s));
            ++iter;
        }
        return chunk_tail(c);
    }
    // ---- DUAL: the violations of the current X, their softmax, and (lagged) the plan of this iteration's exponential
    int phase_dual(ChunkRun& c, IterRun& s) {
        MMW_TRY(kt.begin(KT_DUAL));
        const long long* rs_it = c.rs_ok ? rsfx.p : nullptr;
        const FirstVerify fv = c.fv_pending;
        c.fv_pending = FirstVerify{};
        if (rs_it) ++n_rs_iters;
        if (!rs_it) hipLaunchKernelGGL((k_dual_rows<T>), dim3(c.gr), dim3(BLOCK), 0, st, c.P, c.xcur, rsum.p, e_this.p);
        // Lagged planning inside a chunk (not the first iteration of a run, a replay or after a change of the iterate, which plan exactly): k_dual_h also takes the row sums of the
        // L it walks over anyway -- last iteration's -- and one extra workgroup of k_softmax_b turns them into this iteration's plan
        // (extrapolated bounds, checked by the next plan): k_rowsums + k_plan leave the critical path.
        s.lagged_it = c.optimistic && (s.it > 0 || c.chain_plan) && c.lanczos && c.lag_chunk;
        if (s.lagged_it) {
            s.pa.plan = eng.plan_d.p; s.pa.part = eng.row_part.p; s.pa.viol = eng.viol_d.p; s.pa.tol = eng.tol; s.pa.K = K; s.pa.method = eng.method;
            s.pa.max_order = eng.max_order; s.pa.np = c.gd; s.pa.m_launch = c.m_launch; s.pa.apost = eng.apost() ? 1 : 0; s.pa.iter_seen = pol.age(iter) - 1;
        }
        // Inside a chunk (not its first iteration) the softmax rides in k_dual_h, shifted by the previous iteration's maximum
        // instead of this one's: one small workgroup then folds the sums, and the LOSS pass normalises where it reads
        // (kernels_loop.h, k_dual_h / k_dual_scal).  Two launches of the dependent chain fewer.
        s.fused_dual = c.optimistic && (s.it > 0 || c.chain) && !sw.no_fused_dual;
        if (s.fused_dual) {
            ++n_fused_iters;
            if (yun.n < (size_t)H.C()) MMW_TRY(yun.alloc((size_t)H.C()));
            // MMW_DUAL_STAMPS=1 (developer aid): per-wave phase clocks of the last iteration's launch, printed to stderr
            StampBuf dh_stamps;
            const bool want_dst = s.it + 1 == c.n && live_switch(LIVE_DUAL_STAMPS);
            MMW_TRY(dh_stamps.request(want_dst, (size_t)c.gd * WAVES_PER_BLOCK * 8, st));
            hipLaunchKernelGGL((k_dual_h<T>), dim3(c.gd), dim3(BLOCK), 0, st, c.P, rsum.p, e_this.p, e_accu.p, eta, max_part.p,
                               (const T*)(s.lagged_it ? lval.p : nullptr), 0.5, eng.row_part.p, (const double*)(scal.p + 4), yun.p, wH.p, sum_part.p,
                               rs_it, c.xcur, FirstVerify{}, dh_stamps.p());
            if (want_dst) MMW_TRY(dump_dual_stamps(st, dh_stamps.p(), c.gd));
            hipLaunchKernelGGL(k_dual_scal, dim3(1 + fv.nwg), dim3(DSCAL_THREADS), 0, st, sum_part.p, max_part.p, c.gd, scal.p,
                               dual_gap, eng.viol_d.p, fv);
        } else {
            hipLaunchKernelGGL((k_dual_h<T>), dim3(c.gd + fv.nwg), dim3(BLOCK), 0, st, c.P, rsum.p, e_this.p, e_accu.p, eta, max_part.p,
                               (const T*)(s.lagged_it ? lval.p : nullptr), 0.5, eng.row_part.p, (const double*)nullptr, (T*)nullptr, (T*)nullptr,
                               (double*)nullptr, rs_it, c.xcur, fv);
            hipLaunchKernelGGL((k_softmax_a<T>), dim3(c.gc), dim3(BLOCK), 0, st, c.P, e_accu.p, Y.p, max_part.p, c.gd, sum_part.p);
            hipLaunchKernelGGL((k_softmax_b<T>), dim3(c.gc + (s.lagged_it ? 1 : 0)), dim3(BLOCK), 0, st, (int)H.C(), Y.p, yavg.p, s.acc, sum_part.p, c.gc, scal.p,
                               K + (int)H.E_asso(), d_invn.p, wH.p, s.pa, max_part.p, c.gd);
        }
        MMW_TRY(kt.end());
        MMW_TRY(pt.record(1, iter, st));
        return MMW_OK;
    }
    // ---- LOSS: L += eta * loss(Y); this iteration's sketch rides in its launch
    int phase_loss(ChunkRun& c, IterRun& s) {
        MMW_TRY(kt.begin(KT_LOSS));
        // the X of the previous iteration of this chunk is added to the running sum inside this pass (xavg_deferred), and
        // this iteration's sketch is drawn by leading workgroups of the same launch (VALU work under a memory-bound pass)
        s.rs_zeroed = rs_enabled && rsfx.p != nullptr && bt.sddmm_mfma;  // the coming SDDMM may add its row sums to zeroed totals
        // the exponential of this iteration as one first-order product (decided per chunk, first_order_ok)
        const bool sketch_have = sketch_drawn(c);
        // (a sketch an earlier launch already drew came without the fp16 plane and the measure of its rounding: no first-order form then)
        s.first_it = c.optimistic && pol.first_guess && c.m_launch == 1 && !c.randv && s.rs_zeroed && sizeof(T) == 4 && eng.mfma_now() &&
                              c.lanczos && eng.use_blk && (c.Dpad % 32) == 0 && !sketch_have;
        SketchArgs<T> skl{};
        // (with the per-iteration phase events of mmw_set_timing on as well: the draw then counts into the LOSS phase's microseconds
        // instead of the exponential's -- the reference draws inside mmw.py:172-181 -- and the iteration's total is unchanged; a launch of
        // its own cost the class path 14 us per iteration)
        if (!c.randv && !sketch_have && !kt_exact() && !sw.no_loss_sketch) {
            skl.nblocks = sketch_slabs(); skl.K = K; skl.D = D; skl.seed = c.seed; skl.iter = (uint32_t)iter;
            skl.R = eng.start_block();
            skl.colsq_part = c.lanczos ? eng.partial_sq.p : nullptr;
            skl.planes = eng.start_planes();
            skl.planes_f16 = s.first_it ? 1 : 0;
            skl.dusq_part = s.first_it && fv_measure ? eng.partial_du.p : nullptr;
            eng.planes_ready[0] = skl.planes != nullptr;
            eng.planes0_f16 = s.first_it && skl.planes != nullptr;
            sketch_done_for = (int64_t)iter; sketch_done_seed = c.seed; sketch_done_slabs = skl.nblocks;
        }
        // the blocked copy of L feeds the fp32 LDS kernel only: while the matrix-core kernel runs the products it is left stale
        const bool mf_it = eng.mfma_now() && c.lanczos;
        if (mf_it) lblk_stale = true;
        const PlanArgs pl_loss = s.fused_dual ? s.pa : PlanArgs{};  // the fused pass has no softmax pass B to lend the planning a workgroup
        hipLaunchKernelGGL((k_loss<T>), dim3(c.gl + skl.nblocks + (pl_loss.plan ? 1 : 0)), dim3(BLOCK), skl.nblocks && c.lanczos ? (size_t)(WAVES_PER_BLOCK + 1) * c.Dpad * sizeof(double) : 0,
                           st, c.P, d_lrow.p, s.fused_dual ? yun.p : Y.p, wH.p, scal.p, lval.p, eta,
                           (const int*)(eng.use_blk && !mf_it ? bt.b_bpos.p : nullptr), bt.lval_blk.p,
                           (const T*)(c.xavg_deferred ? xval.p : nullptr), c.xavg_deferred ? xavg.p : (T*)nullptr, skl, c.Dpad,
                           (const int*)(eng.use_mfma ? bt.b_fpos.p : nullptr), bt.afrag.p, s.fused_dual ? Y.p : (T*)nullptr, yavg.p, s.acc, pl_loss,
                           s.rs_zeroed ? rsfx.p : (long long*)nullptr, s.rs_zeroed ? (s.first_it ? 2 * K : K) : 0, s.first_it ? 1 : 0,
                           s.first_it && pol.first_a16_guess ? bt.afrag16.p : (unsigned short*)nullptr);
        c.xavg_deferred = false;
        MMW_TRY(kt.end());
        MMW_TRY(pt.record(2, iter, st));
        return MMW_OK;
    }
    // ---- the sketch (unless it rode) and exp(L/2) applied to it
    int phase_expm(ChunkRun& c, IterRun& s) {
        const bool sketch_rode = sketch_drawn(c);  // by this iteration's LOSS pass or the previous SDDMM launch: nothing to launch, nothing to time
        if (!sketch_rode) MMW_TRY(kt.begin(KT_SKETCH));
        if (c.randv) {
            MMW_TRY(copy_h2d(stage64.p, c.randv + (size_t)s.it * K * D, (size_t)K * D * sizeof(double), st));  // page-locked staging (runtime.h)
            hipLaunchKernelGGL((k_import_block<T>), dim3(grid_elems(eng.bs)), dim3(BLOCK), 0, st, K, D, c.Dpad, stage64.p, eng.start_block());
            eng.planes_ready[0] = false;  // an uploaded sketch is split by a pass of its own
            last_was_rng = false;
        } else {
            if (!sketch_rode) MMW_TRY(launch_sketch(st, c.seed, (uint32_t)iter, s.first_it));
            eng.start_colsq_ready = c.lanczos;  // the Lanczos start norms come out of the sketch kernel
            eng.npart_start = sketch_rode ? sketch_done_slabs : sketch_slabs();
            sketch_done_for = -1;
            last_was_rng = true;
            last_seed = c.seed;
        }
        if (!sketch_rode) MMW_TRY(kt.end());
        MMW_HIP(hipGetLastError());
        // X on the pattern runs on the matrix cores too when the exponential did: the combination then also writes y's planes
        eng.out_planes = nullptr;
        if constexpr (sizeof(T) == 4) {
            if (c.sd_mf_call) {
                if (xh_planes.n < 2 * eng.bs) MMW_TRY(xh_planes.alloc(2 * eng.bs));
                eng.out_planes = xh_planes.p;
            }
        }
        // inside a chunk only the SDDMM reads X_half; the chunk's last iteration leaves the fp32 copy the API hands out
        eng.planes_only = eng.out_planes != nullptr && c.optimistic && s.it + 1 < c.n && !sw.keep_xhalf;
        eng.rownorm_d = drow.p;  // the Lanczos combination also emits the row norms and the trace slabs
        eng.rownorm_part = tr_part.p;
        eng.plan_iter = pol.age(iter);
        if (s.first_it) {
            const size_t need = (size_t)eng.first_grid_max();
            if (tr1_part.n < need) {
                MMW_TRY(tr1_part.alloc(need));
                MMW_HIP(hipMemsetAsync(tr1_part.p, 0, need * sizeof(double), st));
            }
            MMW_TRY(eng.apply_first(eng.planes_only ? (T*)nullptr : Xh.p, 0.5, c.m_launch, s.lagged_it, xh_planes.p, rsfx.p + K, tr1_part.p, &s.ntr1,
                                    pol.first_a16_guess ? bt.afrag16.p : (const unsigned short*)nullptr));
            ++n_first_iters;
            if (pol.first_a16_guess) ++n_first16_iters;
        } else
            MMW_TRY(eng.apply(Xh.p, 0.5, c.m_launch, s.lagged_it));
        return MMW_OK;
    }
    // ---- X on the pattern from exp(L/2)R, and its running sum
    int phase_x(ChunkRun& c, IterRun& s) {
        MMW_TRY(kt.begin(KT_SDDMM));
        if (!c.lanczos)
            hipLaunchKernelGGL((k_rownorm2<T>), dim3(c.gr), dim3(BLOCK), 0, st, K, c.Dpad, Xh.p, drow.p, tr_part.p);
        bool sd_done = false;
        c.rs_ok = false;
        if constexpr (sizeof(T) == 4) {
            if (c.sd_mf_call) {
                const SdMfmaDev SM = bt.sd_mfma_dev();
                const long long* dfx = s.first_it ? rsfx.p + K : nullptr;
                const double* trp = s.first_it ? tr1_part.p : tr_part.p;
                const int ntr = s.first_it ? s.ntr1 : c.gr;
                // the certificate of this iteration's first-order exponential rides in this launch (8 more columns of workgroups)
                FirstVerify fv_now;
                if (s.first_it) {
                    fv_now.plan = eng.plan_d.p; fv_now.viol = eng.viol_d.p; fv_now.o2 = eng.partial_o2.p; fv_now.n_o2 = eng.mf.nb;
                    fv_now.u2 = eng.partial_sq.p; fv_now.du2 = fv_measure ? eng.partial_du.p : nullptr; fv_now.rows = K; fv_now.n_u2 = eng.npart_start; fv_now.Dpad = c.Dpad;
                    fv_now.nwg = c.Dpad / FV_COLS;
                    fv_now.cA = pol.first_a16_guess ? F16_UNIT : F16_CA_TWO;
                    fv_now.du_scale = sw.fv_du_scale;
                }
                const bool fv_rides = s.first_it && sw.fv_in_sddmm;
                const dim3 grid((bt.HB.nbm() + 7) / 8 * 8 + (fv_rides ? 8 : 0), (bt.HB.m_ntile_max + SDM_GT - 1) / SDM_GT);
                long long* rs_out = s.rs_zeroed ? rsfx.p : nullptr;  // this iteration's LOSS pass zeroed the totals
                // MMW_SD_STAMPS=1 (developer aid): per-wave phase clocks of the last iteration's launch, printed to stderr
                StampBuf sdm_stamps;
                const size_t n_st = (size_t)grid.x * grid.y * 16 * 8;
                const bool want_st = s.it + 1 == c.n && live_switch(LIVE_SD_STAMPS);
                MMW_TRY(sdm_stamps.request(want_st, n_st, st));
                // two chunks resident per workgroup (three were built and measured 1 % slower)
                if (bt.HB.mfma_mt == 2) MMW_TRY((launch_sddmm_mfma<2, 2>(c, grid, SM, trp, ntr, s.acc, rs_out, dfx, sdm_stamps.p(), fv_rides ? fv_now : FirstVerify{})));
                else MMW_TRY((launch_sddmm_mfma<1, 2>(c, grid, SM, trp, ntr, s.acc, rs_out, dfx, sdm_stamps.p(), fv_rides ? fv_now : FirstVerify{})));
                if (want_st) MMW_TRY(dump_sddmm_stamps(st, sdm_stamps.p(), n_st, grid, bt.HB.mfma_mt));
                sd_done = true;
                // (MMW_FV_IN_SDDMM=0: certified by spare workgroups of the next iteration's DUAL phase, or by a launch of its own after the chunk's last)
                if (s.first_it && !fv_rides) c.fv_pending = fv_now;
                c.rs_ok = rs_out != nullptr;
            }
        }
        if (!sd_done && eng.use_blk) MMW_TRY(bt.ensure_sd(st, H, K, eng.lay.Dpad, sw.full_tile));
        if (sd_done) {
        } else if (bt.sddmm_blk2 && eng.use_blk) {
            StampBuf sd_stamps;  // MMW_SD_STAMPS=1: phase stamps of the last iteration's SDDMM
            MMW_TRY(sd_stamps.request(s.it + 1 == c.n && live_switch(LIVE_SD_STAMPS), (size_t)16 * 8192, st));
            const Sd2Dev S = bt.sd2_dev();
            constexpr int CT2 = B2_ROW_BYTES / (int)sizeof(T);
            const int per = (bt.sd2_nitems + 7) / 8;
            SketchArgs<T> sk{};
            const size_t sd_lds = std::max((size_t)bt.HB.un8_max * B2_ROW_BYTES, std::min((size_t)(SD2_THREADS / WAVE) * c.Dpad * sizeof(double), (size_t)65536));
            if (c.fuse_sketch && !c.randv && s.it + 1 < c.n && (size_t)(SD2_THREADS / WAVE) * c.Dpad * sizeof(double) <= sd_lds) {
                // the start block and its norm slabs are free once the combination has run: draw the next iteration's sketch here
                constexpr int VBW = SD2_THREADS / BLOCK;  // a workgroup here stands for this many of the stand-alone kernel's
                sk.nblocks = (sketch_slabs() + VBW - 1) / VBW;
                sk.K = K; sk.D = D; sk.seed = c.seed; sk.iter = (uint32_t)(iter + 1);
                sk.R = eng.start_block();
                sk.colsq_part = c.lanczos ? eng.partial_sq.p : nullptr;
                sk.planes = eng.start_planes();
                sk.planes_f16 = 0;
                eng.planes_ready[0] = sk.planes != nullptr;
                eng.planes0_f16 = false;
                sketch_done_for = (int64_t)iter + 1;
                sketch_done_seed = c.seed;
                sketch_done_slabs = sk.nblocks * VBW;
            }
            hipLaunchKernelGGL((k_sddmm_blk2<T>), dim3(per * 8 + sk.nblocks), dim3(SD2_THREADS), sd_lds, st, blkdev(), S, c.P, c.Dpad,
                               (c.Dpad + CT2 - 1) / CT2, Xh.p, drow.p, tr_part.p, c.gr, xval.p, xavg.p, s.acc, sk, sd_stamps.p());
            if (sd_stamps.p()) MMW_TRY(dump_stamps(st, sd_stamps.p()));
        } else if (bt.sddmm_blk && eng.use_blk) {
            const SdDev S = bt.sd_dev();
            constexpr int CT = BLK_TILE_BYTES / (int)sizeof(T);
            const int ntiles = (c.Dpad + CT - 1) / CT;
            const int per = (bt.HB.nb() + 7) / 8;
            hipLaunchKernelGGL((k_sddmm_blk<T>), dim3(per * 8), dim3(BLK_THREADS), (size_t)BLK_UNION_ROWS * BLK_TILE_BYTES, st, blkdev(), S, c.P, c.Dpad,
                               ntiles, Xh.p, drow.p, tr_part.p, c.gr, xval.p, xavg.p, s.acc);
        } else
            switch (eng.lay.NCH) {
                case 1: launch_sddmm<1>(c, s.acc); break;
                case 2: launch_sddmm<2>(c, s.acc); break;
                case 3: launch_sddmm<3>(c, s.acc); break;
                default: launch_sddmm<4>(c, s.acc); break;
            }
        // the running sum of X (mmw.py:77-78): one coalesced pass; none of the SDDMM kernels read-modify-writes xavg
        if (sd_done) {  // the matrix-core SDDMM added X to its running sum itself (tile order)
        } else if (s.acc && s.it + 1 < c.n && !kt_exact()) c.xavg_deferred = true;  // the next iteration's LOSS pass adds it
        else if (s.acc) hipLaunchKernelGGL((k_accumulate<T>), dim3((unsigned)std::min<size_t>(((size_t)H.nnzL() + BLOCK - 1) / BLOCK, 4096)), dim3(BLOCK), 0, st, (size_t)H.nnzL(), xval.p, xavg.p);
        MMW_TRY(kt.end());
        MMW_HIP(hipGetLastError());
        MMW_TRY(pt.record(3, iter, st));
        return MMW_OK;
    }
    // ---- after the call's last iteration: the certificate and the lagged plan that no later iteration checks
    int chunk_tail(ChunkRun& c) {
        if (c.fv_pending.plan) {  // the chunk's last first-order exponential
            hipLaunchKernelGGL(k_first_verify, dim3(c.fv_pending.nwg), dim3(BLOCK), 0, st, c.fv_pending);
            MMW_HIP(hipGetLastError());
        }
        if (c.optimistic && c.n > 1 && c.lag_chunk && c.lanczos) {
            // the chunk's last plan was extrapolated and no later plan of the chunk sees its matrix: check it here
            hipLaunchKernelGGL((k_rowsums<T>), dim3(eng.nwide), dim3(BLOCK), 0, st, K, d_indptr.p, d_col.p, lval.p, 0.5, eng.row_part.p);
            hipLaunchKernelGGL(k_plan_verify, dim3(1), dim3(PLAN_THREADS), 0, st, K, eng.row_part.p, eng.nwide, eng.plan_d.p, eng.viol_d.p, pol.age(iter) - 1);
            MMW_HIP(hipGetLastError());
        }
        // until settle() finds a violation or something touches the iterate.  A handle that has had to replay a chunk keeps restarting
        // its chunks exactly (measured on er-1pct, whose order rises during the run: 5 100 it/s so, 4 500 chained)
        pol.chain_ok = c.optimistic && c.n > 1 && pol.replays == 0 && !sw.no_chunk_chain;
        rs_last = c.rs_ok;
        return MMW_OK;
    }
    int sync() override {
        if (host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(settle());
        const bool want_emax = emax_enq_iter == iter && emax_iter != iter && emax_d.p != nullptr;
        if (want_emax) MMW_HIP(hipMemcpyAsync(&emax_h, emax_d.p, sizeof(double), hipMemcpyDeviceToHost, st));
        MMW_HIP(hipStreamSynchronize(st));
        if (want_emax) emax_iter = iter;
        MMW_TRY(kt.flush());
        return pt.flush(iter, st);
    }
    // The Philox sketch of (seed, iteration) exactly as the loop draws it -- the generator is counter-based, so this is the block
    // iteration `iteration` of a device-RNG run with that seed multiplied, whatever chunk it ran in (parity tests give it to the oracle).
    int sketch(uint64_t seed, int32_t iteration, double* out, int64_t n) override {
        if (host_only) return host_only_pattern();
        if (iteration < 0) return fail(MMW_ERR_ARG, "mmw_sketch: iteration must be >= 0");
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(sync());
        hipLaunchKernelGGL((k_sketch_rng<T>), dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, seed, (uint32_t)iteration, eng.Tm.p, (double*)nullptr);
        MMW_HIP(hipGetLastError());
        return export_block(eng.Tm.p, out, n);
    }
    int export_T(const T* src, size_t n, double* out, int64_t have) {
        if ((int64_t)n != have) return fail(MMW_ERR_ARG, "mmw_read_f64: wrong length " + std::to_string(have) + ", expected " + std::to_string(n));
        hipLaunchKernelGGL((k_to_f64<T>), dim3(grid_elems(n)), dim3(BLOCK), 0, st, n, src, out64.p);
        MMW_HIP(hipGetLastError());
        MMW_TRY(copy_d2h(out, out64.p, (size_t)n * sizeof(double), st));
        return MMW_OK;
    }
    int export_block(const T* src, double* out, int64_t have) {
        const size_t n = (size_t)K * D;
        if ((int64_t)n != have) return fail(MMW_ERR_ARG, "mmw_read_f64: wrong length for a K x D block");
        hipLaunchKernelGGL((k_export_block<T>), dim3(grid_elems(n)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, src, out64.p);
        MMW_HIP(hipGetLastError());
        MMW_TRY(copy_d2h(out, out64.p, (size_t)n * sizeof(double), st));
        return MMW_OK;
    }
    static int export_vals(std::initializer_list<double> v, double* out, int64_t have, const char* wrong_length) {  // a few numbers of fixed count
        if (have != (int64_t)v.size()) return fail(MMW_ERR_ARG, wrong_length);
        std::copy(v.begin(), v.end(), out);
        return MMW_OK;
    }
    int read_f64(int which, double* out, int64_t n) override {
        // the fields a host-only handle holds too
        const std::vector<double>* hv = which == MMW_F_S_SUM ? &H.S_sum : which == MMW_F_NORM_H ? &H.norm_H : which == MMW_F_ST_DATA ? &H.st_data : nullptr;
        if (host_only) return hv ? export_vec(*hv, out, n, "mmw_read_f64") : host_only_pattern();
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(sync());
        if (which == MMW_F_ST_DATA) MMW_TRY(ensure_host_lists());
        if (hv) return export_vec(*hv, out, n, "mmw_read_f64");
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        switch (which) {
            case MMW_F_Y: return export_T(Y.p, C, out, n);
            case MMW_F_E_ACCU: return export_T(e_accu.p, C, out, n);
            case MMW_F_E_THIS: return export_T(e_this.p, C, out, n);
            case MMW_F_E_MAX: {
                if (n != 1) return fail(MMW_ERR_ARG, "the maximum violation is one number");
                if (emax_iter == iter && emax_iter >= 0) {  // reduced behind the last mmw_iterate's work and fetched by mmw_sync
                    out[0] = emax_h;
                    return MMW_OK;
                }
                hipLaunchKernelGGL((k_max_of<T>), dim3(1), dim3(1024), 0, st, C, e_this.p, out64.p);
                MMW_HIP(hipGetLastError());
                return copy_d2h(out, out64.p, sizeof(double), st);
            }
            case MMW_F_LVAL: return export_T(lval.p, nnz, out, n);
            case MMW_F_XVAL: MMW_TRY(x_csr_view()); return export_T(xval.p, nnz, out, n);
            case MMW_F_XAVG: MMW_TRY(x_csr_view()); return export_T(xavg.p, nnz, out, n);
            case MMW_F_YAVG: return export_T(yavg.p, C, out, n);
            case MMW_F_XHALF: return export_block(Xh.p, out, n);
            case MMW_F_SKETCH: {
                if (!last_was_rng || iter == 0) return fail(MMW_ERR_STATE, "the sketch can be read back only after a device-generated iteration");
                hipLaunchKernelGGL((k_sketch_rng<T>), dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, last_seed, (uint32_t)(iter - 1), eng.Tm.p, (double*)nullptr);
                return export_block(eng.Tm.p, out, n);
            }
            case MMW_F_PHASE_US: return export_vec(pt.phase_us, out, n, "mmw_read_f64");
            case MMW_F_EXPM_INFO:
                return export_vals({eng.last.rho, (double)(eng.last.m_eff > 0 ? eng.last.m_eff : eng.last.m), (double)eng.last.nsub, eng.last.mu}, out, n, "expm info has 4 entries");
            case MMW_F_BLOCKING:
                return export_vals({eng.use_blk ? 1.0 : 0.0, (double)(bt.HB.usable ? bt.HB.nb() : 0), (double)bt.HB.reuse, (double)pol.replays}, out, n, "blocking info has 4 entries");
            case MMW_F_SPMM_KIND:
                return export_vals({!eng.use_blk ? 0.0 : (eng.use_mfma ? 3.0 : (eng.blk.half_tile ? 2.0 : 1.0)), eng.use_mfma && eng.last_mfma_ok ? 1.0 : 0.0}, out, n, "spmm kind has 2 entries");
            case MMW_F_DUAL_INFO:
                return export_vals({(double)n_rs_iters, (double)n_fused_iters, (double)n_first_iters, (double)n_first16_iters}, out, n, "dual info has 4 entries");
            case MMW_F_FACTOR: return extras.read_factor(out, n);
            case MMW_F_KERNEL_US: {
                if (n != 2 * KT_NSLOT) return fail(MMW_ERR_ARG, "kernel timers have 2*9 entries");
                for (int i = 0; i < KT_NSLOT; ++i) { out[2 * i] = kt.total_us[i]; out[2 * i + 1] = kt.count[i]; }
                return MMW_OK;
            }
            default: return fail(MMW_ERR_ARG, "mmw_read_f64: unknown field");
        }
    }
    int read_i32(int which, int32_t* out, int64_t n) override {
        MMW_TRY(ensure_host_lists());
        const std::vector<int32_t>* v = host_list_i32(H, which);
        return v ? export_vec(*v, out, n, "mmw_read_i32") : fail(MMW_ERR_ARG, "mmw_read_i32: unknown field");
    }
    int gap(double out[3]) override {
        if (host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(settle());
        if (iter >= nit) return fail(MMW_ERR_STATE, "mmw_gap: call it before an iteration (the running sums then hold iter+1 terms)");
        MMW_TRY(x_csr_view());
        PatternDev<T> Pc = pat();  // the gap's kernels walk the CSR copy
        Pc.e2w = nullptr; Pc.xasso = nullptr; Pc.xdiag_base = -1;
        return extras.gap(Pc, d_lrow.p, xavg.p, yavg.p, iter + 1, out);
    }
    int factor(int32_t rank, double* out, uint64_t seed) override {
        if (host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(settle());
        if (iter < nit) return fail(MMW_ERR_STATE, "mmw_factor: run all announced iterations first (the average divides by nit)");
        MMW_TRY(x_csr_view());
        return extras.factor(d_indptr.p, d_col.p, xavg.p, nit, rank, out, seed);
    }
    int round(int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out, int32_t* rem_out) override {
        if (host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(device));
        return extras.round(Zr, Dp, gX, nbatch, randv, z_out, rem_out);
    }
};
template <typename T>
int expm_apply_impl(const Switches& sw, int device, int method, int max_order, double tol, int32_t K, int32_t D, const int32_t* indptr,
                    const int32_t* indices, const double* data, const double* B, double* out, double info[4], int32_t reps,
                    double* kernel_us) {
    MMW_HIP(hipSetDevice(device));
    hipStream_t st;
    MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    ScopedStream guard{st};
    const int64_t nnz = indptr[K];
    std::vector<int32_t> ip(indptr, indptr + K + 1), ci(indices, indices + nnz);
    std::vector<double> vv(data, data + nnz);
    DevBuf<int> d_ip, d_ci;
    DevBuf<T> d_v, d_out;
    DevBuf<double> d_b64, d_o64;
    MMW_TRY(d_ip.upload(ip, st));
    MMW_TRY(d_ci.upload(ci, st));
    MMW_TRY(d_v.upload_cast(vv, st));
    ExpmEngine<T> eng(sw);
    MMW_TRY(eng.init(st, K, D, d_ip.p, d_ci.p, d_v.p));
    eng.method = method; eng.max_order = max_order; eng.tol = tol;
    MMW_TRY(d_out.alloc(eng.bs));
    MMW_TRY(d_b64.alloc((size_t)K * D));
    MMW_TRY(d_o64.alloc((size_t)K * D));
    MMW_TRY(copy_h2d(d_b64.p, B, (size_t)K * D * sizeof(double), st));
    hipEvent_t e0, e1;
    MMW_HIP(hipEventCreate(&e0));
    MMW_HIP(hipEventCreate(&e1));
    double us = 0.0;
    if (reps < 1) reps = 1;
    for (int r = 0; r < reps; ++r) {
        hipLaunchKernelGGL((k_import_block<T>), dim3(grid_elems(eng.bs)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, d_b64.p, eng.start_block());
        MMW_HIP(hipEventRecord(e0, st));
        int rc = eng.apply(d_out.p, 1.0);
        if (rc != MMW_OK) return rc;
        MMW_HIP(hipEventRecord(e1, st));
        MMW_HIP(hipStreamSynchronize(st));
        float ms = 0;
        MMW_HIP(hipEventElapsedTime(&ms, e0, e1));
        us += ms * 1e3;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    hipLaunchKernelGGL((k_export_block<T>), dim3(grid_elems((size_t)K * D)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, d_out.p, d_o64.p);
    MMW_HIP(hipGetLastError());
    MMW_TRY(copy_d2h(out, d_o64.p, (size_t)K * D * sizeof(double), st));
    if (info) {
        info[0] = eng.last.rho; info[1] = eng.last.m_eff > 0 ? eng.last.m_eff : eng.last.m; info[2] = eng.last.nsub; info[3] = eng.last.mu;
    }
    if (kernel_us) *kernel_us = us / reps;
    return MMW_OK;
}
// mmw_create / mmw_create_from_env: a handle of the asked dtype, initialised by `init` (Solver<T>::init or init_env), handed out on success
template <typename Init> int create_solver(mmw_solver** out, int dtype, bool host_only, Init&& init) {
    auto make = [&](auto s) {
        s->host_only = host_only;
        const int rc = init(*s);
        if (rc == MMW_OK) *out = s.release();
        return rc;
    };
    if (dtype == MMW_F32) return make(std::make_unique<Solver<float>>(Switches::from_env()));
    if (dtype == MMW_F64) return make(std::make_unique<Solver<double>>(Switches::from_env()));
    return fail(MMW_ERR_ARG, "dtype must be MMW_F32 or MMW_F64");
}
}  // namespace
