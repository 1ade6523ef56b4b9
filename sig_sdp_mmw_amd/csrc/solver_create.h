// Creation of the solver handle (solver.h): mmw_create (host CSR arrays -> pattern -> uploads), mmw_create_from_env (the generator's device
// state -> pattern on the device) and mmw_create_from_csr (seven CSR arrays on the device -> pattern on the device), and what all share
// once the pattern is on the device: the iterate's buffers, the engine, the buffers the
// parts would otherwise allocate on first use, the locality blockings, the rounding side.  Nothing here is read after the handle is handed
// out except DeviceLists, through which a handle built on the device fetches the lists that only the API's read fields hand out.
#pragma once
#include "csr_device.h"
#include "solver_loop.h"
#include "solver_read.h"
#include "solver_replay.h"

namespace {
template <typename T> struct Solver;
// ---- mmw_create_from_env: the state never leaves the device.  The generator's receive powers are turned into the pattern, its
// per-entry arrays, the edge lists and the row statistics by the kernels of pattern_device.h; the host gets the row pointers (from
// the count pass's prefix sums), the column indices (the blockings read them) and three K-vectors.  The lists that only the
// API's read fields hand out stay on the device until asked for (ensure_host).
struct DeviceLists {  // device copies kept for ensure_host (a handle built on the device, from a generator or from CSR arrays)
    DevBuf<int> st_ptr, st_idx, gain_x, gain_y, asso_x, asso_y, gu_ptr, qu_ptr, so_ptr;
    DevBuf<double> st_val, s_sum, sq_sum;
    bool host_done = true;  // false: H's list vectors are still empty
    template <typename T> int ensure_host(SolverCore<T>& co) {
        if (host_done) return MMW_OK;
        MMW_HIP(hipSetDevice(co.device));
        const size_t nst = (size_t)co.H.n_st, ng = (size_t)co.H.n_gain, na = (size_t)co.H.n_asso;
        co.H.st_indices.resize(nst); co.H.st_data.resize(nst);
        co.H.gain_x.resize(ng); co.H.gain_y.resize(ng); co.H.asso_x.resize(na); co.H.asso_y.resize(na);
        co.H.diag_pos.resize(co.K); co.H.asso_pos.resize(na);
        MMW_TRY(copy_d2h(co.H.st_indices.data(), st_idx.p, nst * sizeof(int32_t), co.st));
        MMW_TRY(copy_d2h(co.H.st_data.data(), st_val.p, nst * sizeof(double), co.st));
        MMW_TRY(copy_d2h(co.H.gain_x.data(), gain_x.p, ng * sizeof(int32_t), co.st));
        MMW_TRY(copy_d2h(co.H.gain_y.data(), gain_y.p, ng * sizeof(int32_t), co.st));
        MMW_TRY(copy_d2h(co.H.asso_x.data(), asso_x.p, na * sizeof(int32_t), co.st));
        MMW_TRY(copy_d2h(co.H.asso_y.data(), asso_y.p, na * sizeof(int32_t), co.st));
        MMW_TRY(copy_d2h(co.H.diag_pos.data(), co.d_diag.p, (size_t)co.K * sizeof(int32_t), co.st));
        MMW_TRY(copy_d2h(co.H.asso_pos.data(), co.d_apos.p, na * sizeof(int32_t), co.st));
        host_done = true;
        return MMW_OK;
    }
};
// Where the rounding side (Extras) of a handle built on the device takes its lists from: Q and h_max are copied device to device; S_gain
// without its diagonal is either compacted here from the generator's CSR (s_*) or already lies in Extras (so_filled: init_csr's fill pass)
struct RoundSource {
    const int* q_ptr = nullptr; const int* q_idx = nullptr; int64_t nnzQ = 0;
    const double* h_max = nullptr;
    const int* s_ptr = nullptr; const int* s_idx = nullptr; const double* s_val = nullptr;
    bool so_filled = false;
};
// Row order of a geometric instance: boustrophedon strips about one block wide (blocking.h: consecutive runs of it are compact patches)
inline std::vector<int32_t> spatial_order(int K, const std::vector<double>& xy, int rows_per_block) {
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
template <typename T> struct SolverCreate {
    static int init(Solver<T>& s, int dev, int32_t K_, int32_t Z_, int32_t rr, double eta_, int32_t nit_, const int32_t* Sp, const int32_t* Si,
                    const double* Sx, const int32_t* Qp, const int32_t* Qi, const double* Qx, const double* h) {
        SolverCore<T>& co = s.core;
        co.device = dev;
        const double t_0 = tnow();
        // The first kernel launch of a process loads the library's code object (~0.15 s): start it on a helper thread now, under
        // the host-side pattern build.
        static std::atomic<bool> module_loading{false};
        std::thread warm_thread;
        if (!co.host_only && !module_loading.exchange(true))
            warm_thread = std::thread([dev]() {
                if (hipSetDevice(dev) != hipSuccess) return;
                float* p = nullptr;
                if (hipMalloc((void**)&p, 256 * sizeof(float)) != hipSuccess) return;
                hipLaunchKernelGGL((k_fill<float>), dim3(1), dim3(BLOCK), 0, (hipStream_t) nullptr, (size_t)256, p, 0.0f);
                (void)hipDeviceSynchronize();
                (void)hipFree(p);
            });
        struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{warm_thread};
        co.bt.want_mfma(K_, Z_ * rr, co.sw);
        const bool start_blk = !co.host_only && !co.sw.no_blocking;
        double t_struct = 0.0;
        std::string err = build_pattern(co.H, K_, Z_, Sp, Si, Sx, Qp, Qi, Qx, h, [&]() {
            t_struct = tnow();
            if (start_blk) co.bt.build_thread = std::thread([pc = &co]() { pc->bt.host_blockings(pc->H, pc->sw); });
        });
        if (!err.empty()) co.bt.join();
        const double t_1 = tnow();
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_create: " + err);
        co.K = K_; co.Z = Z_; co.rank_radio = rr; co.eta = eta_; co.nit = nit_;
        co.D = co.Z * co.rank_radio;
        if (co.host_only) {  // device == -1: pattern inspection only (CPU tests of the host logic)
            std::string lerr;
            if (make_layout(co.D, V16<T>::N, co.eng.lay, lerr) != MMW_OK) return fail(MMW_ERR_ARG, lerr);
            if (live_switch(LIVE_HOST_BLOCKING)) {  // developer aid: build the locality blocking on the host and print its statistics
                report_host_blocking(co.bt.HB, co.H, co.K, blocking_limits<T>(), co.sw);
            }
            if (co.sw.check_blocking) {  // CPU tests: build the blocking and check its invariants
                const BlockingLimits lim = blocking_limits<T>();
                if (co.bt.HB.order.empty()) build_blocking(co.bt.HB, co.K, co.H.l_indptr, co.H.l_indices, lim);
                build_sd_tables(co.bt.HB, co.K, co.H.l_indptr, co.H.l_indices);
                if (!co.bt.HB.order.empty() && !co.bt.HB.blk_rowptr.empty() && co.bt.HB.blk_rowptr.back() == co.K) {
                    const std::string berr = verify_blocking(co.bt.HB, co.K, co.H.l_indptr, co.H.l_indices, lim);
                    if (!berr.empty()) return fail(MMW_ERR_STATE, "blocking invariant violated: " + berr);
                    for (int mrows : {64, 32, 7}) {
                        build_mfma_blocking(co.bt.HB, co.K, co.H.l_indptr, co.H.l_indices, mrows, co.sw.mf_union_cap);
                        const std::string merr = verify_mfma_blocking(co.bt.HB, co.K, co.H.l_indptr, co.H.l_indices);
                        if (!merr.empty()) return fail(MMW_ERR_STATE, "blocking invariant violated: " + merr);
                    }
                }
            }
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(co.device));
        MMW_HIP(hipStreamCreateWithFlags(&co.st, hipStreamNonBlocking));
        MMW_TRY(co.d_indptr.upload(co.H.l_indptr, co.st));
        MMW_TRY(co.d_col.upload(co.H.l_indices, co.st));
        MMW_TRY(co.d_pid.upload(co.H.pid, co.st));
        MMW_TRY(co.d_mirror.upload(co.H.mirror, co.st));
        MMW_TRY(co.d_diag.upload(co.H.diag_pos, co.st));
        MMW_TRY(co.d_apos.upload(co.H.asso_pos, co.st));
        {
            std::vector<int32_t> lrow((size_t)co.H.nnzL());
            for (int k = 0; k < co.K; ++k)
                for (int e = co.H.l_indptr[k]; e < co.H.l_indptr[k + 1]; ++e) lrow[e] = k;
            MMW_TRY(co.d_lrow.upload(lrow, co.st));
        }
        MMW_TRY(co.d_sab.upload_cast(co.H.sab, co.st));
        MMW_TRY(co.d_sba.upload_cast(co.H.sba, co.st));
        MMW_TRY(co.upload_row_vectors());
        return init_common(s, t_0, t_1, t_struct, /*round_src=*/nullptr);
    }
    static int init_env(Solver<T>& s, int dev, EnvDevice& E, int32_t Z_, int32_t rr, double eta_, int32_t nit_) {
        SolverCore<T>& co = s.core;
        DeviceLists& envl = s.envl;
        co.device = dev;
        const double t_0 = tnow();
        if (Z_ < 2) return fail(MMW_ERR_ARG, "mmw_create_from_env: Z must be >= 2 (the constraints divide by Z-1)");
        if (E.K < 2) return fail(MMW_ERR_ARG, "mmw_create_from_env: K must be >= 2");
        MMW_HIP(hipSetDevice(co.device));
        MMW_HIP(hipStreamCreateWithFlags(&co.st, hipStreamNonBlocking));
        MMW_TRY(E.pattern_inputs());  // (cached in the generator: rxT, positions in the AP lists, the count pass)
        co.K = E.K; co.Z = Z_; co.rank_radio = rr; co.eta = eta_; co.nit = nit_;
        co.D = co.Z * co.rank_radio;
        co.H.K = co.K; co.H.Z = co.Z;
        const int A = E.A;
        const int32_t* c6 = E.h_cnt6.data();
        // prefix sums of the count pass
        std::vector<int32_t> st_ptr(co.K + 1, 0), gu_ptr(co.K + 1, 0), qu_ptr(co.K + 1, 0), so_ptr(co.K + 1, 0);
        co.H.l_indptr.assign(co.K + 1, 0);
        for (int k = 0; k < co.K; ++k) {
            co.H.l_indptr[k + 1] = co.H.l_indptr[k] + c6[k];
            st_ptr[k + 1] = st_ptr[k] + c6[(size_t)co.K + k];
            gu_ptr[k + 1] = gu_ptr[k] + c6[(size_t)2 * co.K + k];
            qu_ptr[k + 1] = qu_ptr[k] + c6[(size_t)3 * co.K + k];
            so_ptr[k + 1] = so_ptr[k] + (E.h_sptr[k + 1] - E.h_sptr[k]) - c6[(size_t)4 * co.K + k];
            if ((int64_t)co.H.l_indptr[k] + c6[k] > (int64_t)INT32_MAX) return fail(MMW_ERR_ARG, "mmw_create_from_env: pattern too large for int32 indexing");
        }
        const size_t nnz = (size_t)co.H.l_indptr[co.K], nst = (size_t)st_ptr[co.K], ng = (size_t)gu_ptr[co.K], na = (size_t)qu_ptr[co.K];
        co.H.n_st = (int64_t)nst; co.H.n_gain = (int64_t)ng; co.H.n_asso = (int64_t)na;
        co.H.st_indptr = st_ptr;
        MMW_TRY(co.d_indptr.upload(co.H.l_indptr, co.st));
        MMW_TRY(envl.st_ptr.upload(st_ptr, co.st)); MMW_TRY(envl.gu_ptr.upload(gu_ptr, co.st)); MMW_TRY(envl.qu_ptr.upload(qu_ptr, co.st)); MMW_TRY(envl.so_ptr.upload(so_ptr, co.st));
        MMW_TRY(co.d_col.alloc(nnz)); MMW_TRY(co.d_lrow.alloc(nnz)); MMW_TRY(co.d_sab.alloc(nnz)); MMW_TRY(co.d_sba.alloc(nnz)); MMW_TRY(co.d_pid.alloc(nnz)); MMW_TRY(co.d_mirror.alloc(nnz));
        MMW_TRY(co.d_diag.alloc(co.K)); MMW_TRY(co.d_apos.alloc(na));
        MMW_TRY(envl.st_idx.alloc(nst)); MMW_TRY(envl.st_val.alloc(nst));
        MMW_TRY(envl.gain_x.alloc(ng)); MMW_TRY(envl.gain_y.alloc(ng)); MMW_TRY(envl.asso_x.alloc(na)); MMW_TRY(envl.asso_y.alloc(na));
        MMW_TRY(envl.s_sum.alloc(co.K)); MMW_TRY(envl.sq_sum.alloc(co.K));
        PatOut<T> O;
        O.l_ptr = co.d_indptr.p; O.st_ptr = envl.st_ptr.p; O.gu_ptr = envl.gu_ptr.p; O.qu_ptr = envl.qu_ptr.p; O.appos = E.appos.p;
        O.l_idx = co.d_col.p; O.lrow = co.d_lrow.p; O.sab = co.d_sab.p; O.sba = co.d_sba.p; O.pid = co.d_pid.p; O.diag_pos = co.d_diag.p;
        O.st_idx = envl.st_idx.p; O.st_val = envl.st_val.p;
        O.gain_x = envl.gain_x.p; O.gain_y = envl.gain_y.p; O.asso_x = envl.asso_x.p; O.asso_y = envl.asso_y.p; O.asso_pos = co.d_apos.p;
        hipLaunchKernelGGL((k_pat_fill<T>), dim3(grid_rows(co.K)), dim3(BLOCK), 0, co.st, co.K, A, E.P.thr, E.rx.p, E.rxT.p, E.asso.p, O);
        MMW_HIP(hipGetLastError());
        // the column indices first: the host-side blockings start on them while the device finishes the rest
        co.H.l_indices.resize(nnz);
        MMW_TRY(copy_d2h(co.H.l_indices.data(), co.d_col.p, nnz * sizeof(int32_t), co.st));
        const double t_struct = tnow();
        co.bt.want_mfma(co.K, Z_ * rr, co.sw);
        if (!co.sw.no_blocking) {
            if (!co.sw.env_rcm) {  // (MMW_ENV_RCM=1: the pattern-only order of the CSR entry point, for comparisons)
                co.bt.HB.rcm_cache = spatial_order(co.K, E.h_sta, 64);
                co.bt.HB.grow = false;
            }
            co.bt.build_thread = std::thread([pc = &co]() { pc->bt.host_blockings(pc->H, pc->sw); });
        }
        hipLaunchKernelGGL(k_pat_mirror, dim3(grid_elems(nnz)), dim3(BLOCK), 0, co.st, nnz, co.d_indptr.p, co.d_col.p, co.d_lrow.p, co.d_mirror.p);
        hipLaunchKernelGGL(k_pat_rowstats, dim3(grid_elems((size_t)co.K)), dim3(BLOCK), 0, co.st, co.K, envl.st_ptr.p, envl.st_val.p, envl.s_sum.p, envl.sq_sum.p);
        MMW_HIP(hipGetLastError());
        co.H.S_sum.resize(co.K); co.H.sq_sum.resize(co.K); co.H.h_max.resize(co.K);
        MMW_TRY(copy_d2h(co.H.S_sum.data(), envl.s_sum.p, (size_t)co.K * sizeof(double), co.st));
        MMW_TRY(copy_d2h(co.H.sq_sum.data(), envl.sq_sum.p, (size_t)co.K * sizeof(double), co.st));
        MMW_TRY(copy_d2h(co.H.h_max.data(), E.h_max.p, (size_t)co.K * sizeof(double), co.st));
        co.H.norm_H.assign(co.K, 0.0);
        co.H.cH.assign(co.K, 0.0);
        {
            const std::string err = update_slots(co.H, co.Z);
            if (!err.empty()) {
                co.bt.join();
                return fail(MMW_ERR_ARG, "mmw_create_from_env: " + err);
            }
        }
        MMW_TRY(co.upload_row_vectors());
        envl.host_done = false;
        const double t_1 = tnow();
        RoundSource R;
        R.q_ptr = E.q_ptr.p; R.q_idx = E.q_idx.p; R.nnzQ = E.nnzQ; R.h_max = E.h_max.p;
        R.s_ptr = E.s_ptr.p; R.s_idx = E.s_idx.p; R.s_val = E.s_val.p;
        return init_common(s, t_0, t_1, t_struct, &R);
    }
    // ---- mmw_create_from_csr: build_pattern on the device, from seven CSR arrays that lie there (pattern_csr_device.h).  Three round trips:
    // {validation verdict, row counts of S}, {row statistics, row counts of L}, {the column indices, for the host-side blockings}.
    static int init_csr(Solver<T>& s, CsrDevice& Cs, int32_t Z_, int32_t rr, double eta_, int32_t nit_) {
        const char* who = "mmw_create_from_csr";
        SolverCore<T>& co = s.core;
        DeviceLists& dl = s.envl;
        const CsrView V = Cs.V;
        const int K = V.K;
        if (co.host_only) {  // device -1: the shared per-row checks in a plain loop, then build_pattern on the host copies
            MMW_TRY(Cs.validate(who));
            return init(s, -1, K, Z_, rr, eta_, nit_, V.Sp, V.Si, V.Sx, V.Qp, V.Qi, V.Qx, V.h);
        }
        co.device = Cs.device;
        const double t_0 = tnow();
        MMW_HIP(hipSetDevice(co.device));
        MMW_HIP(hipStreamCreateWithFlags(&co.st, hipStreamNonBlocking));
        const int gk = grid_rows(K);
        const size_t Ks = (size_t)K;
        // validation (unless the state already has its verdict) and the first count pass, which runs only if every check passed
        if (Cs.checked) MMW_TRY(Cs.verdict(who));
        else MMW_TRY(Cs.enqueue_checks(co.st));
        DevBuf<int> cnt, nfnew;  // cnt: [4][K] = n_so, n_f, st_cnt, n_qu; later n_l, n_gu, the placement cursors
        MMW_TRY(cnt.alloc(4 * Ks)); MMW_TRY(nfnew.alloc(Ks));
        MMW_HIP(hipMemsetAsync(cnt.p, 0, 4 * Ks * sizeof(int), co.st));
        hipLaunchKernelGGL(k_csrpat_count, dim3(gk), dim3(BLOCK), 0, co.st, V, (const unsigned long long*)Cs.d_err.p, cnt.p, cnt.p + Ks, cnt.p + 2 * Ks, cnt.p + 3 * Ks);
        MMW_HIP(hipGetLastError());
        if (!Cs.checked) {
            MMW_TRY(copy_d2h(Cs.err, Cs.d_err.p, sizeof Cs.err, co.st));
            Cs.checked = true;
            MMW_TRY(Cs.verdict(who));
        }
        if (K < 2) return fail(MMW_ERR_ARG, std::string(who) + ": K must be >= 2");
        if (Z_ < 2) return fail(MMW_ERR_ARG, std::string(who) + ": Z must be >= 2 (the constraints divide by Z-1)");
        std::vector<int32_t> h_cnt(4 * Ks);
        MMW_TRY(copy_d2h(h_cnt.data(), cnt.p, h_cnt.size() * sizeof(int32_t), co.st));
        std::vector<int32_t> so_ptr(Ks + 1, 0), f_ptr(Ks + 1, 0), st_ptr(Ks + 1, 0), qu_ptr(Ks + 1, 0), gu_ptr(Ks + 1, 0);
        for (size_t k = 0; k < Ks; ++k) {  // (every total is at most nnz(S) or nnz(Q): int32)
            so_ptr[k + 1] = so_ptr[k] + h_cnt[k];
            f_ptr[k + 1] = f_ptr[k] + h_cnt[Ks + k];
            st_ptr[k + 1] = st_ptr[k] + h_cnt[2 * Ks + k];
            qu_ptr[k + 1] = qu_ptr[k] + h_cnt[3 * Ks + k];
        }
        const size_t nso = (size_t)so_ptr[K], nst = (size_t)st_ptr[K], na = (size_t)qu_ptr[K];
        if ((size_t)f_ptr[K] != nst) return fail(MMW_ERR_STATE, std::string(who) + ": internal: the transpose lost entries");
        DevBuf<int> d_fptr, f_idx, fx, tmp_idx;
        DevBuf<double> f_val, tmp_val;
        Extras<T>& ex = s.extras;
        MMW_TRY(dl.so_ptr.upload(so_ptr, co.st)); MMW_TRY(d_fptr.upload(f_ptr, co.st)); MMW_TRY(dl.st_ptr.upload(st_ptr, co.st)); MMW_TRY(dl.qu_ptr.upload(qu_ptr, co.st));
        MMW_TRY(ex.so_indices.alloc(nso)); MMW_TRY(ex.so_data.alloc(nso)); MMW_TRY(ex.so_hmax.alloc(nso));
        MMW_TRY(f_idx.alloc(nst)); MMW_TRY(f_val.alloc(nst)); MMW_TRY(fx.alloc(nst)); MMW_TRY(tmp_idx.alloc(nst)); MMW_TRY(tmp_val.alloc(nst));
        MMW_TRY(dl.st_idx.alloc(nst)); MMW_TRY(dl.st_val.alloc(nst)); MMW_TRY(dl.s_sum.alloc(Ks)); MMW_TRY(dl.sq_sum.alloc(Ks));
        int* cursor = cnt.p + 2 * Ks;
        MMW_HIP(hipMemsetAsync(cursor, 0, Ks * sizeof(int), co.st));
        hipLaunchKernelGGL(k_csrpat_fill, dim3(gk), dim3(BLOCK), 0, co.st, V, (const int*)dl.so_ptr.p, (const int*)d_fptr.p, (const int*)dl.st_ptr.p, cursor, ex.so_indices.p,
                           ex.so_data.p, ex.so_hmax.p, f_idx.p, f_val.p, tmp_idx.p, tmp_val.p);
        hipLaunchKernelGGL(k_csrpat_sort_rows, dim3(gk), dim3(BLOCK), 0, co.st, K, (const int*)dl.st_ptr.p, (const int*)tmp_idx.p, (const double*)tmp_val.p, dl.st_idx.p, dl.st_val.p);
        hipLaunchKernelGGL(k_pat_rowstats, dim3(grid_elems(Ks)), dim3(BLOCK), 0, co.st, K, dl.st_ptr.p, dl.st_val.p, dl.s_sum.p, dl.sq_sum.p);
        hipLaunchKernelGGL(k_csrpat_count_L, dim3(gk), dim3(BLOCK), 0, co.st, V, (const int*)dl.st_ptr.p, (const int*)dl.st_idx.p, (const int*)d_fptr.p, (const int*)f_idx.p, fx.p,
                           nfnew.p, cnt.p, cnt.p + Ks);
        MMW_HIP(hipGetLastError());
        co.K = K; co.Z = Z_; co.rank_radio = rr; co.eta = eta_; co.nit = nit_;
        co.D = co.Z * co.rank_radio;
        co.H.K = K; co.H.Z = Z_;
        co.H.S_sum.resize(Ks); co.H.sq_sum.resize(Ks); co.H.h_max.resize(Ks);
        MMW_TRY(copy_d2h(co.H.S_sum.data(), dl.s_sum.p, Ks * sizeof(double), co.st));
        MMW_TRY(copy_d2h(co.H.sq_sum.data(), dl.sq_sum.p, Ks * sizeof(double), co.st));
        MMW_TRY(copy_d2h(co.H.h_max.data(), V.h, Ks * sizeof(double), co.st));
        MMW_TRY(copy_d2h(h_cnt.data(), cnt.p, 2 * Ks * sizeof(int32_t), co.st));
        co.H.norm_H.assign(Ks, 0.0);
        co.H.cH.assign(Ks, 0.0);
        co.H.n_st = (int64_t)nst; co.H.n_asso = (int64_t)na;
        co.H.st_indptr = st_ptr;
        {
            const std::string err = update_slots(co.H, co.Z);
            if (!err.empty()) return fail(MMW_ERR_ARG, std::string(who) + ": " + err);
        }
        co.H.l_indptr.assign(Ks + 1, 0);
        for (size_t k = 0; k < Ks; ++k) {
            if ((int64_t)co.H.l_indptr[k] + h_cnt[k] > (int64_t)INT32_MAX) return fail(MMW_ERR_ARG, std::string(who) + ": pattern too large for int32 indexing");
            co.H.l_indptr[k + 1] = co.H.l_indptr[k] + h_cnt[k];
            gu_ptr[k + 1] = gu_ptr[k] + h_cnt[Ks + k];
        }
        const size_t nnz = (size_t)co.H.l_indptr[K], ng = (size_t)gu_ptr[K];
        co.H.n_gain = (int64_t)ng;
        MMW_TRY(co.d_indptr.upload(co.H.l_indptr, co.st)); MMW_TRY(dl.gu_ptr.upload(gu_ptr, co.st));
        MMW_TRY(co.d_col.alloc(nnz)); MMW_TRY(co.d_lrow.alloc(nnz)); MMW_TRY(co.d_sab.alloc(nnz)); MMW_TRY(co.d_sba.alloc(nnz)); MMW_TRY(co.d_pid.alloc(nnz)); MMW_TRY(co.d_mirror.alloc(nnz));
        MMW_TRY(co.d_diag.alloc(Ks)); MMW_TRY(co.d_apos.alloc(na));
        MMW_TRY(dl.gain_x.alloc(ng)); MMW_TRY(dl.gain_y.alloc(ng)); MMW_TRY(dl.asso_x.alloc(na)); MMW_TRY(dl.asso_y.alloc(na));
        DevBuf<int> internal;
        MMW_TRY(internal.alloc(1));
        MMW_HIP(hipMemsetAsync(internal.p, 0, sizeof(int), co.st));
        CsrPatOut<T> O;
        O.l_ptr = co.d_indptr.p; O.st_ptr = dl.st_ptr.p; O.f_ptr = d_fptr.p; O.qu_ptr = dl.qu_ptr.p;
        O.st_idx = dl.st_idx.p; O.st_val = dl.st_val.p; O.f_idx = f_idx.p; O.f_val = f_val.p; O.fx = fx.p; O.n_fnew = nfnew.p;
        O.l_idx = co.d_col.p; O.lrow = co.d_lrow.p; O.sab = co.d_sab.p; O.sba = co.d_sba.p; O.pid = co.d_pid.p; O.diag_pos = co.d_diag.p;
        O.asso_x = dl.asso_x.p; O.asso_y = dl.asso_y.p; O.asso_pos = co.d_apos.p; O.internal = internal.p;
        hipLaunchKernelGGL((k_csrpat_fill_L<T>), dim3(gk), dim3(BLOCK), 0, co.st, V, O);
        MMW_HIP(hipGetLastError());
        // the column indices first: the host-side blockings (mmw_create's own: the pattern-only order, grown blocks) start on them while the
        // device finishes the rest
        co.H.l_indices.resize(nnz);
        MMW_TRY(copy_d2h(co.H.l_indices.data(), co.d_col.p, nnz * sizeof(int32_t), co.st));
        const double t_struct = tnow();
        co.bt.want_mfma(K, Z_ * rr, co.sw);
        if (!co.sw.no_blocking) co.bt.build_thread = std::thread([pc = &co]() { pc->bt.host_blockings(pc->H, pc->sw); });
        hipLaunchKernelGGL(k_csrpat_gain_edges, dim3(gk), dim3(BLOCK), 0, co.st, K, (const int*)co.d_indptr.p, (const int*)co.d_col.p, (const int*)co.d_pid.p, (const int*)dl.gu_ptr.p,
                           dl.gain_x.p, dl.gain_y.p);
        hipLaunchKernelGGL(k_pat_mirror, dim3(grid_elems(nnz)), dim3(BLOCK), 0, co.st, nnz, co.d_indptr.p, co.d_col.p, co.d_lrow.p, co.d_mirror.p);
        MMW_HIP(hipGetLastError());
        int h_internal = 0;
        MMW_TRY(copy_d2h(&h_internal, internal.p, sizeof(int), co.st));
        if (h_internal) {
            co.bt.join();
            return fail(MMW_ERR_ARG, std::string(who) + ": internal: gain edge on an association pair");
        }
        MMW_TRY(co.upload_row_vectors());
        dl.host_done = false;
        const double t_1 = tnow();
        RoundSource R;
        R.q_ptr = V.Qp; R.q_idx = V.Qi; R.nnzQ = V.nnzQ; R.h_max = V.h; R.so_filled = true;
        return init_common(s, t_0, t_1, t_struct, &R);
    }
    static int init_extras_device(SolverCore<T>& co, DeviceLists& envl, Extras<T>& extras, const RoundSource& R) {
        MMW_TRY(extras.init_device(co.st, co.K, &co.kt));
        std::vector<int32_t> so_ptr_h((size_t)co.K + 1);
        MMW_TRY(copy_d2h(so_ptr_h.data(), envl.so_ptr.p, so_ptr_h.size() * sizeof(int32_t), co.st));
        const size_t nso = (size_t)so_ptr_h[co.K];
        MMW_TRY(extras.so_indptr.upload(so_ptr_h, co.st));
        MMW_TRY(extras.q_indptr.alloc((size_t)co.K + 1)); MMW_TRY(extras.q_indices.alloc((size_t)R.nnzQ)); MMW_TRY(extras.h_max.alloc(co.K));
        if (!R.so_filled) {
            MMW_TRY(extras.so_indices.alloc(nso)); MMW_TRY(extras.so_data.alloc(nso)); MMW_TRY(extras.so_hmax.alloc(nso));
            hipLaunchKernelGGL(k_pat_so_fill, dim3(grid_rows(co.K)), dim3(BLOCK), 0, co.st, co.K, R.s_ptr, R.s_idx, R.s_val, (const int*)extras.so_indptr.p, R.h_max,
                               extras.so_indices.p, extras.so_data.p, extras.so_hmax.p);
            MMW_HIP(hipGetLastError());
        }
        MMW_HIP(hipMemcpyAsync(extras.q_indptr.p, R.q_ptr, ((size_t)co.K + 1) * sizeof(int), hipMemcpyDeviceToDevice, co.st));
        if (R.nnzQ) MMW_HIP(hipMemcpyAsync(extras.q_indices.p, R.q_idx, (size_t)R.nnzQ * sizeof(int), hipMemcpyDeviceToDevice, co.st));
        MMW_HIP(hipMemcpyAsync(extras.h_max.p, R.h_max, (size_t)co.K * sizeof(double), hipMemcpyDeviceToDevice, co.st));
        MMW_HIP(hipStreamSynchronize(co.st));
        return MMW_OK;
    }
    // ---- everything after the pattern is on the device: the iterate's buffers, the engine, the blockings, the rounding side
    static int init_common(Solver<T>& s, double t_0, double t_1, double t_struct, const RoundSource* round_src) {
        SolverCore<T>& co = s.core;
        const bool verbose = live_switch(LIVE_VERBOSE);
        MMW_TRY(co.alloc_iterate());
        MMW_TRY(s.loop.alloc_scratch(co));
        MMW_TRY(co.eng.init(co.st, co.K, co.D, co.d_indptr.p, co.d_col.p, co.lval.p));
        co.kt.st = co.st;
        co.eng.kt = &co.kt;
        co.eng.max_order = 12;
        co.eng.tol = sizeof(T) == 4 ? 1e-6 : 1e-9;
        MMW_TRY(co.Xh.alloc(co.eng.bs));
        MMW_TRY(prealloc(co, s.pending, s.loop, s.extras));
        const double t_2 = tnow();
        MMW_TRY(setup_blocking(co, s.loop, s.extras));
        const double t_3 = tnow();
        if (verbose) fprintf(stderr, "[create] pattern %.1f ms (structure after %.1f), uploads+alloc %.1f ms, blocking %.1f ms\n", (t_1 - t_0) * 1e3, (t_struct - t_0) * 1e3, (t_2 - t_1) * 1e3, (t_3 - t_2) * 1e3);
        MMW_TRY(s.reads.resize(co));
        MMW_TRY(s.loop.resize(co));
        MMW_HIP(hipStreamSynchronize(co.st));
        if (round_src) MMW_TRY(init_extras_device(co, s.envl, s.extras, *round_src));
        else MMW_TRY(s.extras.init(co.st, &co.H, co.K, &co.kt));
        return s.reset(co.nit);
    }
    // Buffers the loop, the factor and the rounding would otherwise allocate on first use (hipMalloc is a synchronous driver call
    // of 0.1 - 3 ms, and the first probe of a search pays all of them inside its timed phases): reserved here, while the
    // blocking thread is still at work and this thread would only wait for it.
    static int prealloc(SolverCore<T>& co, PendingChunk<T>& pending, SolverLoop<T>& loop, Extras<T>& extras) {
        const size_t nnz = (size_t)co.H.nnzL(), C = (size_t)co.H.C();
        for (DevBuf<T>* b : {&pending.sn_lval, &pending.sn_xval, &pending.sn_xavg}) MMW_TRY(b->alloc(nnz));
        for (DevBuf<T>* b : {&pending.sn_Y, &pending.sn_yavg, &pending.sn_eaccu, &loop.yun}) MMW_TRY(b->alloc(C));
        MMW_TRY(pending.sn_plan.alloc(1));
        // Krylov basis: the first iterations of a run ask for 2 - 3 steps before the a-posteriori estimate settles on fewer; growing
        // the basis there costs an allocation, a copy and two device synchronisations each time
        if ((double)co.eng.bs * sizeof(T) * 4.0 < 8.0e9) MMW_TRY(co.eng.ensure_blocks(std::min(4, co.eng.max_order + 1)));
        if (co.bt.blk_want_mf && (co.eng.lay.Dpad % 32) == 0) {
            MMW_TRY(loop.xh_planes.alloc(2 * co.eng.bs));
            MMW_TRY(co.eng.reserve_planes());
        }
        const int rank = std::min(co.K - 1, (co.Z - 1) * co.rank_radio);  // what the host class asks mmw_factor for (mmw.py:206)
        if (rank >= 1) {
            MMW_TRY(extras.fac_reserve(co.st, co.K, rank, co.bt.blk_want_mf));
            if ((size_t)10 * co.K * co.Z * sizeof(double) <= ((size_t)2 << 30)) MMW_TRY(extras.round_reserve(co.K, co.Z, rank, 10));  // sdp_solver.rounding's 10 attempts
        }
        return MMW_OK;
    }
    static int setup_blocking(SolverCore<T>& co, SolverLoop<T>& loop, Extras<T>& extras) {
        if (co.sw.no_blocking) return MMW_OK;
        if (co.bt.build_thread.joinable()) co.bt.build_thread.join();  // started under the pattern build (init)
        else co.bt.host_blockings(co.H, co.sw);
        if (co.bt.blk_want_mf && live_switch(LIVE_VERBOSE))
            fprintf(stderr, "[mmw] matrix-core blocking: ok %d blocks %d rows/block %.1f reuse %.2f row tiles %d k-steps %d\n", (int)co.bt.HB.fits_mfma, co.bt.HB.nbm(),
                    (double)co.K / std::max(1, co.bt.HB.nbm()), co.bt.HB.m_reuse, co.bt.HB.mfma_mt, co.bt.HB.kbase.empty() ? 0 : co.bt.HB.kbase.back());
        if (live_switch(LIVE_VERBOSE))
            fprintf(stderr, "[mmw] blocking: usable %d half-tile %d blocks %d rows/block %.1f union/block %.1f entries %lld (nnz %lld, +%.1f%% padding) sd_max %d\n",
                    (int)co.bt.HB.usable, (int)co.bt.HB.fits_half_tile, co.bt.HB.nb(), (double)co.K / std::max(1, co.bt.HB.nb()), (double)co.bt.HB.un_cols.size() / std::max(1, co.bt.HB.nb()),
                    (long long)co.bt.HB.nent, (long long)co.H.nnzL(), 100.0 * ((double)co.bt.HB.nent / (double)co.H.nnzL() - 1.0), co.bt.HB.sd_max);
        if (!co.bt.HB.usable) return MMW_OK;
        MMW_TRY(co.bt.upload(co.st, co.H, co.K, co.sw, co.d_apos.p));
        if (sizeof(T) == 4 && co.bt.HB.fits_mfma) {
            co.eng.use_mfma = true;
            co.eng.mf.nb = co.bt.HB.nbm();
            co.eng.mf.desc = co.bt.b_mdesc.p;
            co.eng.mf.un_fixed = co.bt.b_munfixed.p;
            co.eng.mf.order = co.bt.b_morder.p;
            co.eng.mf.kbase = co.bt.b_kbase.p;
            co.eng.mf.afrag = co.bt.afrag.p;
            co.eng.mf_mt = co.bt.HB.mfma_mt;
            if (co.bt.sddmm_mfma) {  // X in tile order and the fixed-point row totals, for the matrix-core SDDMM
                MMW_TRY(co.x.xs_val.alloc(co.bt.n_xs));
                MMW_TRY(co.x.xs_avg.alloc(co.bt.n_xs));
                MMW_TRY(loop.rsfx.alloc((size_t)2 * co.K));
            }
            if ((size_t)co.bt.HB.nbm() > (size_t)MAX_PART && co.bt.HB.nbm() > co.bt.HB.nb()) {
                MMW_TRY(co.eng.partial.alloc((size_t)co.bt.HB.nbm() * co.eng.lay.Dpad));
                MMW_TRY(co.eng.partial_o2.alloc((size_t)co.bt.HB.nbm() * co.eng.lay.Dpad));
            }
        }
        if (!co.bt.sddmm_mfma) MMW_TRY(co.bt.ensure_sd(co.st, co.H, co.K, co.eng.lay.Dpad, co.sw.full_tile));
        MMW_HIP(hipStreamSynchronize(co.st));
        extras.fac.set_blocking(co.blkdev(), co.bt.b_bepos.p, co.bt.HB.nent);
        if (co.eng.use_mfma) extras.fac.set_mfma(co.eng.mf, co.bt.HB.mfma_mt, co.bt.b_fpos.p, co.bt.afrag_n, (int64_t)co.H.nnzL());
        co.eng.blk_stale = &co.lblk_stale;
        co.eng.blk_refresh = [pc = &co]() -> int {
            hipLaunchKernelGGL((k_gather_blocked<T>), dim3(grid_elems((size_t)pc->bt.HB.nent)), dim3(BLOCK), 0, pc->st, (size_t)pc->bt.HB.nent, pc->bt.b_bepos.p, pc->lval.p, pc->bt.lval_blk.p);
            MMW_HIP(hipGetLastError());
            return MMW_OK;
        };
        return co.eng.enable_blocking(co.blkdev(), co.bt.lval_blk.p);
    }
};
}  // namespace
