// Rounding, epilogue factor and duality-gap routines that hang off a solver handle.
#pragma once
#include "factor.h"
#include "kernels_factor_random.h"
#include "kernels_round.h"
#include "kernels_round_draw.h"
#include "pattern.h"
#include "pattern_device.h"
#include "runtime.h"

namespace mmw {

template <typename T> struct Extras {
    const Switches& sw;
    explicit Extras(const Switches& s) : sw(s), fac(s) {}
    hipStream_t st = nullptr;
    const HostPattern* H = nullptr;
    KernelTimers* kt = nullptr;
    int K = 0;
    // rounding-side state (float64 whatever T is)
    DevBuf<int> so_indptr, so_indices, q_indptr, q_indices;
    DevBuf<double> so_data, h_max, so_hmax;  // so_hmax[e] = h_max[so_indices[e]]: the greedy reads it like so_data
    DevBuf<GreedyHdr> ghdr;
    DevBuf<double> gX, randv, P, gain, nrm;
    DevBuf<int> pref, slot, order, rem, rank_part, gsched, gnsteps;
    DevBuf<unsigned> gmask;
    DevBuf<GreedyHdr> ghdr_s;  // [steps][GB_WAVES]: the users' headers in schedule order
    Factorizer<T> fac;
    // gap work
    DevBuf<T> g_x, g_l, g_y, g_e1, g_e2, g_r, g_vec, g_tm;
    DevBuf<double> g_part, g_scal, g_lz, g_colsum;

    // the rounding's state straight from the device generator (mmw_create_from_env): so_* / q_* / h_max are filled by the caller's kernels
    int init_device(hipStream_t s, int K_, KernelTimers* k) {
        st = s; H = nullptr; K = K_; kt = k;
        MMW_TRY(ghdr.alloc((size_t)K));
        return fac.init(st, K, kt);
    }
    int init(hipStream_t s, const HostPattern* h, int K_, KernelTimers* k) {
        st = s; H = h; K = K_; kt = k;
        MMW_TRY(so_indptr.upload(H->so_indptr, st));
        MMW_TRY(so_indices.upload(H->so_indices, st));
        MMW_TRY(so_data.upload(H->so_data, st));
        {
            std::vector<double> hm(H->so_indices.size());
            for (size_t e = 0; e < hm.size(); ++e) hm[e] = H->h_max[H->so_indices[e]];
            MMW_TRY(so_hmax.upload(hm, st));
        }
        MMW_TRY(ghdr.alloc((size_t)K));
        MMW_TRY(q_indptr.upload(H->q_indptr, st));
        MMW_TRY(q_indices.upload(H->q_indices, st));
        MMW_TRY(h_max.upload(H->h_max, st));
        MMW_HIP(hipStreamSynchronize(st));
        return fac.init(st, K, kt);
    }
    template <typename B> static int ensure(DevBuf<B>& b, size_t n) {
        if (b.n >= n && b.p) return MMW_OK;
        return b.alloc(n);
    }

    // ---- LOG_GAP (mmw.py:79-117): nterms = number of X / Y terms in the running sums
    int gap(const PatternDev<T>& P, const int* lrow, const T* xavg, const T* yavg, int nterms, double out[3]) {
        const size_t nnz = (size_t)P.nnzL, C = (size_t)P.C;
        const int gr = grid_rows(K);
        MMW_TRY(ensure(g_x, nnz)); MMW_TRY(ensure(g_l, nnz)); MMW_TRY(ensure(g_y, C)); MMW_TRY(ensure(g_e1, C)); MMW_TRY(ensure(g_e2, C));
        MMW_TRY(ensure(g_r, K)); MMW_TRY(ensure(g_part, ROW_GRID_MAX)); MMW_TRY(ensure(g_scal, 8));
        const double inv = 1.0 / (double)nterms;
        hipLaunchKernelGGL((k_scaled_copy<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, xavg, inv, g_x.p);
        hipLaunchKernelGGL((k_scaled_copy<T>), dim3(grid_elems(C)), dim3(BLOCK), 0, st, C, yavg, inv, g_y.p);
        // violations at Xbar: reuse the DUAL kernels with a zero accumulator and eta = 1 -> block maxima of e
        MMW_HIP(hipMemsetAsync(g_e2.p, 0, C * sizeof(T), st));
        hipLaunchKernelGGL((k_dual_rows<T>), dim3(gr), dim3(BLOCK), 0, st, P, g_x.p, g_r.p, g_e1.p);
        hipLaunchKernelGGL((k_dual_h<T>), dim3(gr), dim3(BLOCK), 0, st, P, g_r.p, g_e1.p, g_e2.p, 1.0, g_part.p);
        hipLaunchKernelGGL(k_max_reduce, dim3(1), dim3(BLOCK), 0, st, gr, g_part.p, g_scal.p + 4);
        // L(Ybar) on the pattern
        hipLaunchKernelGGL((k_ysums<T>), dim3(1), dim3(BLOCK), 0, st, K, P.E_asso, g_y.p, P.cH, P.inv_norm_H, g_scal.p);
        MMW_HIP(hipMemsetAsync(g_l.p, 0, nnz * sizeof(T), st));
        hipLaunchKernelGGL((k_hweights<T>), dim3(grid_elems((size_t)K)), dim3(BLOCK), 0, st, K, g_y.p + (K + P.E_asso), P.inv_norm_H, g_r.p);  // g_r is free again
        hipLaunchKernelGGL((k_loss<T>), dim3(gr), dim3(BLOCK), 0, st, P, lrow, g_y.p, g_r.p, g_scal.p, g_l.p, -1.0, (const int*)nullptr, (T*)nullptr);
        MMW_HIP(hipGetLastError());
        double emax = 0.0;
        MMW_HIP(hipMemcpyAsync(&emax, g_scal.p + 4, sizeof(double), hipMemcpyDeviceToHost, st));
        double lam = 0.0;
        MMW_TRY(lambda_min(P.indptr, P.col, g_l.p, &lam));
        MMW_HIP(hipStreamSynchronize(st));
        out[0] = emax;
        out[1] = lam * (double)K;
        out[2] = out[0] - out[1];
        return MMW_OK;
    }

    // smallest eigenvalue of the symmetric matrix (pattern, val): plain Lanczos (the extreme Ritz value of the
    // three-term recurrence converges to lambda_min with or without reorthogonalisation), tridiagonal on the host
    int lambda_min(const int* indptr, const int* col, const T* val, double* lam) {
        BlockLayout lay;
        std::string err;
        MMW_TRY(make_layout(1, V16<T>::N, lay, err));
        const int Dp = lay.Dpad;
        const size_t bs = (size_t)K * Dp;
        const int m_max = std::min(K, 600), chunk = 20;
        MMW_TRY(ensure(g_vec, 3 * bs)); MMW_TRY(ensure(g_tm, bs));
        MMW_TRY(ensure(g_lz, (size_t)4 * (m_max + 3) * Dp));
        MMW_TRY(ensure(g_colsum, Dp));
        DevBuf<double>& part = fac.partial;
        if (part.n < (size_t)MAX_PART * Dp) MMW_TRY(part.alloc((size_t)MAX_PART * std::max(Dp, 4)));
        LanczosScalars S;
        const size_t n = (size_t)(m_max + 3) * Dp;
        S.alpha = g_lz.p; S.beta = g_lz.p + n; S.sinv = g_lz.p + 2 * n; S.coef = g_lz.p + 3 * n;
        const int nblk = grid_slabs(K), gr = grid_slabs(K * 4);
        const size_t shcol = (size_t)BLOCK * sizeof(double);
        auto blk = [&](int j) { return g_vec.p + (size_t)((j - 1) % 3) * bs; };
        const double eps = sizeof(T) == 4 ? 1e-6 : 1e-14;
        // deterministic start vector: Philox normals, one column
        hipLaunchKernelGGL((k_sketch_rng<T>), dim3(nblk), dim3(BLOCK), 0, st, K, 1, Dp, 0x6a09e667f3bcc908ull, 7u, blk(1), (double*)nullptr);
        // rows are normalised to +-1 by the sketch kernel; that is a fine start vector
        hipLaunchKernelGGL((k_colsq<T>), dim3(gr), dim3(BLOCK), shcol, st, K, Dp, blk(1), part.p);
        hipLaunchKernelGGL((k_colreduce<LZ_INIT>), dim3((Dp + 15) / 16), dim3(1024), 0, st, gr, Dp, part.p, g_colsum.p, 0, eps, S, (const ExpmPlan*)nullptr);
        std::vector<double> a, b, ha((size_t)(m_max + 3) * Dp), hb((size_t)(m_max + 3) * Dp);
        const double tol = sizeof(T) == 4 ? 1e-5 : 1e-11;
        double theta = 0.0;
        int j = 1;
        while (j <= m_max) {
            const int jend = std::min(m_max, j + chunk - 1);
            for (; j <= jend; ++j) {
                MMW_TRY((spmm_launch<T, SPMM_LANCZOS>(st, sw, K, lay, nblk, indptr, col, val, blk(j), g_tm.p, nullptr, nullptr, 1.0, 0.0, 1.0, part.p)));
                hipLaunchKernelGGL((k_colreduce<LZ_ALPHA>), dim3((Dp + 15) / 16), dim3(1024), 0, st, nblk, Dp, part.p, g_colsum.p, j, eps, S, (const ExpmPlan*)nullptr);
                hipLaunchKernelGGL((k_lz_update<T>), dim3(gr), dim3(BLOCK), shcol, st, K, Dp, j, g_tm.p, blk(j), j > 1 ? blk(j - 1) : blk(j), blk(j + 1), S, part.p, (const ExpmPlan*)nullptr);
                hipLaunchKernelGGL((k_colreduce<LZ_BETA>), dim3((Dp + 15) / 16), dim3(1024), 0, st, gr, Dp, part.p, g_colsum.p, j, eps, S, (const ExpmPlan*)nullptr);
            }
            MMW_HIP(hipGetLastError());
            const int m = j - 1;
            MMW_HIP(hipMemcpyAsync(ha.data(), S.alpha, (size_t)(m + 1) * Dp * sizeof(double), hipMemcpyDeviceToHost, st));
            MMW_HIP(hipMemcpyAsync(hb.data(), S.beta, (size_t)(m + 1) * Dp * sizeof(double), hipMemcpyDeviceToHost, st));
            MMW_HIP(hipStreamSynchronize(st));
            a.assign(m, 0.0);
            b.assign(m, 0.0);
            int mm = m;
            for (int i = 1; i <= m; ++i) {
                a[i - 1] = ha[(size_t)i * Dp];
                b[i - 1] = hb[(size_t)i * Dp];  // beta_i couples i and i+1
                if (i < m && b[i - 1] == 0.0) {  // invariant subspace found
                    mm = i;
                    break;
                }
            }
            double lastc = 0.0;
            theta = tridiag_min_eig(a, b, mm, &lastc);
            double scale = 0.0;
            for (int i = 0; i < mm; ++i) scale = std::max(scale, std::fabs(a[i]) + (i < mm - 1 ? std::fabs(b[i]) : 0.0));
            const double resid = std::fabs(b[mm - 1] * lastc);
            if (mm < m || resid <= tol * std::max(scale, 1e-300) || m >= K) break;
        }
        *lam = theta;
        return MMW_OK;
    }

    int factor(const int* indptr, const int* col, const T* xavg, int nit, int32_t rank, double* out, uint64_t seed) {
        const int rc = fac.run(indptr, col, xavg, 1.0 / (double)nit, rank, seed, out);
        if (rc == MMW_OK) spec_live = false;  // (MMW_F_FACTOR_ROWNORM belongs to a spectral factor)
        return rc;
    }

    // ---- the spectral baseline (sdp_solver.py:165-185; kernels_spectral.h): the Laplacian of S_gain + S_gain^T as a second value vector
    // on the L pattern, built on the first call that asks for it, and the factor's own iteration on it with the eigenvector export
    DevBuf<double> lap64, spec_rownorm;
    DevBuf<T> lapT;  // fp32 handles: the values narrowed for the products (fp64 handles read lap64)
    bool lap_ready = false;
    bool spec_live = false;      // out64 holds a spectral block: MMW_F_FACTOR_ROWNORM answers
    double spec_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> spec_eig;
    int ensure_laplacian(const int* indptr, const int* col, const int* diag_pos, size_t nnz) {
        if (lap_ready) return MMW_OK;
        MMW_TRY(lap64.alloc(nnz));
        hipLaunchKernelGGL(k_lap_fill, dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, indptr, col, diag_pos, (const int*)so_indptr.p, (const int*)so_indices.p,
                           (const double*)so_data.p, lap64.p);
        MMW_HIP(hipGetLastError());
        if constexpr (sizeof(T) == 4) {
            MMW_TRY(lapT.alloc(nnz));
            hipLaunchKernelGGL((k_lap_narrow<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, (const double*)lap64.p, lapT.p);
            MMW_HIP(hipGetLastError());
        }
        lap_ready = true;
        return MMW_OK;
    }
    int read_laplacian(const int* indptr, const int* col, const int* diag_pos, size_t nnz, double* out, int64_t n) {
        if ((int64_t)nnz != n) return fail(MMW_ERR_ARG, "mmw_read_f64(LAPLACIAN): wrong length " + std::to_string(n) + ", expected " + std::to_string(nnz));
        MMW_TRY(ensure_laplacian(indptr, col, diag_pos, nnz));
        return copy_d2h(out, lap64.p, nnz * sizeof(double), st);
    }
    int factor_spectral(const int* indptr, const int* col, const int* diag_pos, size_t nnz, int32_t Z, int index_order, double* out, uint64_t seed) {
        MMW_TRY(ensure_laplacian(indptr, col, diag_pos, nnz));
        MMW_TRY(ensure(spec_rownorm, (size_t)K));
        EigExport eig;
        eig.index_order = index_order;
        eig.rownorm = spec_rownorm.p;
        const T* val;
        if constexpr (sizeof(T) == 4) val = lapT.p;
        else val = lap64.p;
        MMW_TRY(fac.run(indptr, col, val, 1.0, Z, seed, out, &eig));  // (a refused or failed call exports nothing: the last factor stands)
        spec_live = true;
        spec_eig = eig.eig;
        const double rec[8] = {(double)fac.outer_done, fac.last_resid, (double)Z, (double)eig.block, eig.eig[0], eig.theta_next, (double)eig.mf_passes, 0.0};
        std::copy(rec, rec + 8, spec_info);
        return MMW_OK;
    }
    // ---- the random embedding (sdp_solver.py:109-114; kernels_factor_random.h): K x cols row-normalised Philox normals of (seed, 0) into
    // the buffer the factors live in, on the handle's stream behind whatever is in flight there.  Nothing of the iterate is read or
    // written, so the caller does not settle a pending chunk for it.  A block that needs a larger buffer gets it BEFORE the old one is
    // let go: a refused call leaves the last factor where it was.
    int factor_random(int32_t cols, int index_order, double* out, uint64_t seed) {
        const size_t n = (size_t)K * (size_t)cols;
        if (fac.out64.cap < n || !fac.out64.p) {
            size_t free_b = 0, total_b = 0;
            MMW_HIP(hipMemGetInfo(&free_b, &total_b));
            if (n > free_b / sizeof(double))
                return fail(MMW_ERR_HIP, "mmw_factor_random: the block of K x cols = " + std::to_string(K) + " x " + std::to_string(cols) + " doubles (" +
                                             std::to_string(n) + " x 8 bytes) does not fit: " + std::to_string(free_b) + " bytes are free on the device");
            DevBuf<double> grown;
            if (grown.alloc(n) != MMW_OK) {
                (void)hipGetLastError();
                return fail(MMW_ERR_HIP, "mmw_factor_random: the block of K x cols = " + std::to_string(K) + " x " + std::to_string(cols) + " doubles (" +
                                             std::to_string(n) + " x 8 bytes) could not be allocated");
            }
            fac.out64.swap(grown);  // (the old buffer goes with `grown`: hipFree waits for the launches that still read it)
        }
        fac.out64.n = std::max(fac.out64.n, n);
        fac.last_n = 0;
        fac.last_on_host = false;
        hipLaunchKernelGGL(k_factor_random, dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, (int)cols, seed, index_order, fac.out64.p);
        MMW_HIP(hipGetLastError());
        if (out) MMW_TRY(fac.fetch_last(n));  // (out == nullptr: the block stays on the device until somebody reads it)
        fac.last_n = n;
        fac.last_rank = cols;
        spec_live = false;  // (MMW_F_FACTOR_ROWNORM belongs to a spectral factor)
        if (out) memcpy(out, fac.last_host.p, n * sizeof(double));
        return MMW_OK;
    }
    int read_rownorm(double* out, int64_t n) {
        if (!spec_live) return fail(MMW_ERR_STATE, "mmw_read_f64(FACTOR_ROWNORM): the handle's last factor is not a spectral one");
        if (n != (int64_t)K) return fail(MMW_ERR_ARG, "mmw_read_f64(FACTOR_ROWNORM): wrong length");
        return copy_d2h(out, spec_rownorm.p, (size_t)K * sizeof(double), st);
    }
    int read_factor(double* out, int64_t n) {
        if ((int64_t)fac.last_n != n || n == 0) return fail(MMW_ERR_STATE, "mmw_read_f64(FACTOR): no factor of that size has been computed");
        MMW_TRY(fac.fetch_last(fac.last_n));
        memcpy(out, fac.last_host.p, fac.last_n * sizeof(double));
        return MMW_OK;
    }

    // handle creation: the buffers the factor and one batched rounding call of (Z, D', nbatch) would size on first use
    int fac_reserve(hipStream_t s, int K_, int rank, bool mf_possible) {
        fac.st = s; fac.K = K_; fac.dw.st = s;
        return fac.reserve(rank, mf_possible);
    }
    PinnedBuf stage;  // host side of mmw_round's transfers
    int round_reserve(int K_, int32_t Z, int32_t Dp, int32_t nb) {
        MMW_TRY(stage.ensure((size_t)K_ * Dp * sizeof(double) + (size_t)nb * Z * Dp * sizeof(double) + (size_t)nb * K_ * sizeof(int) + 8 + (size_t)nb * sizeof(int)));
        const size_t nP = (size_t)nb * K_ * Z;
        MMW_TRY(ensure(gX, (size_t)K_ * Dp)); MMW_TRY(ensure(randv, (size_t)nb * Z * Dp));
        MMW_TRY(ensure(P, nP)); MMW_TRY(ensure(pref, nP)); MMW_TRY(ensure(gain, nP));
        MMW_TRY(ensure(slot, (size_t)nb * K_)); MMW_TRY(ensure(nrm, K_)); MMW_TRY(ensure(order, K_)); MMW_TRY(ensure(rem, nb));
        MMW_TRY(ensure(rank_part, (size_t)RANK_SPLIT * K_));
        return MMW_OK;
    }

    // the lists one rounding reads: the handle's own state, or the set built from an environment (round_env)
    struct RoundView {
        const int* so_indptr; const int* so_indices; const int* q_indptr; const int* q_indices;
        const double* so_data; const double* so_hmax; const double* h_max;
    };
    // every refusal of mmw_round / mmw_round_env (`who`) that needs no device: before anything is allocated, copied, launched or timed
    int round_check(const std::string& who, int32_t Z, int32_t Dp, const double* gX_h, int32_t nb, const double* randv_h, int32_t* z_out, int32_t* rem_out) const {
        if (Z < 1 || Dp < 1 || nb < 1) return fail(MMW_ERR_ARG, who + ": Z, D' and nbatch must be positive");
        if (!randv_h || !z_out || !rem_out) return fail(MMW_ERR_ARG, who + ": null pointer");
        // gX == nullptr: the factor this handle computed last, where mmw_factor left it on the device (no copy out and in again)
        if (!gX_h && ((size_t)K * Dp != fac.last_n || Dp != fac.last_rank || fac.last_n == 0))
            return fail(MMW_ERR_STATE, who + ": gX is null and the handle holds no factor of K x D'");
        // every Z this call cannot run is refused here: k_greedy_b keeps GB_WAVES rows of Z flags in LDS (Z <= 4800, which also keeps
        // k_slot_pref's 8 Z bytes within the default 64 KiB)
        if ((size_t)GB_WAVES * Z * 4 > 150 * 1024) return fail(MMW_ERR_ARG, who + ": 32 Z bytes exceed the greedy kernel's LDS");
        return MMW_OK;
    }
    int round(int32_t Z, int32_t Dp, const double* gX_h, int32_t nb, const double* randv_h, int32_t* z_out, int32_t* rem_out) {
        MMW_TRY(round_check("mmw_round", Z, Dp, gX_h, nb, randv_h, z_out, rem_out));
        const RoundView own{so_indptr.p, so_indices.p, q_indptr.p, q_indices.p, so_data.p, so_hmax.p, h_max.p};
        return round_on(own, Z, Dp, gX_h, nb, randv_h, z_out, rem_out);
    }
    // ---- mmw_round_env: the same rounding against the state an environment holds now.  The second list set belongs to the handle and is
    // kept for the (environment, generation) it was built from: the attempts of one time point, and every point of a sweep in which nobody
    // moved, build it once.  The handle's own lists, its iterate and its factor are not touched.
    RoundListSet env_lists;
    uint64_t env_uid = 0, env_gen = 0;  // uid 0: nothing cached
    int32_t env_builds = 0;             // how often the set was built (MMW_I_ROUND_LIST_BUILDS)
    // the one statement of the cache rule: the view of `E`'s state, built when (uid, gen) is not the cached one
    int env_view(const EnvListSource& E, RoundView& view) {
        if (env_uid != E.uid || env_gen != E.gen) {
            env_uid = 0;
            MMW_TRY(env_lists.build(st, E));
            env_uid = E.uid; env_gen = E.gen;
            ++env_builds;
        }
        const RoundListSet& L = env_lists;
        view = RoundView{L.so_indptr.p, L.so_indices.p, L.q_indptr.p, L.q_indices.p, L.so_data.p, L.so_hmax.p, L.h_max.p};
        return MMW_OK;
    }
    int round_env(const EnvListSource& E, int32_t Z, int32_t Dp, const double* gX_h, int32_t nb, const double* randv_h, int32_t* z_out, int32_t* rem_out) {
        MMW_TRY(round_check("mmw_round_env", Z, Dp, gX_h, nb, randv_h, z_out, rem_out));
        RoundView view;
        MMW_TRY(env_view(E, view));
        return round_on(view, Z, Dp, gX_h, nb, randv_h, z_out, rem_out);
    }
    // the device buffers one call of nb attempts reads and writes
    int round_buffers(int32_t Z, int32_t Dp, bool own_gX, int32_t nb) {
        const size_t nP = (size_t)nb * K * Z;
        if (own_gX) MMW_TRY(ensure(gX, (size_t)K * Dp));
        MMW_TRY(ensure(randv, (size_t)nb * Z * Dp));
        MMW_TRY(ensure(P, nP));
        MMW_TRY(ensure(pref, nP));
        MMW_TRY(ensure(gain, nP));
        MMW_TRY(ensure(slot, (size_t)nb * K));
        MMW_TRY(ensure(nrm, K));
        MMW_TRY(ensure(order, K));
        MMW_TRY(ensure(rank_part, (size_t)RANK_SPLIT * K));
        MMW_TRY(ensure(rem, nb));
        return MMW_OK;
    }
    int round_on(const RoundView& V, int32_t Z, int32_t Dp, const double* gX_h, int32_t nb, const double* randv_h, int32_t* z_out, int32_t* rem_out) {
        MMW_TRY(round_buffers(Z, Dp, gX_h != nullptr, nb));
        const double* gX_d = gX_h ? gX.p : fac.out64.p;
        // inputs and outputs cross through the handle's page-locked staging buffer (runtime.h, PinnedBuf)
        const size_t b_gx = gX_h ? (size_t)K * Dp * sizeof(double) : 0, b_rv = (size_t)nb * Z * Dp * sizeof(double);
        const size_t b_z = (((size_t)nb * K * sizeof(int)) + 7) & ~(size_t)7, b_rem = (size_t)nb * sizeof(int);
        MMW_TRY(stage.ensure(b_gx + b_rv + b_z + b_rem));
        char* sp = static_cast<char*>(stage.p);
        if (gX_h) memcpy(sp, gX_h, b_gx);
        memcpy(sp + b_gx, randv_h, b_rv);
        if (gX_h) MMW_HIP(hipMemcpyAsync(gX.p, sp, b_gx, hipMemcpyHostToDevice, st));
        MMW_HIP(hipMemcpyAsync(randv.p, sp + b_gx, b_rv, hipMemcpyHostToDevice, st));
        MMW_TRY(round_chain(V, Z, Dp, gX_d, nb));
        MMW_HIP(hipMemcpyAsync(sp + b_gx + b_rv, slot.p, (size_t)nb * K * sizeof(int), hipMemcpyDeviceToHost, st));
        MMW_HIP(hipMemcpyAsync(sp + b_gx + b_rv + b_z, rem.p, b_rem, hipMemcpyDeviceToHost, st));
        MMW_HIP(hipStreamSynchronize(st));
        memcpy(z_out, sp + b_gx + b_rv, (size_t)nb * K * sizeof(int));
        memcpy(rem_out, sp + b_gx + b_rv + b_z, b_rem);
        return MMW_OK;
    }
    // from "gX_d and randv[nb][Z][D'] are on the device" to "slot[nb][K] and rem[nb] are on the device": the chain mmw_round and
    // mmw_round_attempts share (round_buffers has sized what it touches)
    int round_chain(const RoundView& V, int32_t Z, int32_t Dp, const double* gX_d, int32_t nb) {
        const size_t baseb = (size_t)GB_WAVES * Z * 4;
        const size_t nP = (size_t)nb * K * Z;
        MMW_HIP(hipMemsetAsync(gain.p, 0, nP * sizeof(double), st));
        MMW_HIP(hipMemsetAsync(slot.p, 0xFF, (size_t)nb * K * sizeof(int), st));
        if (kt) MMW_TRY(kt->begin(KT_PROJECT));
        hipLaunchKernelGGL(k_row_norms_f64, dim3(grid_rows(K)), dim3(BLOCK), 0, st, K, Dp, gX_d, nrm.p);
        hipLaunchKernelGGL(k_rank_count, dim3((K + BLOCK - 1) / BLOCK, RANK_SPLIT), dim3(BLOCK), 0, st, K, nrm.p, rank_part.p);
        hipLaunchKernelGGL(k_rank_scatter, dim3((K + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, K, (const int*)rank_part.p, order.p);
        hipLaunchKernelGGL(k_project_mfma, dim3((K + 63) / 64, (Z + 15) / 16, nb), dim3(BLOCK), 0, st, K, Z, Dp, gX_d, randv.p, P.p);
        hipLaunchKernelGGL(k_slot_pref, dim3(K, nb), dim3(BLOCK), (size_t)Z * sizeof(double), st, K, Z, P.p, pref.p);
        if (kt) MMW_TRY(kt->end());
        MMW_HIP(hipGetLastError());
        if (kt) MMW_TRY(kt->begin(KT_GREEDY));
        hipLaunchKernelGGL(k_greedy_headers, dim3(grid_elems((size_t)K)), dim3(BLOCK), 0, st, K, order.p, V.so_indptr, V.q_indptr, V.h_max, ghdr.p);
        // steps scheduled out of order (kernels_round.h, k_greedy_schedule): interaction masks of the visiting order, the schedule,
        // the headers step by step; then one workgroup per attempt follows it
        MMW_TRY(ensure(gmask, (size_t)K));
        MMW_TRY(ensure(gsched, (size_t)K * GB_WAVES));
        MMW_TRY(ensure(gnsteps, 1));
        MMW_TRY(ensure(ghdr_s, (size_t)K * GB_WAVES));  // (at most K steps)
        MMW_HIP(hipMemsetAsync(gmask.p, 0, (size_t)K * sizeof(unsigned), st));
        const size_t pairs = (size_t)K * GS_W;
        hipLaunchKernelGGL(k_greedy_cmask, dim3((unsigned)((pairs + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, K, (const GreedyHdr*)ghdr.p,
                           V.so_indices, V.q_indices, gmask.p);
        hipLaunchKernelGGL(k_greedy_schedule, dim3(1), dim3(WAVE), 0, st, K, (const unsigned*)gmask.p, gsched.p, gnsteps.p);
        hipLaunchKernelGGL(k_greedy_sched_headers, dim3(grid_elems((size_t)K * 2)), dim3(BLOCK), 0, st, K, (const int*)gnsteps.p, (const int*)gsched.p,
                           (const GreedyHdr*)ghdr.p, ghdr_s.p);
        if (live_switch(LIVE_VERBOSE)) {
            int ns = 0;
            MMW_HIP(hipMemcpyAsync(&ns, gnsteps.p, sizeof(int), hipMemcpyDeviceToHost, st));
            MMW_HIP(hipStreamSynchronize(st));
            fprintf(stderr, "[round] %d users in %d steps (%.1f per step)\n", K, ns, (double)K / std::max(ns, 1));
        }
        const bool slot_lds = baseb + (size_t)K * 4 <= 150 * 1024;
        const size_t sh = baseb + (slot_lds ? (size_t)K * 4 : 0);
        if (slot_lds) {
            MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_greedy_b<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            hipLaunchKernelGGL((k_greedy_b<true, true>), dim3(nb), dim3(GB_WAVES * 64), sh, st, K, Z, (const GreedyHdr*)ghdr_s.p, (const int*)nullptr, pref.p,
                               V.so_indices, V.so_data, V.so_hmax, V.q_indices, gain.p, slot.p, rem.p, (const int*)gnsteps.p);
        } else {
            MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_greedy_b<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            hipLaunchKernelGGL((k_greedy_b<false, true>), dim3(nb), dim3(GB_WAVES * 64), sh, st, K, Z, (const GreedyHdr*)ghdr_s.p, (const int*)nullptr, pref.p,
                               V.so_indices, V.so_data, V.so_hmax, V.q_indices, gain.p, slot.p, rem.p, (const int*)gnsteps.p);
        }
        if (kt) MMW_TRY(kt->end());
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }

    // ---- mmw_round_attempts / mmw_round_env_attempts / mmw_round_randv: the attempts of one rounding() call (sdp_solver.py:18-25) drawn,
    // run and chosen among on the device (kernels_round_draw.h).  Attempt a's directions depend on (seed, a) alone, so the call returns
    // what the loop over single attempts with stop-at-first returns, however many attempts it ran side by side.
    DevBuf<int> win, pick_info;  // the winner's K slots; {pick, rem[pick]}
    // the refusals that read arguments only (`who`: the entry), before the handle is looked at
    static int attempts_check(const std::string& who, int32_t Z, int32_t Dp, int32_t nattempt, int pick_rule, const int32_t* z_out, const int32_t* rem_out,
                              const int32_t* pick_out) {
        if (Z < 1 || Dp < 1) return fail(MMW_ERR_ARG, who + ": Z and D' must be positive");
        if (nattempt < 1 || nattempt > ROUND_MAX_ATTEMPTS)
            return fail(MMW_ERR_ARG, who + ": nattempt = " + std::to_string(nattempt) + " must be in [1, " + std::to_string(ROUND_MAX_ATTEMPTS) + "]");
        if (pick_rule != 0 && pick_rule != 1) return fail(MMW_ERR_ARG, who + ": pick_rule must be 0 (the first feasible attempt, else the last) or 1 (the fewest users left over)");
        if (!z_out || !rem_out || !pick_out) return fail(MMW_ERR_ARG, who + ": null pointer");
        if ((size_t)GB_WAVES * Z * 4 > 150 * 1024) return fail(MMW_ERR_ARG, who + ": 32 Z bytes exceed the greedy kernel's LDS");
        return MMW_OK;
    }
    int attempts_factor_check(const std::string& who, int32_t Dp, const double* gX_h) const {
        if (!gX_h && ((size_t)K * Dp != fac.last_n || Dp != fac.last_rank || fac.last_n == 0))
            return fail(MMW_ERR_STATE, who + ": gX is null and the handle holds no factor of K x D'");
        return MMW_OK;
    }
    int round_attempts(int32_t Z, int32_t Dp, const double* gX_h, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out, int32_t* rem_out,
                       int32_t* pick_out, int32_t* z_all) {
        MMW_TRY(attempts_factor_check("mmw_round_attempts", Dp, gX_h));
        const RoundView own{so_indptr.p, so_indices.p, q_indptr.p, q_indices.p, so_data.p, so_hmax.p, h_max.p};
        return round_attempts_on(own, Z, Dp, gX_h, nattempt, seed, pick_rule, z_out, rem_out, pick_out, z_all);
    }
    int round_env_attempts(const EnvListSource& E, int32_t Z, int32_t Dp, const double* gX_h, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out,
                           int32_t* rem_out, int32_t* pick_out, int32_t* z_all) {
        MMW_TRY(attempts_factor_check("mmw_round_env_attempts", Dp, gX_h));
        RoundView view;
        MMW_TRY(env_view(E, view));
        return round_attempts_on(view, Z, Dp, gX_h, nattempt, seed, pick_rule, z_out, rem_out, pick_out, z_all);
    }
    void launch_randv(int32_t Z, int32_t Dp, int32_t nattempt, uint64_t seed, uint32_t attempt0) {
        const size_t waves = (size_t)nattempt * Z;
        hipLaunchKernelGGL(k_round_randv, dim3((unsigned)((waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), dim3(BLOCK), 0, st, Z, Dp, nattempt, seed, attempt0,
                           randv.p);
    }
    int round_attempts_on(const RoundView& V, int32_t Z, int32_t Dp, const double* gX_h, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out,
                          int32_t* rem_out, int32_t* pick_out, int32_t* z_all) {
        MMW_TRY(round_buffers(Z, Dp, gX_h != nullptr, nattempt));
        MMW_TRY(ensure(win, (size_t)K));
        MMW_TRY(ensure(pick_info, 2));
        const double* gX_d = gX_h ? gX.p : fac.out64.p;
        // in: gX when the caller hands one.  out: the winner's K slots, {pick, rem[pick]}, the nattempt counts (and all slots when asked)
        const size_t b_gx = gX_h ? (size_t)K * Dp * sizeof(double) : 0;
        const size_t b_win = (size_t)K * sizeof(int), b_info = 2 * sizeof(int), b_rem = (size_t)nattempt * sizeof(int);
        const size_t b_all = z_all ? (size_t)nattempt * K * sizeof(int) : 0;
        MMW_TRY(stage.ensure(b_gx + b_win + b_info + b_rem + b_all));
        char* sp = static_cast<char*>(stage.p);
        if (gX_h) {
            memcpy(sp, gX_h, b_gx);
            MMW_HIP(hipMemcpyAsync(gX.p, sp, b_gx, hipMemcpyHostToDevice, st));
        }
        launch_randv(Z, Dp, nattempt, seed, 0u);
        MMW_TRY(round_chain(V, Z, Dp, gX_d, nattempt));
        hipLaunchKernelGGL(k_round_pick, dim3((unsigned)((K + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, K, nattempt, pick_rule, (const int*)rem.p, (const int*)slot.p,
                           win.p, pick_info.p);
        MMW_HIP(hipGetLastError());
        char* so = sp + b_gx;
        MMW_HIP(hipMemcpyAsync(so, win.p, b_win, hipMemcpyDeviceToHost, st));
        MMW_HIP(hipMemcpyAsync(so + b_win, pick_info.p, b_info, hipMemcpyDeviceToHost, st));
        MMW_HIP(hipMemcpyAsync(so + b_win + b_info, rem.p, b_rem, hipMemcpyDeviceToHost, st));
        if (z_all) MMW_HIP(hipMemcpyAsync(so + b_win + b_info + b_rem, slot.p, b_all, hipMemcpyDeviceToHost, st));
        MMW_HIP(hipStreamSynchronize(st));
        memcpy(z_out, so, b_win);
        int info[2];
        memcpy(info, so + b_win, b_info);
        *pick_out = info[0];
        memcpy(rem_out, so + b_win + b_info, b_rem);
        if (z_all) memcpy(z_all, so + b_win + b_info + b_rem, b_all);
        return MMW_OK;
    }
    // the seam for the tests: the directions of ONE attempt by the same kernel, copied out
    int round_randv(int32_t Z, int32_t Dp, uint64_t seed, int32_t attempt, double* out) {
        MMW_TRY(ensure(randv, (size_t)Z * Dp));
        launch_randv(Z, Dp, 1, seed, (uint32_t)attempt);
        MMW_HIP(hipGetLastError());
        return copy_d2h(out, randv.p, (size_t)Z * Dp * sizeof(double), st);
    }
};

}  // namespace mmw
