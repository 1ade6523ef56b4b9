// Batched solver (mmw_batch_*): many small fp64 instances, one workgroup each (csrc/kernels_batch.h).  Every instance's pattern is built by the
// host code mmw_create uses (build_pattern / update_slots), then all of them are packed into one int32 and one fp64 arena.
#pragma once
#include <limits>

#include "kernels_batch.h"
#include "solver.h"

struct mmw_batch {
    int device = 0;
    bool host_only = false;
    hipStream_t st = nullptr;
    int B = 0, rank_radio = 2, max_order = MAX_ORDER;
    double tol = 1e-9;
    std::vector<double> eta;  // per instance
    std::vector<HostPattern> H;
    std::vector<int> nit, iter;
    std::vector<char> active;
    std::vector<BatchDesc> desc;  // offsets and sizes; nrun / iter0 / seed / o_randv are set per call
    DevBuf<int> ia;
    DevBuf<double> fa, rbuf, skbuf;
    DevBuf<BatchDesc> d_desc;
    // the duality-gap log (mmw_batch_set_gap): a buffer of its own, made when the gap is first enabled, so the arenas do not move
    bool gap_ever = false, gap_on = false;
    int gap_mcap = GAP_DEFAULT_M;
    std::vector<GapDesc> gdesc;
    DevBuf<double> ga;
    DevBuf<GapDesc> d_gdesc;
    ~mmw_batch() {
        if (host_only || !st) return;
        (void)hipSetDevice(device);
        (void)hipStreamDestroy(st);
    }
    static int host_only_batch() { return fail(MMW_ERR_STATE, "this batch was created with device -1 (host patterns only)"); }
    static std::string check_limits(const HostPattern& P, int D) {
        if (P.K > BATCH_MAX_K) return "K = " + std::to_string(P.K) + " exceeds the batch limit " + std::to_string(BATCH_MAX_K);
        if (D > BATCH_MAX_D) return "D = " + std::to_string(D) + " exceeds the batch limit " + std::to_string(BATCH_MAX_D);
        if (P.nnzL() > BATCH_MAX_NNZ) return "nnzL = " + std::to_string(P.nnzL()) + " exceeds the batch limit " + std::to_string(BATCH_MAX_NNZ);
        const int64_t bytes = fp64_words(P, D) * 8 + int_words(P) * 4;
        if (bytes > BATCH_MAX_BYTES) return "instance needs " + std::to_string(bytes) + " bytes, over the batch limit " + std::to_string(BATCH_MAX_BYTES);
        return "";
    }
    static int64_t int_words(const HostPattern& P) { return (int64_t)P.K + 1 + 3 * P.nnzL() + P.K + P.E_asso(); }
    static int64_t fp64_words(const HostPattern& P, int D) {
        const int64_t K = P.K, nnz = P.nnzL(), C = P.C();
        return 5 * nnz + 6 * K + 4 * C + 4 * K * D + 4 + 64;
    }
    // offsets of every instance; the int32 arena never changes, the fp64 one follows the slot counts
    int layout() {
        desc.assign(B, BatchDesc{});
        int64_t oi = 0, of = 0;
        auto a32 = [](int64_t x) { return (x + 31) & ~(int64_t)31; };  // 256-byte aligned instance arrays
        for (int b = 0; b < B; ++b) {
            const HostPattern& P = H[b];
            BatchDesc& d = desc[b];
            const int64_t K = P.K, nnz = P.nnzL(), C = P.C();
            d.K = P.K; d.Z = P.Z; d.D = P.Z * rank_radio; d.E_asso = (int)P.E_asso(); d.C = (int)C; d.nnzL = (int)nnz;
            d.max_order = max_order; d.eta = eta[b]; d.tol = tol; d.o_randv = -1;
            const std::string err = check_limits(P, d.D);
            if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_batch: instance " + std::to_string(b) + ": " + err + " (run it on a handle)");
            d.o_indptr = oi; oi += K + 1;
            d.o_col = oi; oi += nnz;
            d.o_lrow = oi; oi += nnz;
            d.o_pid = oi; oi += nnz;
            d.o_diag = oi; oi += K;
            d.o_apos = oi; oi += P.E_asso();
            oi = a32(oi);
            const int64_t KD = K * d.D;
            d.o_sab = of; of += 2 * nnz;  // sab, then sba
            d.o_hmax = of; of += K;
            d.o_ssum = of; of += K;
            d.o_invn = of; of += K;
            d.o_cH = of; of += K;
            d.o_lval = of = a32(of); of += nnz;
            d.o_xval = of = a32(of); of += nnz;
            d.o_xavg = of = a32(of); of += nnz;
            d.o_Y = of = a32(of); of += C;
            d.o_yavg = of = a32(of); of += C;
            d.o_eaccu = of = a32(of); of += C;
            d.o_ethis = of = a32(of); of += C;
            d.o_wH = of = a32(of); of += K;
            d.o_rsum = of = a32(of); of += K;
            d.o_Xh = of = a32(of); of += KD;
            d.o_R = of = a32(of); of += KD;
            d.o_W1 = of = a32(of); of += KD;
            d.o_W2 = of = a32(of); of += KD;
            d.o_info = of = a32(of); of += 4;
            of = a32(of);
        }
        if (host_only) return MMW_OK;
        std::vector<int> hi((size_t)oi, 0);
        std::vector<double> hf((size_t)of, 0.0);
        for (int b = 0; b < B; ++b) {
            const HostPattern& P = H[b];
            const BatchDesc& d = desc[b];
            const int K = P.K;
            const int64_t nnz = P.nnzL();
            std::copy(P.l_indptr.begin(), P.l_indptr.end(), hi.begin() + d.o_indptr);
            std::copy(P.l_indices.begin(), P.l_indices.end(), hi.begin() + d.o_col);
            for (int k = 0; k < K; ++k)
                for (int e = P.l_indptr[k]; e < P.l_indptr[k + 1]; ++e) hi[d.o_lrow + e] = k;
            std::copy(P.pid.begin(), P.pid.end(), hi.begin() + d.o_pid);
            std::copy(P.diag_pos.begin(), P.diag_pos.end(), hi.begin() + d.o_diag);
            std::copy(P.asso_pos.begin(), P.asso_pos.end(), hi.begin() + d.o_apos);
            std::copy(P.sab.begin(), P.sab.end(), hf.begin() + d.o_sab);
            std::copy(P.sba.begin(), P.sba.end(), hf.begin() + d.o_sab + nnz);
            std::copy(P.h_max.begin(), P.h_max.end(), hf.begin() + d.o_hmax);
            std::copy(P.S_sum.begin(), P.S_sum.end(), hf.begin() + d.o_ssum);
            for (int k = 0; k < K; ++k) hf[d.o_invn + k] = 1.0 / P.norm_H[k];
            std::copy(P.cH.begin(), P.cH.end(), hf.begin() + d.o_cH);
        }
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(ia.upload(hi, st));
        MMW_TRY(fa.upload(hf, st));
        MMW_TRY(d_desc.alloc((size_t)B));
        return MMW_OK;
    }
    // offsets of every instance's gap work space (nnzL + 5 K doubles, all instances first) and log (4 doubles per announced
    // iteration, all logs after the work spaces); every log row NaN
    int gap_layout() {
        gdesc.assign(B, GapDesc{});
        int64_t og = 0;
        auto a32 = [](int64_t x) { return (x + 31) & ~(int64_t)31; };
        for (int b = 0; b < B; ++b) { gdesc[b].o_work = og; og = a32(og + (int64_t)desc[b].nnzL + 5 * (int64_t)desc[b].K); }
        const int64_t log0 = og;
        for (int b = 0; b < B; ++b) { gdesc[b].o_log = og; og = a32(og + 4 * (int64_t)nit[b]); }
        const std::vector<double> init((size_t)(og - log0), std::numeric_limits<double>::quiet_NaN());
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(ga.alloc((size_t)og));
        MMW_TRY(copy_h2d(ga.p + log0, init.data(), init.size() * sizeof(double), st));
        MMW_TRY(d_gdesc.alloc((size_t)B));
        return MMW_OK;
    }
    int set_gap(int enabled, int32_t m_cap) {
        if (host_only) return host_only_batch();
        if (m_cap > GAP_MAX_M) return fail(MMW_ERR_ARG, "mmw_batch_set_gap: m_cap must be at most " + std::to_string(GAP_MAX_M));
        if (enabled && !gap_ever) {
            MMW_TRY(gap_layout());
            gap_ever = true;
        }
        gap_on = enabled != 0;
        gap_mcap = m_cap <= 0 ? GAP_DEFAULT_M : m_cap;
        return MMW_OK;
    }
    int read_gap(int b, double* out, int64_t n) {
        MMW_TRY(check_inst(b));
        if (host_only) return host_only_batch();
        if (!gap_ever) return fail(MMW_ERR_STATE, "mmw_batch_read_gap: the gap was never enabled on this batch (mmw_batch_set_gap)");
        if (n != 4 * (int64_t)iter[b]) return fail(MMW_ERR_ARG, "mmw_batch_read_gap: wrong length " + std::to_string(n) + ", expected 4 x " + std::to_string(iter[b]) + " iterations done");
        if (n == 0) return MMW_OK;
        MMW_HIP(hipSetDevice(device));
        return copy_d2h(out, ga.p + gdesc[b].o_log, (size_t)n * sizeof(double), st);
    }
    // the reference's initial point (mmw.py:62-73): Y = 1/C, X = I, L = 0, sums zero
    int reset(int32_t nit_) {
        if (host_only) return host_only_batch();
        if (nit_ < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        MMW_HIP(hipSetDevice(device));
        for (int b = 0; b < B; ++b) {
            nit[b] = nit_;
            MMW_TRY(reset_one(b));
        }
        if (gap_ever) MMW_TRY(gap_layout());  // an empty log for the new run
        return MMW_OK;
    }
    int reset_one(int b) {
        iter[b] = 0;
        const BatchDesc& d = desc[b];
        std::vector<double> init((size_t)(d.o_info - d.o_lval), 0.0);  // the iterate (lval ... W2) in one copy
        for (int k = 0; k < d.K; ++k) init[d.o_xval - d.o_lval + H[b].diag_pos[k]] = 1.0;
        // the running sums start empty: iteration i adds X_i and Y_i when it starts, so after n iterations they hold X_0 + ... + X_{n-1}
        for (int c = 0; c < d.C; ++c) init[d.o_Y - d.o_lval + c] = 1.0 / (double)d.C;
        return copy_h2d(fa.p + d.o_lval, init.data(), init.size() * sizeof(double), st);
    }
    int iterate(int32_t n, const double* randv, const uint64_t* seeds) {
        if (host_only) return host_only_batch();
        if (n < 1) return fail(MMW_ERR_ARG, "mmw_batch_iterate: n must be >= 1");
        if (!randv && !seeds) return fail(MMW_ERR_ARG, "mmw_batch_iterate: give either the sketches or one seed per instance");
        MMW_HIP(hipSetDevice(device));
        std::vector<BatchDesc> dd = desc;
        int64_t off = 0;
        int runs = 0;
        for (int b = 0; b < B; ++b) {
            BatchDesc& d = dd[b];
            d.nrun = active[b] ? std::min(n, nit[b] - iter[b]) : 0;
            d.iter0 = iter[b];
            d.eta = eta[b]; d.tol = tol; d.max_order = max_order;
            d.seed = seeds ? seeds[b] : 0;
            if (randv && d.nrun > 0) { d.o_randv = off; off += (int64_t)d.nrun * d.K * d.D; }
            runs += d.nrun > 0;
        }
        if (!runs) return fail(MMW_ERR_STATE, "mmw_batch_iterate: every instance has run its announced iterations");
        if (randv) MMW_TRY(rbuf.alloc((size_t)off));
        if (randv) MMW_TRY(copy_h2d(rbuf.p, randv, (size_t)off * sizeof(double), st));
        MMW_TRY(copy_h2d(d_desc.p, dd.data(), dd.size() * sizeof(BatchDesc), st));
        const double* rv = randv ? rbuf.p : (const double*)nullptr;
        if (gap_on) {
            for (int b = 0; b < B; ++b) gdesc[b].m_cap = gap_mcap;
            MMW_TRY(copy_h2d(d_gdesc.p, gdesc.data(), gdesc.size() * sizeof(GapDesc), st));
            hipLaunchKernelGGL(k_mmw_batch<true>, dim3(B), dim3(BATCH_THREADS), 0, st, d_desc.p, ia.p, fa.p, rv, d_gdesc.p, ga.p);
        } else {
            hipLaunchKernelGGL(k_mmw_batch<false>, dim3(B), dim3(BATCH_THREADS), 0, st, d_desc.p, ia.p, fa.p, rv, (const GapDesc*)nullptr, (double*)nullptr);
        }
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < B; ++b) iter[b] += dd[b].nrun;
        return MMW_OK;
    }
    int set_slots(const int32_t* Z, int32_t nit_) {
        if (host_only) return host_only_batch();
        if (nit_ < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        std::vector<HostPattern> keep = H;  // a refused slot count leaves the batch as it was
        for (int b = 0; b < B; ++b) {
            if (Z[b] <= 0) continue;
            const std::string err = update_slots(H[b], Z[b]);
            if (!err.empty()) { H = std::move(keep); return fail(MMW_ERR_ARG, "mmw_batch_set_slots: instance " + std::to_string(b) + ": " + err); }
            const std::string lerr = check_limits(H[b], Z[b] * rank_radio);
            if (!lerr.empty()) { H = std::move(keep); return fail(MMW_ERR_ARG, "mmw_batch_set_slots: instance " + std::to_string(b) + ": " + lerr + " (run it on a handle)"); }
        }
        MMW_TRY(layout());
        for (int b = 0; b < B; ++b) {
            active[b] = Z[b] > 0;
            nit[b] = nit_;
            MMW_TRY(reset_one(b));
        }
        if (gap_ever) MMW_TRY(gap_layout());
        return MMW_OK;
    }
    int check_inst(int b) const {
        if (b < 0 || b >= B) return fail(MMW_ERR_ARG, "mmw_batch: instance index out of range");
        return MMW_OK;
    }
    int read_dev(int64_t o, int64_t len, double* out, int64_t n) {
        if (n != len) return fail(MMW_ERR_ARG, "mmw_batch_read_f64: wrong length " + std::to_string(n) + ", expected " + std::to_string(len));
        MMW_HIP(hipSetDevice(device));
        return copy_d2h(out, fa.p + o, (size_t)len * sizeof(double), st);
    }
    static int read_host(const std::vector<double>& v, double* out, int64_t n) { return export_vec(v, out, n, "mmw_batch_read_f64"); }
    int read_f64(int b, int which, double* out, int64_t n) {
        MMW_TRY(check_inst(b));
        const HostPattern& P = H[b];
        switch (which) {
            case MMW_F_S_SUM: return read_host(P.S_sum, out, n);
            case MMW_F_NORM_H: return read_host(P.norm_H, out, n);
            case MMW_F_ST_DATA: return read_host(P.st_data, out, n);
            default: break;
        }
        if (host_only) return host_only_batch();
        const BatchDesc& d = desc[b];
        const int64_t KD = (int64_t)d.K * d.D;
        switch (which) {
            case MMW_F_Y: return read_dev(d.o_Y, d.C, out, n);
            case MMW_F_E_ACCU: return read_dev(d.o_eaccu, d.C, out, n);
            case MMW_F_E_THIS: return read_dev(d.o_ethis, d.C, out, n);
            case MMW_F_LVAL: return read_dev(d.o_lval, d.nnzL, out, n);
            case MMW_F_XVAL: return read_dev(d.o_xval, d.nnzL, out, n);
            case MMW_F_XAVG: return read_dev(d.o_xavg, d.nnzL, out, n);
            case MMW_F_YAVG: return read_dev(d.o_yavg, d.C, out, n);
            case MMW_F_XHALF: return read_dev(d.o_Xh, KD, out, n);
            case MMW_F_SKETCH:
                if (iter[b] == 0) return fail(MMW_ERR_STATE, "mmw_batch_read_f64: no iteration has run on this instance");
                return read_dev(d.o_R, KD, out, n);
            case MMW_F_EXPM_INFO: return read_dev(d.o_info, 4, out, n);
            default: return fail(MMW_ERR_ARG, "mmw_batch_read_f64: field not held by a batch");
        }
    }
    int read_i32(int b, int which, int32_t* out, int64_t n) {
        MMW_TRY(check_inst(b));
        const std::vector<int32_t>* v = host_list_i32(H[b], which);
        return v ? export_vec(*v, out, n, "mmw_batch_read_i32") : fail(MMW_ERR_ARG, "mmw_batch_read_i32: unknown field");
    }
    int sketch(int b, uint64_t seed, int32_t iteration, double* out, int64_t n) {
        MMW_TRY(check_inst(b));
        if (host_only) return host_only_batch();
        if (iteration < 0) return fail(MMW_ERR_ARG, "mmw_batch_sketch: iteration must be >= 0");
        const BatchDesc& d = desc[b];
        const int64_t KD = (int64_t)d.K * d.D;
        if (n != KD) return fail(MMW_ERR_ARG, "mmw_batch_sketch: wrong length for a K x D block");
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(skbuf.alloc((size_t)KD));
        hipLaunchKernelGGL(k_batch_sketch, dim3(1), dim3(BATCH_THREADS), 0, st, d.K, d.D, seed, (uint32_t)iteration, skbuf.p);
        MMW_HIP(hipGetLastError());
        return copy_d2h(out, skbuf.p, (size_t)KD * sizeof(double), st);
    }
};
// mmw_batch_export: the instance's iterate into an fp64 handle of the same (state, Z), as if the handle had run those iterations.
inline int batch_export_into(mmw_batch* bt, int b, Solver<double>* s) {
    const BatchDesc& d = bt->desc[b];
    const HostPattern& P = bt->H[b];
    if (s->host_only || bt->host_only) return fail(MMW_ERR_STATE, "mmw_batch_export: host-only batch or handle");
    if (s->device != bt->device) return fail(MMW_ERR_ARG, "mmw_batch_export: the handle lives on another device");
    if (s->K != d.K || s->Z != d.Z || s->D != d.D || s->H.nnzL() != (int64_t)d.nnzL || s->H.C() != (int64_t)d.C)
        return fail(MMW_ERR_ARG, "mmw_batch_export: the handle's K / Z / nnzL do not match the instance's");
    if (s->H.l_indices != P.l_indices || s->H.l_indptr != P.l_indptr) return fail(MMW_ERR_ARG, "mmw_batch_export: the handle's pattern is not the instance's");
    MMW_HIP(hipSetDevice(s->device));
    MMW_TRY(s->settle());
    MMW_HIP(hipStreamSynchronize(bt->st));
    MMW_HIP(hipStreamSynchronize(s->st));
    // the state a reset leaves (plans, lagged history, chains, timers), then the iterate on top
    MMW_TRY(s->reset(std::max(1, bt->nit[b])));
    const size_t nnz = (size_t)d.nnzL, C = (size_t)d.C;
    const double* f = bt->fa.p;
    const struct { double* dst; int64_t off; size_t n; } parts[7] = {{s->lval.p, d.o_lval, nnz}, {s->xval.p, d.o_xval, nnz}, {s->xavg.p, d.o_xavg, nnz}, {s->Y.p, d.o_Y, C},
                                                                     {s->yavg.p, d.o_yavg, C}, {s->e_accu.p, d.o_eaccu, C}, {s->e_this.p, d.o_ethis, C}};
    for (const auto& p : parts) MMW_HIP(hipMemcpyAsync(p.dst, f + p.off, p.n * sizeof(double), hipMemcpyDeviceToDevice, s->st));
    // The batch adds X_i / Y_i to the running sums when iteration i starts; a handle adds them as soon as they are made while
    // iterations remain (mmw_gap reads iter + 1 terms then).  Before the last iteration the handle's sums hold the current X / Y too.
    if (bt->iter[b] < bt->nit[b]) {
        const unsigned gx = (unsigned)std::min<size_t>((nnz + BLOCK - 1) / BLOCK, 4096), gy = (unsigned)std::min<size_t>((C + BLOCK - 1) / BLOCK, 4096);
        hipLaunchKernelGGL((k_accumulate<double>), dim3(gx), dim3(BLOCK), 0, s->st, nnz, s->xval.p, s->xavg.p);
        hipLaunchKernelGGL((k_accumulate<double>), dim3(gy), dim3(BLOCK), 0, s->st, C, s->Y.p, s->yavg.p);
        MMW_HIP(hipGetLastError());
    }
    // derived copies: L in the LDS-staged SpMM's traversal order (when the handle's blocking is attached; a later attach gathers it
    // from lval itself)
    if (s->bt.lval_blk.p && s->bt.HB.nent > 0) {
        hipLaunchKernelGGL((k_gather_blocked<double>), dim3(grid_elems((size_t)s->bt.HB.nent)), dim3(BLOCK), 0, s->st, (size_t)s->bt.HB.nent,
                           s->bt.b_bepos.p, s->lval.p, s->bt.lval_blk.p);
        MMW_HIP(hipGetLastError());
    }
    s->lblk_stale = false;
    s->iter = bt->iter[b];
    MMW_HIP(hipStreamSynchronize(s->st));
    return MMW_OK;
}
