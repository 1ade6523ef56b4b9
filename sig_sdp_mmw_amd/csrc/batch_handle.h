// Batched solver (mmw_batch_*): many small fp64 instances, one workgroup each (csrc/kernels_batch.h).  Every instance's pattern is built by the
// host code mmw_create uses (build_pattern / update_slots), then all of them are packed into one int32 and one fp64 arena.
#pragma once
#include <limits>

#include "kernels_batch.h"
#include "kernels_batch_epilogue.h"
#include "kernels_batch_factor_split.h"
#include "kernels_batch_gm.h"
#include "kernels_batch_split.h"
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
    // the split (mmw_batch_set_split, kernels_batch_split.h): workgroups per instance (empty: one each, the single-launch kernel); the
    // work tables and the slab of per-slice Taylor degrees are buffers of its own, rebuilt from `parts` and the current D per call
    std::vector<int> parts;
    DevBuf<SplitSlice> d_wexpm;
    DevBuf<SplitRange> d_wx;
    DevBuf<double> slab;
    // the epilogue (mmw_batch_factor / mmw_batch_round, kernels_batch_epilogue.h): buffers of its own, made on first use and sized for
    // the taking instances of the call; the state's rounding lists go up once (they do not depend on the slot count)
    std::vector<FactorDesc> fdesc;  // per instance: where its factor of the last mmw_batch_factor lies (rank 0: none)
    DevBuf<double> ew, rw, rs_f, rvbuf;
    DevBuf<int> ei, ri, rs_i;
    DevBuf<FactorDesc> d_fdesc;
    DevBuf<RoundDesc> d_rdesc;
    DevBuf<FactorRandomDesc> d_frdesc;
    // the factor's split (mmw_batch_set_factor_split, kernels_batch_factor_split.h): workgroups per instance and round (empty: one
    // launch, k_batch_factor); the item table, the spans, the slab and the sweep records are buffers of its own, rebuilt per call
    std::vector<int> fparts;
    DevBuf<FactorItem> d_fitems;
    DevBuf<FactorSpan> d_fspans;
    DevBuf<double> fslab, frec;
    double fcall[4] = {0.0, 0.0, 0.0, 0.0};  // MMW_F_FACTOR_CALL: the last mmw_batch_factor {path, launches, host sweeps, largest grid}
    struct RoundLists { int64_t soptr, soidx, qptr, qidx, sodata, sohmax, hmax; };
    std::vector<RoundLists> rlists;
    // the greedy baselines (mmw_batch_gm, kernels_batch_gm.h): what the pattern does not keep of Q -- its values, and the clique
    // structure decided at creation (GmState::find_cliques) -- goes up once, beside the rounding lists; the call's buffers
    struct GmExtra {
        std::vector<double> q_data;
        std::vector<int32_t> grp;  // clique id per user, -1: no Q row
        int G = 0;
        bool clique = false;
    };
    std::vector<GmExtra> gmx;
    std::vector<int64_t> gm_ogrp, gm_oq;
    DevBuf<int> gm_i;
    DevBuf<double> gm_f;
    GmWork gmw;
    void gm_extra(int b, const int32_t* Qp, const double* Qx) {
        GmState g;
        g.K = H[b].K;
        g.q_indptr = H[b].q_indptr; g.q_indices = H[b].q_indices;
        g.q_data.assign(Qx, Qx + Qp[g.K]);
        GmExtra& x = gmx[b];
        x.clique = g.find_cliques();
        x.G = g.G;
        x.grp = std::move(g.grp);
        x.q_data = std::move(g.q_data);
    }
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
    int set_split(const int32_t* p) {
        if (host_only) return host_only_batch();
        bool any = false;
        for (int b = 0; p && b < B; ++b) {
            if (p[b] < 1 || p[b] > BATCH_MAX_PARTS)
                return fail(MMW_ERR_ARG, "mmw_batch_set_split: instance " + std::to_string(b) + ": parts = " + std::to_string(p[b]) + " is outside [1, " +
                                             std::to_string(BATCH_MAX_PARTS) + "]");
            any = any || p[b] > 1;
        }
        if (any) parts.assign(p, p + B);
        else parts.clear();
        return MMW_OK;
    }
    int set_factor_split(const int32_t* p) {
        if (host_only) return host_only_batch();
        bool any = false;
        for (int b = 0; p && b < B; ++b) {
            if (p[b] < 1 || p[b] > BATCH_MAX_PARTS)
                return fail(MMW_ERR_ARG, "mmw_batch_set_factor_split: instance " + std::to_string(b) + ": parts = " + std::to_string(p[b]) + " is outside [1, " +
                                             std::to_string(BATCH_MAX_PARTS) + "]");
            any = any || p[b] > 1;
        }
        if (any) fparts.assign(p, p + B);
        else fparts.clear();
        return MMW_OK;
    }
    // One iteration as three launches for all instances (kernels_batch_split.h); `dd` is on the device already.
    int iterate_split(const std::vector<BatchDesc>& dd, const double* rv) {
        std::vector<SplitSlice> we;
        std::vector<SplitRange> wx;
        int nmax = 0;
        for (int b = 0; b < B; ++b) {
            const BatchDesc& d = dd[b];
            if (d.nrun <= 0) continue;
            nmax = std::max(nmax, d.nrun);
            const int W = split_width(d.D, parts[b]), G = split_slices(d.D, parts[b]), slab0 = (int)we.size();
            for (int g = 0; g < G; ++g) we.push_back(SplitSlice{b, g, W, slab0 + g});
            for (int p = 0; p < parts[b]; ++p) wx.push_back(SplitRange{b, p, parts[b], slab0, G});
        }
        MMW_TRY(d_wexpm.upload(we, st));
        MMW_TRY(d_wx.upload(wx, st));
        MMW_TRY(slab.alloc(we.size()));
        for (int it = 0; it < nmax; ++it) {
            if (gap_on)
                hipLaunchKernelGGL(k_batch_split_head<true>, dim3(B), dim3(BATCH_THREADS), 0, st, d_desc.p, ia.p, fa.p, d_gdesc.p, ga.p, it);
            else
                hipLaunchKernelGGL(k_batch_split_head<false>, dim3(B), dim3(BATCH_THREADS), 0, st, d_desc.p, ia.p, fa.p, (const GapDesc*)nullptr, (double*)nullptr, it);
            hipLaunchKernelGGL(k_batch_split_expm, dim3((unsigned)we.size()), dim3(BATCH_THREADS), 0, st, d_desc.p, d_wexpm.p, ia.p, fa.p, rv, slab.p, it);
            hipLaunchKernelGGL(k_batch_split_x, dim3((unsigned)wx.size()), dim3(BATCH_THREADS), 0, st, d_desc.p, d_wx.p, ia.p, fa.p, slab.p, it);
        }
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
        fdesc.clear();
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
        bool split = false;
        for (int b = 0; b < B; ++b) {
            BatchDesc& d = dd[b];
            d.nrun = active[b] ? std::min(n, nit[b] - iter[b]) : 0;
            d.iter0 = iter[b];
            d.eta = eta[b]; d.tol = tol; d.max_order = max_order;
            d.seed = seeds ? seeds[b] : 0;
            if (randv && d.nrun > 0) { d.o_randv = off; off += (int64_t)d.nrun * d.K * d.D; }
            runs += d.nrun > 0;
            split = split || (d.nrun > 0 && !parts.empty() && parts[b] > 1);
        }
        if (!runs) return fail(MMW_ERR_STATE, "mmw_batch_iterate: every instance has run its announced iterations");
        if (randv) MMW_TRY(rbuf.alloc((size_t)off));
        if (randv) MMW_TRY(copy_h2d(rbuf.p, randv, (size_t)off * sizeof(double), st));
        MMW_TRY(copy_h2d(d_desc.p, dd.data(), dd.size() * sizeof(BatchDesc), st));
        const double* rv = randv ? rbuf.p : (const double*)nullptr;
        if (gap_on) {
            for (int b = 0; b < B; ++b) gdesc[b].m_cap = gap_mcap;
            MMW_TRY(copy_h2d(d_gdesc.p, gdesc.data(), gdesc.size() * sizeof(GapDesc), st));
        }
        if (split) {
            MMW_TRY(iterate_split(dd, rv));
        } else if (gap_on) {
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
        fdesc.clear();
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
            case MMW_F_FACTOR_CALL: return read_host(std::vector<double>(fcall, fcall + 4), out, n);
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
            case MMW_F_FACTOR:
            case MMW_F_FACTOR_INFO: {
                if (fdesc.empty() || fdesc[b].rank == 0) return fail(MMW_ERR_STATE, "mmw_batch_read_f64: instance " + std::to_string(b) + " has no factor (mmw_batch_factor)");
                const FactorDesc& f = fdesc[b];
                const int64_t len = which == MMW_F_FACTOR ? (int64_t)f.K * f.rank : EPI_INFO;
                if (n != len) return fail(MMW_ERR_ARG, "mmw_batch_read_f64: wrong length " + std::to_string(n) + ", expected " + std::to_string(len));
                MMW_HIP(hipSetDevice(device));
                return copy_d2h(out, ew.p + (which == MMW_F_FACTOR ? f.o_fac : f.o_info), (size_t)len * sizeof(double), st);
            }
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
    // ---- the epilogue on the device
    int takers(const char* who, const int32_t* take, std::vector<int>& tk) const {
        tk.clear();
        for (int b = 0; b < B; ++b) {
            if (take ? take[b] == 0 : !active[b]) continue;
            if (!active[b]) return fail(MMW_ERR_STATE, std::string(who) + ": instance " + std::to_string(b) + " sits out (mmw_batch_set_slots gave it no slot count)");
            tk.push_back(b);
        }
        if (tk.empty()) return fail(MMW_ERR_ARG, std::string(who) + ": no instance takes part");
        return MMW_OK;
    }
    int factor(const int32_t* take, const int32_t* rank, const double* const* xavg) {
        if (host_only) return host_only_batch();
        std::vector<int> tk;
        MMW_TRY(takers("mmw_batch_factor", take, tk));
        std::vector<int> rk(B, 0);
        for (int b : tk) {
            const BatchDesc& d = desc[b];
            const std::string who = "mmw_batch_factor: instance " + std::to_string(b);
            if (d.K > EPI_MAX_K) return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(d.K) + " exceeds the epilogue limit " + std::to_string(EPI_MAX_K) + " (factor it on a handle: mmw_batch_export)");
            if (!(xavg && xavg[b]) && iter[b] < nit[b])
                return fail(MMW_ERR_STATE, who + " has run " + std::to_string(iter[b]) + " of its " + std::to_string(nit[b]) + " iterations");
            rk[b] = rank ? rank[b] : std::min(d.K - 1, (d.Z - 1) * rank_radio);
            if (rk[b] < 1 || rk[b] > d.K) return fail(MMW_ERR_ARG, who + ": rank must be in [1, K]");
        }
        auto a32 = [](int64_t x) { return (x + 31) & ~(int64_t)31; };
        std::vector<FactorDesc> fd(B, FactorDesc{});
        std::vector<FactorDesc> launch;
        int64_t of = a32((int64_t)tk.size() * EPI_INFO_STRIDE), oi = 0;  // the records first, side by side: one copy brings them back
        int64_t ninfo = 0;
        for (int b : tk) {
            const BatchDesc& d = desc[b];
            FactorDesc& f = fd[b];
            const int64_t K = d.K;
            f.o_info = EPI_INFO_STRIDE * ninfo++;
            f.K = d.K; f.rank = rk[b]; f.nnzL = d.nnzL; f.cap = EPI_SWEEP_CAP;
            f.o_lrow = d.o_lrow; f.o_col = d.o_col;
            const bool parity = xavg && xavg[b];
            f.src_work = parity ? 1 : 0;
            f.div = parity ? 1.0 : (double)nit[b];
            f.o_src = d.o_xavg;
            if (parity) { f.o_src = of; of = a32(of + d.nnzL); }
            f.o_A = of; of = a32(of + K * K);
            f.o_fac = of; of = a32(of + K * f.rank);
            f.o_nrm = of; of = a32(of + K);
            f.o_ord = oi; oi = a32(oi + K);
            launch.push_back(f);
        }
        fdesc.clear();  // the buffers are laid out anew: earlier factors are gone whatever happens below
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(ew.alloc((size_t)of));
        MMW_TRY(ei.alloc((size_t)oi));
        for (int b : tk)
            if (fd[b].src_work) MMW_TRY(copy_h2d(ew.p + fd[b].o_src, xavg[b], (size_t)fd[b].nnzL * sizeof(double), st));
        MMW_TRY(d_fdesc.alloc(launch.size()));
        MMW_TRY(copy_h2d(d_fdesc.p, launch.data(), launch.size() * sizeof(FactorDesc), st));
        bool split = false;
        for (int b : tk) split = split || (!fparts.empty() && fparts[b] > 1);
        if (split) {
            MMW_TRY(factor_split(tk, launch));
        } else {
            hipLaunchKernelGGL(k_batch_factor, dim3((unsigned)launch.size()), dim3(BATCH_THREADS), 0, st, d_fdesc.p, ia.p, fa.p, ew.p, ei.p);
            fcall[0] = 0.0; fcall[1] = 1.0; fcall[2] = 0.0; fcall[3] = (double)launch.size();
        }
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        // A factor that used up its sweeps while rows still rotated is handed out (its rows are orthogonal to the |cos| it reports),
        // and said so: nothing above looks at the record on its own.
        std::vector<double> rec((size_t)tk.size() * EPI_INFO_STRIDE);
        MMW_TRY(copy_d2h(rec.data(), ew.p, rec.size() * sizeof(double), st));
        for (size_t t = 0; t < tk.size(); ++t) {
            const double* r = rec.data() + t * EPI_INFO_STRIDE;
            if (r[0] >= EPI_SWEEP_CAP && r[1] > EPI_ROT_TOL)
                fprintf(stderr, "mmw_batch_factor: instance %d (K = %d): still rotating after the cap of %d sweeps, largest |cos| of a row pair %.3g\n",
                        tk[t], desc[tk[t]].K, EPI_SWEEP_CAP, r[1]);
        }
        fdesc = std::move(fd);
        return MMW_OK;
    }
    // The factor as head / one launch per round / tail for all taking instances (kernels_batch_factor_split.h); `launch` is on the
    // device already (d_fdesc).  One synchronisation per sweep: the host reads the sweep records, ends the instances the device has
    // ended (no rotation, or the cap) and takes their items out of the table, so the grids shrink with the instances still rotating.
    int factor_split(const std::vector<int>& tk, const std::vector<FactorDesc>& launch) {
        const int n = (int)tk.size();
        std::vector<FactorSpan> spans((size_t)n);
        std::vector<FactorItem> items;
        int nslot = 0;
        for (int t = 0; t < n; ++t) {
            const int K = launch[t].K, parts = fparts[tk[t]];
            const int P = factor_pairs(K), per = factor_item_pairs(K, parts), G = factor_item_count(K, parts);
            spans[t] = FactorSpan{nslot, G};
            for (int g = 0; g < G; ++g) items.push_back(FactorItem{t, g * per, std::min(per, P - g * per), factor_rounds(K), nslot++});
        }
        std::stable_sort(items.begin(), items.end(), [](const FactorItem& a, const FactorItem& b) { return a.rounds > b.rounds; });
        MMW_TRY(d_fspans.upload(spans, st));
        MMW_TRY(d_fitems.upload(items, st));
        MMW_TRY(fslab.alloc((size_t)nslot * FSPLIT_SLOT));
        MMW_TRY(frec.alloc((size_t)n * FSPLIT_REC));
        hipLaunchKernelGGL(k_batch_factor_head, dim3((unsigned)n), dim3(BATCH_THREADS), 0, st, d_fdesc.p, d_fspans.p, ia.p, fa.p, ew.p, fslab.p, frec.p);
        int64_t launches = 1, sweeps = 0;
        size_t widest = std::max((size_t)n, items.size());
        std::vector<char> live((size_t)n, 1);
        std::vector<double> rec((size_t)n * FSPLIT_REC);
        int nlive = n;
        while (nlive > 0 && sweeps < EPI_SWEEP_CAP) {
            size_t cnt = items.size();  // items with more than r rounds: a prefix of the table
            for (int r = 0;; ++r) {
                while (cnt > 0 && items[cnt - 1].rounds <= r) --cnt;
                if (cnt == 0) break;
                hipLaunchKernelGGL(k_batch_factor_round, dim3((unsigned)cnt), dim3(BATCH_THREADS), 0, st, d_fdesc.p, d_fitems.p, ew.p, fslab.p, frec.p, r);
                ++launches;
            }
            hipLaunchKernelGGL(k_batch_factor_sweep, dim3((unsigned)n), dim3(WAVE), 0, st, d_fdesc.p, d_fspans.p, fslab.p, frec.p);
            ++launches;
            ++sweeps;
            MMW_HIP(hipGetLastError());
            MMW_TRY(copy_d2h(rec.data(), frec.p, rec.size() * sizeof(double), st));
            bool ended = false;
            for (int t = 0; t < n; ++t)
                if (live[t] && rec[(size_t)t * FSPLIT_REC + 3] != 0.0) { live[t] = 0; --nlive; ended = true; }
            if (ended && nlive > 0) {
                std::vector<FactorItem> keep;
                for (const FactorItem& w : items)
                    if (live[w.inst]) keep.push_back(w);
                items = std::move(keep);
                MMW_TRY(d_fitems.upload(items, st));
            }
        }
        hipLaunchKernelGGL(k_batch_factor_tail, dim3((unsigned)n), dim3(BATCH_THREADS), 0, st, d_fdesc.p, frec.p, ew.p, ei.p);
        ++launches;
        fcall[0] = 1.0; fcall[1] = (double)launches; fcall[2] = (double)sweeps; fcall[3] = (double)widest;
        return MMW_OK;
    }
    // the state's rounding lists (S_gain without its diagonal, Q_asso, h_max: csrc/pattern.h), all instances, once
    int round_lists() {
        if (!rlists.empty()) return MMW_OK;
        std::vector<RoundLists> rl(B);
        std::vector<int> hi;
        std::vector<double> hf;
        auto pad = [](auto& v) { v.resize((v.size() + 31) & ~(size_t)31); };
        for (int b = 0; b < B; ++b) {
            const HostPattern& P = H[b];
            RoundLists& r = rl[b];
            r.soptr = (int64_t)hi.size(); hi.insert(hi.end(), P.so_indptr.begin(), P.so_indptr.end());
            r.soidx = (int64_t)hi.size(); hi.insert(hi.end(), P.so_indices.begin(), P.so_indices.end());
            r.qptr = (int64_t)hi.size(); hi.insert(hi.end(), P.q_indptr.begin(), P.q_indptr.end());
            r.qidx = (int64_t)hi.size(); hi.insert(hi.end(), P.q_indices.begin(), P.q_indices.end());
            pad(hi);
            r.sodata = (int64_t)hf.size(); hf.insert(hf.end(), P.so_data.begin(), P.so_data.end());
            r.sohmax = (int64_t)hf.size();
            for (int32_t n : P.so_indices) hf.push_back(P.h_max[n]);
            r.hmax = (int64_t)hf.size(); hf.insert(hf.end(), P.h_max.begin(), P.h_max.end());
            pad(hf);
        }
        MMW_TRY(rs_i.upload(hi, st));
        MMW_TRY(rs_f.upload(hf, st));
        rlists = std::move(rl);
        return MMW_OK;
    }
    // The rounding lists of another state of the same users (mmw_batch_round_env, batch_env_handle.h): where they lie, and per
    // instance their offsets.  Null: the lists of the state the batch was built from.
    struct RoundSource {
        const char* who;
        const int* si;
        const double* sf;
        const RoundLists* lists;  // [B]
        const int* K;             // [B] users of every instance of the other state
    };
    int round(const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out, int32_t* rem_out, int32_t* used_out,
              const RoundSource* src = nullptr) {
        const std::string who = src ? src->who : "mmw_batch_round";
        if (host_only) return host_only_batch();
        if (nattempt < 1 || nattempt > 4096) return fail(MMW_ERR_ARG, who + ": nattempt must be in [1, 4096]");
        std::vector<int> tk;
        MMW_TRY(takers(who.c_str(), take, tk));
        for (int b : tk) {
            if (fdesc.empty() || fdesc[b].rank == 0 || fdesc[b].K != desc[b].K)
                return fail(MMW_ERR_STATE, who + ": instance " + std::to_string(b) + " has no factor (mmw_batch_factor)");
            if (src && src->K[b] != desc[b].K)
                return fail(MMW_ERR_ARG, who + ": instance " + std::to_string(b) + ": K = " + std::to_string(desc[b].K) + " in the batch, " +
                                             std::to_string(src->K[b]) + " in the environment");
        }
        MMW_HIP(hipSetDevice(device));
        if (!src) MMW_TRY(round_lists());
        auto a32 = [](int64_t x) { return (x + 31) & ~(int64_t)31; };
        std::vector<RoundDesc> rd;
        int64_t of = 0, oi = 0;
        for (int b : tk) oi += (int64_t)nattempt * fdesc[b].K + nattempt + 1;  // slots, remainders and attempts run of every instance: what goes back
        const int64_t nback = oi;
        oi = a32(oi);
        int64_t oz = 0;
        for (int b : tk) {
            const FactorDesc& f = fdesc[b];
            const RoundLists& l = src ? src->lists[b] : rlists[b];
            const int64_t K = f.K, Z = desc[b].Z;
            RoundDesc r{};
            r.K = f.K; r.Z = desc[b].Z; r.Dp = f.rank; r.nattempt = nattempt; r.stop_first = stop_at_first != 0;
            r.index_order = f.unit_rows;
            r.seed = seeds[b];
            r.o_fac = f.o_fac;
            r.s_soptr = l.soptr; r.s_soidx = l.soidx; r.s_qptr = l.qptr; r.s_qidx = l.qidx;
            r.s_sodata = l.sodata; r.s_sohmax = l.sohmax; r.s_hmax = l.hmax;
            r.r_randv = of; of = a32(of + Z * f.rank);
            r.r_inprod = of; of = a32(of + K * Z);
            r.r_gain = of; of = a32(of + K * Z);
            r.r_nrm = of; of = a32(of + K);
            r.r_order = oi; oi = a32(oi + K);
            r.r_pref = oi; oi = a32(oi + K * Z);
            r.r_z = oz; oz += (int64_t)nattempt * K;
            r.r_rem = oz; oz += nattempt + 1;
            rd.push_back(r);
        }
        MMW_TRY(rw.alloc((size_t)of));
        MMW_TRY(ri.alloc((size_t)oi));
        MMW_TRY(d_rdesc.alloc(rd.size()));
        MMW_TRY(copy_h2d(d_rdesc.p, rd.data(), rd.size() * sizeof(RoundDesc), st));
        hipLaunchKernelGGL(k_batch_round, dim3((unsigned)rd.size()), dim3(BATCH_THREADS), 0, st, d_rdesc.p, ew.p, src ? src->si : rs_i.p,
                           src ? src->sf : rs_f.p, rw.p, ri.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        std::vector<int> host((size_t)nback);
        MMW_TRY(copy_d2h(host.data(), ri.p, host.size() * sizeof(int), st));
        for (int b = 0; b < B; ++b) {
            used_out[b] = 0;
            for (int a = 0; a < nattempt; ++a) rem_out[(size_t)b * nattempt + a] = -1;
        }
        int32_t* z = z_out;
        for (size_t t = 0; t < tk.size(); ++t) {
            const RoundDesc& r = rd[t];
            const size_t nz = (size_t)nattempt * r.K;
            std::copy(host.begin() + r.r_z, host.begin() + r.r_z + nz, z);
            z += nz;
            std::copy(host.begin() + r.r_rem, host.begin() + r.r_rem + nattempt, rem_out + (size_t)tk[t] * nattempt);
            used_out[tk[t]] = host[r.r_rem + nattempt];
        }
        return MMW_OK;
    }
    int round_randv(int b, uint64_t seed, int32_t attempt, double* out, int64_t n) {
        MMW_TRY(check_inst(b));
        if (host_only) return host_only_batch();
        if (attempt < 0) return fail(MMW_ERR_ARG, "mmw_batch_round_randv: attempt must be >= 0");
        if (fdesc.empty() || fdesc[b].rank == 0) return fail(MMW_ERR_STATE, "mmw_batch_round_randv: instance " + std::to_string(b) + " has no factor (mmw_batch_factor)");
        const int Z = desc[b].Z, Dp = fdesc[b].rank;
        if (n != (int64_t)Z * Dp) return fail(MMW_ERR_ARG, "mmw_batch_round_randv: wrong length for a Z x rank block");
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(rvbuf.alloc((size_t)n));
        hipLaunchKernelGGL(k_batch_randv, dim3(1), dim3(BATCH_THREADS), 0, st, Z, Dp, seed, (uint32_t)attempt, rvbuf.p);
        MMW_HIP(hipGetLastError());
        return copy_d2h(out, rvbuf.p, (size_t)n * sizeof(double), st);
    }
    // ---- the sweeps' baselines
    // rand_sdp_solver.run_with_state (sdp_solver.py:109-114): the instance's sketch of (seed, iteration 0) as its resident factor, rank D
    int factor_random(const int32_t* take, const uint64_t* seeds) {
        if (host_only) return host_only_batch();
        std::vector<int> tk;
        MMW_TRY(takers("mmw_batch_factor_random", take, tk));
        for (int b : tk)
            if (desc[b].K > EPI_MAX_K)
                return fail(MMW_ERR_ARG, "mmw_batch_factor_random: instance " + std::to_string(b) + ": K = " + std::to_string(desc[b].K) +
                                             " exceeds the epilogue limit " + std::to_string(EPI_MAX_K) + " (round it on a handle)");
        auto a32 = [](int64_t x) { return (x + 31) & ~(int64_t)31; };
        std::vector<FactorDesc> fd(B, FactorDesc{});
        std::vector<FactorRandomDesc> launch;
        int64_t of = a32((int64_t)tk.size() * EPI_INFO_STRIDE), ninfo = 0;
        for (int b : tk) {
            FactorDesc& f = fd[b];
            f.K = desc[b].K; f.rank = desc[b].D; f.unit_rows = 1;
            f.o_info = EPI_INFO_STRIDE * ninfo++;
            f.o_fac = of; of = a32(of + (int64_t)f.K * f.rank);
            launch.push_back(FactorRandomDesc{f.K, f.rank, seeds[b], f.o_fac, f.o_info});
        }
        fdesc.clear();  // the buffers are laid out anew: earlier factors are gone whatever happens below
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(ew.alloc((size_t)of));
        MMW_TRY(d_frdesc.upload(launch, st));
        hipLaunchKernelGGL(k_batch_factor_random, dim3((unsigned)launch.size()), dim3(BATCH_THREADS), 0, st, d_frdesc.p, ew.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        fdesc = std::move(fd);
        return MMW_OK;
    }
    // the instance's state as the greedy procedures read it (host-only batch)
    GmState gm_state(int b) const {
        const HostPattern& P = H[b];
        GmState g;
        g.K = P.K; g.G = gmx[b].G; g.clique = gmx[b].clique;
        g.so_indptr = P.so_indptr; g.so_indices = P.so_indices; g.so_data = P.so_data;
        for (int32_t n : P.so_indices) g.so_hmax.push_back(P.h_max[n]);
        g.q_indptr = P.q_indptr; g.q_indices = P.q_indices; g.q_data = gmx[b].q_data;
        g.grp = gmx[b].grp; g.h_max = P.h_max;
        return g;
    }
    int gm_lists() {
        if (!gm_ogrp.empty()) return MMW_OK;
        std::vector<int> hi;
        std::vector<double> hf;
        std::vector<int64_t> og(B), oq(B);
        for (int b = 0; b < B; ++b) {
            og[b] = (int64_t)hi.size(); hi.insert(hi.end(), gmx[b].grp.begin(), gmx[b].grp.end());
            oq[b] = (int64_t)hf.size(); hf.insert(hf.end(), gmx[b].q_data.begin(), gmx[b].q_data.end());
        }
        MMW_TRY(gm_i.upload(hi, st));
        MMW_TRY(gm_f.upload(hf, st));
        gm_ogrp = std::move(og); gm_oq = std::move(oq);
        return MMW_OK;
    }
    int gm(int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out, int32_t* rem_out, double* key_out) {
        const std::string who = "mmw_batch_gm";
        MMW_TRY(batch_gm_args(who, kind, nattempt));
        std::vector<int> tk;
        MMW_TRY(takers(who.c_str(), take, tk));
        for (int b : tk) {
            const std::string inst = who + ": instance " + std::to_string(b);
            if (H[b].K > EPI_MAX_K) return fail(MMW_ERR_ARG, inst + ": K = " + std::to_string(H[b].K) + " exceeds the limit " + std::to_string(EPI_MAX_K) + " (it stays on a GreedyHandle)");
            if (!gmx[b].clique) return fail(MMW_ERR_ARG, inst + ": Q_asso is not a union of cliques with weights >= 1 (it stays on a GreedyHandle)");
        }
        if (host_only) {
            for (int b = 0; b < B; ++b) zz_out[b] = rem_out[b] = -1;
            std::vector<double> key;
            for (int b : tk) {
                const GmState g = gm_state(b);
                const int K = g.K, Zb = Z[b] <= 0 ? K : Z[b];
                g.key_host(kind, key);
                int entered = 0, stop = GM_STOP_SLOTS, total = 0;
                g.run_host(key.data(), Zb, nattempt, z_out, entered, stop, total);
                zz_out[b] = stop == GM_STOP_ALL_ASSIGNED ? entered : Zb;
                rem_out[b] = K - total;
                z_out += K;
                if (key_out) { std::copy(key.begin(), key.end(), key_out); key_out += K; }
            }
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(round_lists());
        MMW_TRY(gm_lists());
        std::vector<GmDesc> gd;
        for (int b : tk) {
            const RoundLists& l = rlists[b];
            GmDesc g{};
            g.K = H[b].K; g.G = gmx[b].G; g.kind = kind; g.Zb = Z[b] <= 0 ? g.K : Z[b]; g.nattempt = nattempt;
            g.s_soptr = l.soptr; g.s_soidx = l.soidx; g.s_qptr = l.qptr;
            g.s_sodata = l.sodata; g.s_sohmax = l.sohmax; g.s_hmax = l.hmax;
            g.g_grp = gm_ogrp[b]; g.g_qdata = gm_oq[b];
            gd.push_back(g);
        }
        return gmw.run(st, B, tk, gd, rs_i.p, rs_f.p, gm_i.p, gm_f.p, z_out, zz_out, rem_out, key_out);
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
