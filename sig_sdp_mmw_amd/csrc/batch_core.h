// What every part of the batched solver reads (batch_handle.h): the instances' host patterns (built by the host code mmw_create uses,
// build_pattern / update_slots), their run counters, and the int32 and the fp64 arena all of them are packed into.
#pragma once
#include <limits>

#include "kernels_batch.h"
#include "solver.h"

// the instances of a call: those `take` flags, or every active one (take null).  `active` null: every instance is active.
inline int batch_takers(const char* who, int B, const int32_t* take, const char* active, std::vector<int>& tk) {
    tk.clear();
    for (int b = 0; b < B; ++b) {
        const bool act = !active || active[b];
        if (take ? take[b] == 0 : !act) continue;
        if (!act) return fail(MMW_ERR_STATE, std::string(who) + ": instance " + std::to_string(b) + " sits out (mmw_batch_set_slots gave it no slot count)");
        tk.push_back(b);
    }
    if (tk.empty()) return fail(MMW_ERR_ARG, std::string(who) + ": no instance takes part");
    return MMW_OK;
}
// workgroups per instance as the entry `who` takes them, 1 ... maxp each (null or all ones: `dst` empty, the unsplit path)
inline int check_parts(const char* who, const int32_t* p, int B, std::vector<int>& dst, int maxp = MMW_BATCH_MAX_PARTS) {
    bool any = false;
    for (int b = 0; p && b < B; ++b) {
        if (p[b] < 1 || p[b] > maxp)
            return fail(MMW_ERR_ARG, std::string(who) + ": instance " + std::to_string(b) + ": parts = " + std::to_string(p[b]) + " is outside [1, " +
                                         std::to_string(maxp) + "]");
        any = any || p[b] > 1;
    }
    if (any) dst.assign(p, p + B);
    else dst.clear();
    return MMW_OK;
}

struct BatchCore {
    int device = 0, B = 0, rank_radio = 2, max_order = MAX_ORDER;
    bool host_only = false;
    hipStream_t st = nullptr;
    double tol = 1e-9;
    std::vector<double> eta;  // per instance
    std::vector<HostPattern> H;
    std::vector<int> nit, iter;
    std::vector<char> active;
    std::vector<BatchDesc> desc;  // offsets and sizes; nrun / iter0 / seed / o_randv are set per call
    DevBuf<int> ia;
    DevBuf<double> fa;
    DevBuf<BatchDesc> d_desc;
    static int host_only_batch() { return fail(MMW_ERR_STATE, "this batch was created with device -1 (host patterns only)"); }
    int check_inst(int b) const {
        if (b < 0 || b >= B) return fail(MMW_ERR_ARG, "mmw_batch: instance index out of range");
        return MMW_OK;
    }
    int takers(const char* who, const int32_t* take, std::vector<int>& tk) const { return batch_takers(who, B, take, active.data(), tk); }
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
    // the reference's initial point (mmw.py:62-73) of one instance: Y = 1/C, X = I, L = 0, sums zero
    int reset_one(int b) {
        iter[b] = 0;
        const BatchDesc& d = desc[b];
        std::vector<double> init((size_t)(d.o_info - d.o_lval), 0.0);  // the iterate (lval ... W2) in one copy
        for (int k = 0; k < d.K; ++k) init[d.o_xval - d.o_lval + H[b].diag_pos[k]] = 1.0;
        // the running sums start empty: iteration i adds X_i and Y_i when it starts, so after n iterations they hold X_0 + ... + X_{n-1}
        for (int c = 0; c < d.C; ++c) init[d.o_Y - d.o_lval + c] = 1.0 / (double)d.C;
        return copy_h2d(fa.p + d.o_lval, init.data(), init.size() * sizeof(double), st);
    }
};
