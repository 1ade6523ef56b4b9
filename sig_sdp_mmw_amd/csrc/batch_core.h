// What every part of the batched solver reads (batch_handle.h): the instances' host patterns (built by the host code mmw_create uses,
// build_pattern / update_slots), their run counters, and the int32 and the fp64 arena all of them are packed into.
//
// A batch built on the device (mmw_batch_create_from_env, batch_from_env.h) holds of every host pattern only what its creation read
// back: the sizes, l_indptr, S_sum, the squared row sums, h_max and the Z-dependent scalars.  It keeps its own device copy of the
// state (si / sf), and full(b) completes instance b's pattern from that copy with build_pattern the first time an entry needs a list.
#pragma once
#include <cstring>
#include <limits>
#include <stdexcept>

#include "kernels_batch.h"
#include "kernels_batch_carry.h"
#include "kernels_batch_pattern.h"
#include "kernels_batch_relayout.h"
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
// Row ranges of one instance (the row split's and the head split's): boundary p is the first row at which the prefix of indptr reaches
// p nnzL / rows (compared in integers), boundary `rows` is K.  Contiguous, a cover of [0, K), balanced by stored entries; ranges may be
// empty.  out: rows + 1 boundaries.
inline void batch_row_bounds(const int32_t* indptr, int K, int rows, int32_t* out) {
    const int64_t nnz = indptr[K];
    int r = 0;
    for (int p = 0; p < rows; ++p) {
        while (r < K && (int64_t)indptr[r] * rows < (int64_t)p * nnz) ++r;
        out[p] = r;
    }
    out[rows] = K;
}

struct BatchCore {
    int device = 0, B = 0, rank_radio = 2, max_order = MAX_ORDER;
    bool host_only = false;
    hipStream_t st = nullptr;
    double tol = 1e-9;
    std::vector<double> eta;  // per instance
    mutable std::vector<HostPattern> H;  // read through pat(b) / full(b)
    // built on the device: the state's copy (BatchPatItem says where instance b's lists lie) and, per instance, whether its host lists
    // are still to be fetched
    bool on_device = false;
    std::vector<BatchPatItem> sat;
    DevBuf<int> si;
    DevBuf<double> sf;
    mutable std::vector<char> lazy;
    std::vector<int> nit, iter;
    std::vector<char> active;
    std::vector<BatchDesc> desc;  // offsets and sizes; nrun / iter0 / seed / o_randv are set per call
    DevBuf<int> ia;
    DevBuf<double> fa;
    DevBuf<double> fb, rl;  // a slot change writes the fp64 arena anew into fb and swaps (relayout); rl is that call's upload
    DevBuf<BatchDesc> d_desc;
    // what every pattern holds from creation on: K, Z, the sizes, l_indptr, S_sum, h_max, norm_H, cH
    const HostPattern& pat(int b) const { return H[b]; }
    // the whole pattern; a failure on the way is thrown and reported by the entry (runtime.h guarded)
    const HostPattern& full(int b) const {
        if (on_device && lazy[b]) complete(b);
        return H[b];
    }
    void fetch(void* dst, const void* src, size_t bytes) const {
        if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
        if (copy_d2h(dst, src, bytes, st) != MMW_OK) throw std::runtime_error("reading the batch's copy of the state: " + last_error_ref());
    }
    // Q_asso of instance b from the batch's own copy of the state
    void fetch_q(int b, std::vector<int32_t>& qp, std::vector<int32_t>& qi, std::vector<double>& qx) const {
        const BatchPatItem& t = sat[b];
        const size_t K = (size_t)H[b].K;
        qp.resize(K + 1);
        fetch(qp.data(), si.p + t.c_qptr, (K + 1) * sizeof(int32_t));
        qi.resize((size_t)qp[K]); qx.resize((size_t)qp[K]);
        fetch(qi.data(), si.p + t.c_qidx, qi.size() * sizeof(int32_t));
        fetch(qx.data(), sf.p + t.v_qval, qx.size() * sizeof(double));
    }
    // S_gain, Q_asso and h_max of instance b from that copy
    void fetch_state(int b, std::vector<int32_t>& sp, std::vector<int32_t>& six, std::vector<double>& sx, std::vector<int32_t>& qp,
                     std::vector<int32_t>& qi, std::vector<double>& qx, std::vector<double>& h) const {
        const BatchPatItem& t = sat[b];
        const size_t K = (size_t)H[b].K;
        sp.resize(K + 1); h.resize(K);
        fetch(sp.data(), si.p + t.c_sptr, (K + 1) * sizeof(int32_t));
        fetch(h.data(), sf.p + t.v_hmax, K * sizeof(double));
        six.resize((size_t)sp[K]); sx.resize((size_t)sp[K]);
        fetch(six.data(), si.p + t.c_sidx, six.size() * sizeof(int32_t));
        fetch(sx.data(), sf.p + t.v_sval, sx.size() * sizeof(double));
        fetch_q(b, qp, qi, qx);
    }
    void complete(int b) const {
        std::vector<int32_t> sp, six, qp, qi;
        std::vector<double> sx, qx, h;
        fetch_state(b, sp, six, sx, qp, qi, qx, h);
        HostPattern T;
        const std::string err = build_pattern(T, H[b].K, H[b].Z, sp.data(), six.data(), sx.data(), qp.data(), qi.data(), qx.data(), h.data());
        if (!err.empty()) throw std::runtime_error("mmw_batch: instance " + std::to_string(b) + ": completing the host pattern: " + err);
        if (T.nnzL() != H[b].nnzL() || T.E_asso() != H[b].E_asso() || T.nnzST() != H[b].nnzST() || T.E_gain() != H[b].E_gain())
            throw std::runtime_error("mmw_batch: instance " + std::to_string(b) + ": the host pattern differs from the one built on the device");
        T.sq_sum = std::move(H[b].sq_sum);
        H[b] = std::move(T);
        lazy[b] = 0;
    }
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
    // Offsets of every instance for the slot counts the patterns hold now, used by creation and by every slot change: the int32 arena
    // never changes, the fp64 one follows the slot counts.  `out` is only written when every instance fits.
    int offsets(std::vector<BatchDesc>& out, int64_t& oi, int64_t& of) const {
        std::vector<BatchDesc> nd((size_t)B, BatchDesc{});
        oi = of = 0;
        for (int b = 0; b < B; ++b) {
            const HostPattern& P = H[b];
            BatchDesc& d = nd[b];
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
        out = std::move(nd);
        return MMW_OK;
    }
    // creation only: both arenas filled on the host (the fp64 one zero but for the pattern data) and uploaded whole
    int layout() {
        int64_t oi = 0, of = 0;
        MMW_TRY(offsets(desc, oi, of));
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
        for (int k = 0; k < d.K; ++k) init[d.o_xval - d.o_lval + full(b).diag_pos[k]] = 1.0;
        // the running sums start empty: iteration i adds X_i and Y_i when it starts, so after n iterations they hold X_0 + ... + X_{n-1}
        for (int c = 0; c < d.C; ++c) init[d.o_Y - d.o_lval + c] = 1.0 / (double)d.C;
        return copy_h2d(fa.p + d.o_lval, init.data(), init.size() * sizeof(double), st);
    }
    // the same for every instance of a batch built on the device, in one launch (k_batch_pattern_init): no host list is needed
    int init_point() {
        constexpr size_t DW = sizeof(BatchDesc) / sizeof(double);
        std::vector<double> stage(DW * B + (size_t)B);
        std::memcpy(stage.data(), desc.data(), sizeof(BatchDesc) * B);
        for (int b = 0; b < B; ++b) {
            iter[b] = 0;
            stage[DW * B + b] = 1.0 / (double)desc[b].C;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(rl.upload(stage, st));
        hipLaunchKernelGGL(k_batch_pattern_init, dim3(B), dim3(BATCH_THREADS), 0, st, (const BatchDesc*)rl.p, rl.p + DW * B, ia.p, fa.p, 1);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        return MMW_OK;
    }
    // A slot change on the device (kernels_batch_relayout.h).  The patterns hold the new slot counts already; mode[b] says what
    // instance b starts from.  One upload -- both descriptor tables, the per-instance items and the host-computed 1 / norm_H and cH --
    // one launch from `fa` into the second arena `fb` (made on the first slot change, grown only when the new layout needs more),
    // then the two trade places.  Every kernel takes fa.p as an argument of its launch, so nothing else has to be re-bound.
    int relayout(const std::vector<int>& mode) {
        std::vector<BatchDesc> nd;
        int64_t oi = 0, of = 0;
        MMW_TRY(offsets(nd, oi, of));
        constexpr size_t DW = sizeof(BatchDesc) / sizeof(double), IW = sizeof(RelayoutItem) / sizeof(double);
        static_assert(sizeof(BatchDesc) % sizeof(double) == 0 && sizeof(RelayoutItem) % sizeof(double) == 0, "the staging buffer is one array of doubles");
        int64_t Ksum = 0;
        for (int b = 0; b < B; ++b) Ksum += H[b].K;
        const size_t w_old = 0, w_new = w_old + DW * B, w_item = w_new + DW * B, w_invn = w_item + IW * B, w_cH = w_invn + (size_t)Ksum;
        std::vector<double> stage(w_cH + (size_t)Ksum);
        std::memcpy(stage.data() + w_old, desc.data(), sizeof(BatchDesc) * B);
        std::memcpy(stage.data() + w_new, nd.data(), sizeof(BatchDesc) * B);
        int64_t os = 0;
        for (int b = 0; b < B; ++b) {
            const HostPattern& P = H[b];
            const RelayoutItem t{mode[b], 0, os, 1.0 / (double)nd[b].C};
            std::memcpy(stage.data() + w_item + IW * b, &t, sizeof t);
            for (int k = 0; k < P.K; ++k) stage[w_invn + os + k] = 1.0 / P.norm_H[k];
            std::copy(P.cH.begin(), P.cH.end(), stage.begin() + w_cH + os);
            os += P.K;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(fb.alloc((size_t)of));
        MMW_TRY(rl.upload(stage, st));
        hipLaunchKernelGGL(k_batch_relayout, dim3(B), dim3(BATCH_THREADS), 0, st, (const BatchDesc*)(rl.p + w_old), (const BatchDesc*)(rl.p + w_new),
                           (const RelayoutItem*)(rl.p + w_item), rl.p + w_invn, rl.p + w_cH, ia.p, fa.p, fb.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        fa.swap(fb);
        desc = std::move(nd);
        return MMW_OK;
    }
    // (the index maps of a carry: carry_maps in pattern.h, which mmw_batch_carry and the solver handle's mmw_carry_map share)
};
