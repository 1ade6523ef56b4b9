// A state that lives on the device as its seven CSR arrays (mmw_csr, include/mmw_hip.h): S_gain and Q_asso as (indptr int32 [K+1],
// indices int32 [nnz], data f64 [nnz]) and h_max f64 [K].  The arrays are the library's own copies (mmw_csr_upload) or borrowed from the
// caller (mmw_csr_wrap: a graph built on the GPU by someone else); device -1 keeps host copies for the CPU suite.  The lengths are always
// the caller's announcement, never read from an array.  The handle validates its arrays once (pattern_csr_device.h) -- they do not change
// while it lives -- and whoever reads columns as addresses (the bounds, mmw_create_from_csr) asks for that verdict first.
#pragma once
#include "pattern_csr_device.h"

namespace mmw {

struct CsrDevice {
    int device = -1;
    bool host_only = false;
    hipStream_t st = nullptr;
    CsrView V;  // the arrays every reader uses: the owned copies, the borrowed pointers, or (host_only) the host vectors
    DevBuf<int> sp, si, qp, qi;
    DevBuf<double> sx, qx, hm;
    std::vector<int32_t> h_sp, h_si, h_qp, h_qi;
    std::vector<double> h_sx, h_qx, h_hm;
    bool checked = false;
    unsigned long long err[CSR_PHASES] = {CSR_OK, CSR_OK, CSR_OK};
    DevBuf<unsigned long long> d_err;
    bool have_bounds = false;
    int32_t bnd[2] = {0, 0};

    ~CsrDevice() {
        if (st) {
            (void)hipSetDevice(device);
            (void)hipStreamDestroy(st);
        }
    }
    static int check_sizes(const char* who, int32_t K, int64_t nnzS, int64_t nnzQ) {
        if (K < 1) return fail(MMW_ERR_ARG, std::string(who) + ": K must be positive");
        if (nnzS < 0 || nnzQ < 0 || nnzS > (int64_t)INT32_MAX || nnzQ > (int64_t)INT32_MAX) return fail(MMW_ERR_ARG, std::string(who) + ": nnz must be in [0, 2^31)");
        return MMW_OK;
    }
    int open(int dev) {
        device = dev;
        MMW_HIP(hipSetDevice(device));
        MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return MMW_OK;
    }
    int upload(int dev, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* Sp, const int32_t* Si, const double* Sx, const int32_t* Qp, const int32_t* Qi,
               const double* Qx, const double* h) {
        V.K = K; V.nnzS = (int)nnzS; V.nnzQ = (int)nnzQ;
        h_sp.assign(Sp, Sp + K + 1); h_qp.assign(Qp, Qp + K + 1); h_hm.assign(h, h + K);
        if (nnzS) { h_si.assign(Si, Si + nnzS); h_sx.assign(Sx, Sx + nnzS); }
        if (nnzQ) { h_qi.assign(Qi, Qi + nnzQ); h_qx.assign(Qx, Qx + nnzQ); }
        if (dev == -1) {
            host_only = true;
            V.Sp = h_sp.data(); V.Si = h_si.data(); V.Sx = h_sx.data(); V.Qp = h_qp.data(); V.Qi = h_qi.data(); V.Qx = h_qx.data(); V.h = h_hm.data();
            return MMW_OK;
        }
        MMW_TRY(open(dev));
        MMW_TRY(sp.upload(h_sp, st)); MMW_TRY(si.upload(h_si, st)); MMW_TRY(sx.upload(h_sx, st));
        MMW_TRY(qp.upload(h_qp, st)); MMW_TRY(qi.upload(h_qi, st)); MMW_TRY(qx.upload(h_qx, st)); MMW_TRY(hm.upload(h_hm, st));
        V.Sp = sp.p; V.Si = si.p; V.Sx = sx.p; V.Qp = qp.p; V.Qi = qi.p; V.Qx = qx.p; V.h = hm.p;
        for (auto* v : {&h_sp, &h_si, &h_qp, &h_qi}) std::vector<int32_t>().swap(*v);  // the state lives on the device from here on
        for (auto* v : {&h_sx, &h_qx, &h_hm}) std::vector<double>().swap(*v);
        return MMW_OK;
    }
    int wrap(int dev, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* Sp, const int32_t* Si, const double* Sx, const int32_t* Qp, const int32_t* Qi,
             const double* Qx, const double* h) {
        MMW_TRY(open(dev));
        V.K = K; V.nnzS = (int)nnzS; V.nnzQ = (int)nnzQ;
        V.Sp = Sp; V.Si = Si; V.Sx = Sx; V.Qp = Qp; V.Qi = Qi; V.Qx = Qx; V.h = h;
        return MMW_OK;
    }
    void pointers(void* out[7]) const {
        const void* p[7] = {V.Sp, V.Si, V.Sx, V.Qp, V.Qi, V.Qx, V.h};
        for (int i = 0; i < 7; ++i) out[i] = host_only ? nullptr : const_cast<void*>(p[i]);
        if (!host_only && V.nnzS == 0) out[1] = out[2] = nullptr;  // (an owned empty array is a one-element allocation: hand out what wrap takes)
        if (!host_only && V.nnzQ == 0) out[4] = out[5] = nullptr;
    }
    // the host copy of the state, made on request
    int state(int32_t* Sp, int32_t* Si, double* Sx, int32_t* Qp, int32_t* Qi, double* Qx, double* h) {
        const size_t K = (size_t)V.K, ns = (size_t)V.nnzS, nq = (size_t)V.nnzQ;
        if (host_only) {
            memcpy(Sp, V.Sp, (K + 1) * sizeof(int32_t)); memcpy(Qp, V.Qp, (K + 1) * sizeof(int32_t)); memcpy(h, V.h, K * sizeof(double));
            if (ns) { memcpy(Si, V.Si, ns * sizeof(int32_t)); memcpy(Sx, V.Sx, ns * sizeof(double)); }
            if (nq) { memcpy(Qi, V.Qi, nq * sizeof(int32_t)); memcpy(Qx, V.Qx, nq * sizeof(double)); }
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(copy_d2h(Sp, V.Sp, (K + 1) * sizeof(int32_t), st)); MMW_TRY(copy_d2h(Si, V.Si, ns * sizeof(int32_t), st)); MMW_TRY(copy_d2h(Sx, V.Sx, ns * sizeof(double), st));
        MMW_TRY(copy_d2h(Qp, V.Qp, (K + 1) * sizeof(int32_t), st)); MMW_TRY(copy_d2h(Qi, V.Qi, nq * sizeof(int32_t), st)); MMW_TRY(copy_d2h(Qx, V.Qx, nq * sizeof(double), st));
        return copy_d2h(h, V.h, K * sizeof(double), st);
    }
    // the three validation launches on `s` (not waited for): whoever enqueues behind them on `s` tests d_err itself
    int enqueue_checks(hipStream_t s) {
        MMW_TRY(d_err.alloc(CSR_PHASES));
        MMW_HIP(hipMemsetAsync(d_err.p, 0xff, CSR_PHASES * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_csr_check, dim3(grid_elems((size_t)V.K)), dim3(BLOCK), 0, s, V, 0, d_err.p);
        hipLaunchKernelGGL(k_csr_check, dim3(grid_rows(V.K)), dim3(BLOCK), 0, s, V, 1, d_err.p);
        hipLaunchKernelGGL(k_csr_check, dim3(grid_rows(V.K)), dim3(BLOCK), 0, s, V, 2, d_err.p);
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    // the verdict: MMW_OK, or MMW_ERR_ARG with `who`: and build_pattern's words for the first error in (class, row) order
    int verdict(const char* who) const {
        for (int p = 0; p < CSR_PHASES; ++p)
            if (err[p] != CSR_OK) return fail(MMW_ERR_ARG, std::string(who) + ": " + csr_err_text(err[p]));
        return MMW_OK;
    }
    int validate(const char* who) {
        if (!checked) {
            if (host_only) csr_check_host(V, err);
            else {
                MMW_HIP(hipSetDevice(device));
                MMW_TRY(enqueue_checks(st));
                MMW_TRY(copy_d2h(err, d_err.p, sizeof err, st));
            }
            checked = true;
        }
        return verdict(who);
    }
    // binary_search_relaxation.set_bounds: lower = longest Q row + 1, upper = max_a #{j != a : S[a,j] != 0 or S[j,a] != 0} + 2
    int bounds(int32_t out[2]) {
        if (!have_bounds) {
            MMW_TRY(validate("mmw_csr_bounds"));
            const int K = V.K;
            std::vector<int32_t> row_only((size_t)K, 0), col_cnt((size_t)K, 0), qptr((size_t)K + 1);
            if (host_only) {
                for (int a = 0; a < K; ++a)
                    for (int i = V.Sp[a]; i < V.Sp[a + 1]; ++i) {
                        const int c = V.Si[i];
                        if (c == a || V.Sx[i] == 0.0) continue;
                        ++col_cnt[c];
                        const int w = csr_lower(V.Si, V.Sp[c], V.Sp[c + 1], a);
                        if (!(w < V.Sp[c + 1] && V.Si[w] == a && V.Sx[w] != 0.0)) ++row_only[a];
                    }
                memcpy(qptr.data(), V.Qp, qptr.size() * sizeof(int32_t));
            } else {
                MMW_HIP(hipSetDevice(device));
                DevBuf<int> cnt;
                MMW_TRY(cnt.alloc((size_t)2 * K));
                MMW_HIP(hipMemsetAsync(cnt.p, 0, (size_t)2 * K * sizeof(int), st));
                hipLaunchKernelGGL(k_csr_sym_count, dim3(grid_rows(K)), dim3(BLOCK), 0, st, V, (const unsigned long long*)d_err.p, cnt.p, cnt.p + K);
                MMW_HIP(hipGetLastError());
                MMW_TRY(copy_d2h(row_only.data(), cnt.p, (size_t)K * sizeof(int), st));
                MMW_TRY(copy_d2h(col_cnt.data(), cnt.p + K, (size_t)K * sizeof(int), st));
                MMW_TRY(copy_d2h(qptr.data(), V.Qp, qptr.size() * sizeof(int32_t), st));
            }
            int lb = 0, ub = 0;
            for (int k = 0; k < K; ++k) {
                lb = std::max(lb, qptr[k + 1] - qptr[k]);
                ub = std::max(ub, row_only[k] + col_cnt[k]);
            }
            bnd[0] = lb + 1; bnd[1] = ub + 2;
            have_bounds = true;
        }
        out[0] = bnd[0]; out[1] = bnd[1];
        return MMW_OK;
    }
};

}  // namespace mmw
