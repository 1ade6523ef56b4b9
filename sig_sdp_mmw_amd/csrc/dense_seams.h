// The factor's dense building blocks as handle-less calls (mmw_dense_gram / _gemm / _chol / _orth, include/mmw_hip.h): each runs one
// operation of DenseWork<T> / Factorizer<T> (factor.h) on blocks that come and go as float64 host arrays, so that a test can hold the
// operation against the same operation in NumPy.  The switches are read at the call (MMW_CHOL_LDS, MMW_FACTOR_NO_NS).
#pragma once
#include <vector>

#include "factor.h"

namespace mmw {

// a float64 host array on the device as T (rounded on the host, as the factor's blocks are stored)
template <typename T> int dense_upload(DevBuf<T>& d, const double* h, size_t n, hipStream_t st) {
    std::vector<T> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (T)h[i];
    MMW_TRY(d.alloc(n));
    return copy_h2d(d.p, tmp.data(), n * sizeof(T), st);
}
template <typename T> int dense_download(double* h, const T* d, size_t n, hipStream_t st) {
    std::vector<T> tmp(n);
    MMW_TRY(copy_d2h(tmp.data(), d, n * sizeof(T), st));
    for (size_t i = 0; i < n; ++i) h[i] = (double)tmp[i];
    return MMW_OK;
}

template <typename T> int dense_gram_impl(hipStream_t st, int K, int b, int ld, const double* V, const double* W, bool sym, double* G_out) {
    const Switches switches = Switches::from_env();
    DenseWork<T> dw(switches);
    dw.st = st;
    DevBuf<T> dV, dW;
    MMW_TRY(dense_upload(dV, V, (size_t)K * ld, st));
    MMW_TRY(dense_upload(dW, W, (size_t)K * ld, st));
    MMW_TRY(dw.gram(K, b, ld, dV.p, dW.p, sym));
    return copy_d2h(G_out, dw.G.p, (size_t)b * b * sizeof(double), st);
}

template <typename T> int dense_gemm_impl(hipStream_t st, int K, int b, int n, int ld, const double* V, int ldq, const double* Q, double* C_out) {
    const Switches switches = Switches::from_env();
    DenseWork<T> dw(switches);
    dw.st = st;
    DevBuf<T> dV, dC;
    DevBuf<double> dQ;
    MMW_TRY(dense_upload(dV, V, (size_t)K * ld, st));
    MMW_TRY(dense_upload(dQ, Q, (size_t)b * ldq, st));
    MMW_TRY(dC.alloc((size_t)K * ld));
    MMW_HIP(hipMemsetAsync(dC.p, 0, (size_t)K * ld * sizeof(T), st));
    MMW_TRY(dw.gemm(K, b, n, ld, dV.p, dQ.p, ldq, dC.p));
    return dense_download(C_out, dC.p, (size_t)K * ld, st);
}

inline int dense_chol_impl(hipStream_t st, int b, const double* G, double* L_out, double* dscale_out, double* dinv_out, int32_t* ok) {
    const Switches switches = Switches::from_env();
    DenseWork<double> dw(switches);
    dw.st = st;
    MMW_TRY(dw.ensure(b, 1));
    const size_t n_inv = (size_t)((b + CH_NB - 1) / CH_NB) * CH_NB * CH_NB;
    MMW_TRY(dw.dinv.alloc(n_inv));
    MMW_HIP(hipMemsetAsync(dw.dinv.p, 0, n_inv * sizeof(double), st));  // (a failed factorisation leaves the later panels' inverses unwritten)
    MMW_TRY(copy_h2d(dw.G.p, G, (size_t)b * b * sizeof(double), st));
    bool good = false;
    MMW_TRY(dw.chol_factor(b, &good));
    MMW_TRY(copy_d2h(L_out, dw.G.p, (size_t)b * b * sizeof(double), st));
    for (int i = 0; i < b; ++i)
        for (int j = i + 1; j < b; ++j) L_out[(size_t)i * b + j] = 0.0;  // the factorisation never touches what lies above the diagonal
    MMW_TRY(copy_d2h(dscale_out, dw.dscale.p, (size_t)b * sizeof(double), st));
    MMW_TRY(copy_d2h(dinv_out, dw.dinv.p, n_inv * sizeof(double), st));
    *ok = good ? 1 : 0;
    return MMW_OK;
}

template <typename T> int dense_orth_impl(hipStream_t st, int K, int b, int ld, const double* V, double eps, double* Q_out, int32_t* path_out) {
    const Switches switches = Switches::from_env();
    Factorizer<T> f(switches);
    MMW_TRY(f.init(st, K, nullptr));
    DevBuf<T> A, B;
    MMW_TRY(dense_upload(A, V, (size_t)K * ld, st));
    MMW_TRY(B.alloc((size_t)K * ld));
    int path[2] = {-1, -1};
    MMW_TRY(f.orthonormalise(b, ld, A, B, eps, path));
    MMW_TRY(dense_download(Q_out, A.p, (size_t)K * ld, st));
    path_out[0] = path[0];
    path_out[1] = path[1];
    return MMW_OK;
}

inline int dense_shape(const char* who, int32_t K, int32_t b, int32_t ld) {
    if (K < 1) return fail(MMW_ERR_ARG, std::string(who) + ": K must be >= 1");
    if (b < 1 || b > 2048) return fail(MMW_ERR_ARG, std::string(who) + ": b must be in [1, 2048]");
    if (ld < b) return fail(MMW_ERR_ARG, std::string(who) + ": ld must be >= b");
    return MMW_OK;
}
// the checks every dtype-taking call shares, then a stream of the call's own
template <typename F32Call, typename F64Call> int dense_call(const char* who, int device, int dtype, F32Call&& f32, F64Call&& f64) {
    if (dtype != MMW_F32 && dtype != MMW_F64) return fail(MMW_ERR_ARG, std::string(who) + ": dtype must be MMW_F32 or MMW_F64");
    MMW_TRY(check_device(who, device, DEV_BARE));
    MMW_HIP(hipSetDevice(device));
    ScopedStream stream;
    MMW_HIP(hipStreamCreate(&stream.s));
    return dtype == MMW_F32 ? f32(stream.s) : f64(stream.s);
}

}  // namespace mmw
