// C-ABI of the MI355X MMW hot path (include/mmw_hip.h), the library's one translation unit.  The handles: solver.h (mmw_solver, mmw_env),
// gm_handle.h (mmw_gm), batch_handle.h (mmw_batch: batch_core.h and the parts' headers), batch_env_handle.h (mmw_batch_env), batch_from_env.h and batch_from_csr.h (a batch built on the device, from an environment or from CSR states).  Every entry that can throw runs inside guarded() (runtime.h): no C++ exception crosses the C boundary.
#include "batch_env_handle.h"
#include "batch_from_csr.h"
#include "batch_from_env.h"
#include "batch_handle.h"
#include "dense_seams.h"
#include "gm_handle.h"

using namespace mmw;

extern "C" {
const char* mmw_last_error(void) { return last_error_ref().c_str(); }
int mmw_version(void) { return 300; }
int mmw_device_count(int* n) { return guarded("mmw_device_count", [&]() -> int { return device_count(n); }); }
int mmw_create(mmw_solver** out, int device, int dtype, int32_t K, int32_t Z, int32_t rank_radio, double eta, int32_t nit,
               const int32_t* S_indptr, const int32_t* S_indices, const double* S_data, const int32_t* Q_indptr,
               const int32_t* Q_indices, const double* Q_data, const double* h_max) {
    return guarded("mmw_create", [&]() -> int {
        if (!out || !S_indptr || !S_indices || !S_data || !Q_indptr || !Q_indices || !Q_data || !h_max)
            return fail(MMW_ERR_ARG, "mmw_create: null pointer");
        *out = nullptr;
        if (rank_radio < 1) return fail(MMW_ERR_ARG, "rank_radio must be >= 1");
        if (nit < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        const bool host_only = device == -1;
        if (!host_only) MMW_TRY(check_device("mmw_create", device, DEV_ID_VISIBLE));
        return create_solver(out, dtype, host_only, [&](auto& s) {
            return std::decay_t<decltype(s)>::Create::init(s, device, K, Z, rank_radio, eta, nit, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max);
        });
    });
}
int mmw_create_from_env(mmw_solver** out, mmw_env* env, int dtype, int32_t Z, int32_t rank_radio, double eta, int32_t nit) {
    return guarded("mmw_create_from_env", [&]() -> int {
        if (!out || !env) return fail(MMW_ERR_ARG, "mmw_create_from_env: null pointer");
        *out = nullptr;
        if (rank_radio < 1) return fail(MMW_ERR_ARG, "rank_radio must be >= 1");
        if (nit < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        return create_solver(out, dtype, false, [&](auto& s) { return std::decay_t<decltype(s)>::Create::init_env(s, env->e.device, env->e, Z, rank_radio, eta, nit); });
    });
}
int mmw_env_bounds(mmw_env* e, int32_t out[2]) { return entry("mmw_env_bounds", !e || !out, "null pointer", [&] { return e->e.bounds(out); }); }
// ---- a state on the device as its seven CSR arrays (csr_device.h) and the handle built from it there (solver_create.h: init_csr)
static int csr_make(const char* who, bool borrow, mmw_csr** out, int device, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* Sp, const int32_t* Si, const double* Sx,
                    const int32_t* Qp, const int32_t* Qi, const double* Qx, const double* h) {
    return guarded(who, [&]() -> int {
        if (!out) return fail(MMW_ERR_ARG, std::string(who) + ": null pointer");
        *out = nullptr;
        MMW_TRY(CsrDevice::check_sizes(who, K, nnzS, nnzQ));
        if (!Sp || !Qp || !h || (nnzS && (!Si || !Sx)) || (nnzQ && (!Qi || !Qx))) return fail(MMW_ERR_ARG, std::string(who) + ": null pointer (an array may be null only where its length is 0)");
        if (borrow && device == -1) return fail(MMW_ERR_ARG, std::string(who) + ": device -1 (host only) has no device pointers to borrow: use mmw_csr_upload");
        if (device != -1) MMW_TRY(check_device(who, device, DEV_ID_VISIBLE));
        auto c = std::make_unique<mmw_csr>();
        MMW_TRY(borrow ? c->c.wrap(device, K, nnzS, nnzQ, Sp, Si, Sx, Qp, Qi, Qx, h) : c->c.upload(device, K, nnzS, nnzQ, Sp, Si, Sx, Qp, Qi, Qx, h));
        *out = c.release();
        return MMW_OK;
    });
}
int mmw_csr_upload(mmw_csr** out, int device, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* S_indptr, const int32_t* S_indices, const double* S_data,
                   const int32_t* Q_indptr, const int32_t* Q_indices, const double* Q_data, const double* h_max) {
    return csr_make("mmw_csr_upload", false, out, device, K, nnzS, nnzQ, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max);
}
int mmw_csr_wrap(mmw_csr** out, int device, int32_t K, int64_t nnzS, int64_t nnzQ, const int32_t* S_indptr, const int32_t* S_indices, const double* S_data,
                 const int32_t* Q_indptr, const int32_t* Q_indices, const double* Q_data, const double* h_max) {
    return csr_make("mmw_csr_wrap", true, out, device, K, nnzS, nnzQ, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max);
}
int mmw_csr_destroy(mmw_csr* c) { return guarded("mmw_csr_destroy", [&]() -> int { delete c; return MMW_OK; }); }
int mmw_csr_sizes(mmw_csr* c, int64_t out[4]) {
    return entry("mmw_csr_sizes", !c || !out, "null pointer", [&] {
        out[0] = c->c.V.K; out[1] = 0; out[2] = c->c.V.nnzS; out[3] = c->c.V.nnzQ;
        return MMW_OK;
    });
}
int mmw_csr_pointers(mmw_csr* c, void* out[7]) {
    return entry("mmw_csr_pointers", !c || !out, "null pointer", [&] {
        c->c.pointers(out);
        return MMW_OK;
    });
}
int mmw_csr_state(mmw_csr* c, int32_t* S_indptr, int32_t* S_indices, double* S_data, int32_t* Q_indptr, int32_t* Q_indices, double* Q_data, double* h_max) {
    return entry("mmw_csr_state", !c || !S_indptr || !Q_indptr || !h_max || (c && c->c.V.nnzS && (!S_indices || !S_data)) || (c && c->c.V.nnzQ && (!Q_indices || !Q_data)),
                 "mmw_csr_state: null pointer", [&] { return c->c.state(S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max); });
}
int mmw_csr_bounds(mmw_csr* c, int32_t out[2]) { return entry("mmw_csr_bounds", !c || !out, "null pointer", [&] { return c->c.bounds(out); }); }
int mmw_create_from_csr(mmw_solver** out, mmw_csr* csr, int dtype, int32_t Z, int32_t rank_radio, double eta, int32_t nit) {
    return guarded("mmw_create_from_csr", [&]() -> int {
        if (!out || !csr) return fail(MMW_ERR_ARG, "mmw_create_from_csr: null pointer");
        *out = nullptr;
        if (rank_radio < 1) return fail(MMW_ERR_ARG, "rank_radio must be >= 1");
        if (nit < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        return create_solver(out, dtype, csr->c.host_only, [&](auto& s) { return std::decay_t<decltype(s)>::Create::init_csr(s, csr->c, Z, rank_radio, eta, nit); });
    });
}
int mmw_destroy(mmw_solver* s) { return guarded("mmw_destroy", [&]() -> int { delete s; return MMW_OK; }); }
int mmw_sizes(mmw_solver* s, int64_t out[10]) { return entry("mmw_sizes", !s, "null solver handle", [&] { return s->sizes(out); }); }
int mmw_set_expm(mmw_solver* s, int method, int max_order, double tol) { return entry("mmw_set_expm", !s, "null solver handle", [&] { return s->set_expm(method, max_order, tol); }); }
int mmw_set_timing(mmw_solver* s, int enabled) { return entry("mmw_set_timing", !s, "null solver handle", [&] { return s->set_timing(enabled); }); }
int mmw_set_profile(mmw_solver* s, int enabled) { return entry("mmw_set_profile", !s, "null solver handle", [&] { return s->set_profile(enabled); }); }
int mmw_bench_spmm(mmw_solver* s, int blocked, int reps, double* avg_us) { return entry("mmw_bench_spmm", !s, "null solver handle", [&] { return s->bench_spmm(blocked, reps, avg_us); }); }
int mmw_reset(mmw_solver* s, int32_t nit) { return entry("mmw_reset", !s, "null solver handle", [&] { return s->reset(nit); }); }
int mmw_set_slots(mmw_solver* s, int32_t Z, int32_t nit) { return entry("mmw_set_slots", !s, "null solver handle", [&] { return s->set_slots(Z, nit, 0); }); }
int mmw_set_slots_warm(mmw_solver* s, int32_t Z, int32_t nit) { return entry("mmw_set_slots_warm", !s, "null solver handle", [&] { return s->set_slots(Z, nit, 1); }); }
// ---- the iterate carried from a handle on the state before the stations moved to one on the state after (solver_carry.h)
int mmw_carry(mmw_solver* dst, mmw_solver* src) { return entry("mmw_carry", !dst || !src, "null solver handle", [&] { return dst->carry(src); }); }
int mmw_carry_map(mmw_solver* dst, mmw_solver* src, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc) {
    return entry("mmw_carry_map", !dst || !src || (!lmap && nl) || (!cmap && nc), "null pointer", [&]() -> int {
        MMW_TRY(carry_refusal("mmw_carry_map", dst->carry_info(), src->carry_info(), false));
        const HostPattern* N = nullptr;
        const HostPattern* O = nullptr;
        MMW_TRY(dst->carry_pattern(&N));
        MMW_TRY(src->carry_pattern(&O));
        if (nl != N->nnzL() || nc != N->C())
            return fail(MMW_ERR_ARG, "mmw_carry_map: wrong lengths " + std::to_string(nl) + ", " + std::to_string(nc) + ", expected nnzL = " + std::to_string(N->nnzL()) +
                                         " and C = " + std::to_string(N->C()));
        carry_maps(*N, *O, lmap, cmap);
        return MMW_OK;
    });
}
int mmw_set_eta(mmw_solver* s, double eta) { return entry("mmw_set_eta", !s, "null solver handle", [&] { return s->set_eta(eta); }); }
int mmw_iterate(mmw_solver* s, int32_t n, const double* randv, uint64_t seed) { return entry("mmw_iterate", !s, "null solver handle", [&] { return s->iterate(n, randv, seed); }); }
int mmw_sync(mmw_solver* s) { return entry("mmw_sync", !s, "null solver handle", [&] { return s->sync(); }); }
int mmw_sketch(mmw_solver* s, uint64_t seed, int32_t iteration, double* out, int64_t n) { return entry("mmw_sketch", !s, "null solver handle", [&] { return !out && n ? fail(MMW_ERR_ARG, "null output") : s->sketch(seed, iteration, out, n); }); }
int mmw_read_f64(mmw_solver* s, int which, double* out, int64_t n) { return entry("mmw_read_f64", !s, "null solver handle", [&] { return !out && n ? fail(MMW_ERR_ARG, "null output") : s->read_f64(which, out, n); }); }
int mmw_read_i32(mmw_solver* s, int which, int32_t* out, int64_t n) { return entry("mmw_read_i32", !s, "null solver handle", [&] { return !out && n ? fail(MMW_ERR_ARG, "null output") : s->read_i32(which, out, n); }); }
int mmw_gap(mmw_solver* s, double out[3]) { return entry("mmw_gap", !s, "null solver handle", [&] { return s->gap(out); }); }
int mmw_set_gap(mmw_solver* s, int enabled, int32_t m_cap, int32_t first_steps) { return entry("mmw_set_gap", !s, "null solver handle", [&] { return s->set_gap(enabled, m_cap, first_steps); }); }
int mmw_read_gap(mmw_solver* s, double* out, int64_t n) { return entry("mmw_read_gap", !s || (!out && n), "null pointer", [&] { return s->read_gap(out, n); }); }
int mmw_gap_checks(int32_t K, int32_t m_cap, int32_t* out, int32_t room, int32_t* n) {
    return entry("mmw_gap_checks", !n, "null pointer", [&] {
        if (K < 1) return fail(MMW_ERR_ARG, "mmw_gap_checks: K must be >= 1");
        if (m_cap > GAP_MAX_M) return fail(MMW_ERR_ARG, "mmw_gap_checks: m_cap = " + std::to_string(m_cap) + " exceeds " + std::to_string(GAP_MAX_M));
        const std::vector<int> c = gap_check_list(K, m_cap <= 0 ? GAP_DEFAULT_M : m_cap);
        *n = (int32_t)c.size();
        if (out && room < (int32_t)c.size()) return fail(MMW_ERR_ARG, "mmw_gap_checks: room for " + std::to_string(room) + " of " + std::to_string(c.size()) + " checks");
        if (out) std::copy(c.begin(), c.end(), out);
        return MMW_OK;
    });
}
int mmw_factor(mmw_solver* s, int32_t rank, double* out, uint64_t seed) { return entry("mmw_factor", !s, "null solver handle", [&] { return s->factor(rank, out, seed); }); }
int mmw_factor_spectral(mmw_solver* s, int32_t Z, int32_t index_order, double* out, uint64_t seed) {
    return entry("mmw_factor_spectral", !s, "null solver handle", [&] { return s->factor_spectral(Z, index_order, out, seed); });
}
int mmw_factor_random(mmw_solver* s, int32_t cols, int32_t index_order, double* out, uint64_t seed) {
    return entry("mmw_factor_random", !s, "mmw_factor_random: null solver handle", [&] { return s->factor_random(cols, index_order, out, seed); });
}
int mmw_round(mmw_solver* s, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out, int32_t* rem_out) {
    return entry("mmw_round", !s, "null solver handle", [&] { return s->round(Zr, Dp, gX, nbatch, randv, z_out, rem_out); });
}
int mmw_expm_apply(int device, int dtype, int method, int max_order, double tol, int32_t K, int32_t D, const int32_t* indptr,
                   const int32_t* indices, const double* data, const double* B, double* out, double info[4], int32_t reps,
                   double* kernel_us) {
    return guarded("mmw_expm_apply", [&]() -> int {
        if (!indptr || !indices || !data || !B || !out) return fail(MMW_ERR_ARG, "mmw_expm_apply: null pointer");
        if (K < 1 || D < 1) return fail(MMW_ERR_ARG, "mmw_expm_apply: K and D must be positive");
        if (max_order < 1 || max_order > MAX_ORDER) return fail(MMW_ERR_ARG, "max_order must be in [1,16]");
        if (method != MMW_EXPM_LANCZOS && method != MMW_EXPM_TAYLOR) return fail(MMW_ERR_ARG, "unknown expm method");
        MMW_TRY(check_device("mmw_expm_apply", device, DEV_BARE));
        const Switches sw = Switches::from_env();
        if (dtype == MMW_F32) return expm_apply_impl<float>(sw, device, method, max_order, tol, K, D, indptr, indices, data, B, out, info, reps, kernel_us);
        if (dtype == MMW_F64) return expm_apply_impl<double>(sw, device, method, max_order, tol, K, D, indptr, indices, data, B, out, info, reps, kernel_us);
        return fail(MMW_ERR_ARG, "dtype must be MMW_F32 or MMW_F64");
    });
}
int mmw_sym_eig(int device, int32_t b, const double* G, double rel_tol, int32_t max_sweeps, double* theta, double* Q, int32_t* sweeps) {
    return guarded("mmw_sym_eig", [&]() -> int {
        if (!G || !theta || !Q) return fail(MMW_ERR_ARG, "mmw_sym_eig: null pointer");
        if (b < 1 || b > 2048) return fail(MMW_ERR_ARG, "mmw_sym_eig: b must be in [1, 2048]");
        if (!(rel_tol > 0.0) || max_sweeps < 1) return fail(MMW_ERR_ARG, "mmw_sym_eig: rel_tol and max_sweeps must be positive");
        MMW_TRY(check_device("mmw_sym_eig", device, DEV_BARE));
        MMW_HIP(hipSetDevice(device));
        ScopedStream stream;
        MMW_HIP(hipStreamCreate(&stream.s));
        const Switches switches = Switches::from_env();
        mmw::DenseWork<double> dw(switches);
        dw.st = stream.s;
        MMW_TRY(dw.ensure(b, 1));
        MMW_TRY(copy_h2d(dw.G.p, G, (size_t)b * b * sizeof(double), stream.s));
        int sw = 0;
        MMW_TRY(dw.jacobi(b, rel_tol, max_sweeps, &sw));
        MMW_TRY(copy_d2h(theta, dw.diag.p, (size_t)b * sizeof(double), stream.s));
        MMW_TRY(copy_d2h(Q, dw.Q.p, (size_t)b * b * sizeof(double), stream.s));
        if (sweeps) *sweeps = sw;
        return MMW_OK;
    });
}
// ---- the factor's dense building blocks, one operation per call (dense_seams.h)
int mmw_dense_gram(int device, int dtype, int32_t K, int32_t b, int32_t ld, const double* V, const double* W, int sym, double* G_out) {
    return guarded("mmw_dense_gram", [&]() -> int {
        if (!V || !W || !G_out) return fail(MMW_ERR_ARG, "mmw_dense_gram: null pointer");
        MMW_TRY(dense_shape("mmw_dense_gram", K, b, ld));
        return dense_call("mmw_dense_gram", device, dtype, [&](hipStream_t st) { return dense_gram_impl<float>(st, K, b, ld, V, W, sym != 0, G_out); },
                          [&](hipStream_t st) { return dense_gram_impl<double>(st, K, b, ld, V, W, sym != 0, G_out); });
    });
}
int mmw_dense_gemm(int device, int dtype, int32_t K, int32_t b, int32_t n, int32_t ld, const double* V, int32_t ldq, const double* Q, double* C_out) {
    return guarded("mmw_dense_gemm", [&]() -> int {
        if (!V || !Q || !C_out) return fail(MMW_ERR_ARG, "mmw_dense_gemm: null pointer");
        MMW_TRY(dense_shape("mmw_dense_gemm", K, b, ld));
        if (n < 1 || ldq < n) return fail(MMW_ERR_ARG, "mmw_dense_gemm: n must be >= 1 and ldq >= n");
        if (n > ld) return fail(MMW_ERR_ARG, "mmw_dense_gemm: n must be <= ld (the product is stored with the block's row stride)");
        return dense_call("mmw_dense_gemm", device, dtype, [&](hipStream_t st) { return dense_gemm_impl<float>(st, K, b, n, ld, V, ldq, Q, C_out); },
                          [&](hipStream_t st) { return dense_gemm_impl<double>(st, K, b, n, ld, V, ldq, Q, C_out); });
    });
}
int mmw_dense_chol(int device, int32_t b, const double* G, double* L_out, double* dscale_out, double* dinv_out, int32_t* ok) {
    return guarded("mmw_dense_chol", [&]() -> int {
        if (!G || !L_out || !dscale_out || !dinv_out || !ok) return fail(MMW_ERR_ARG, "mmw_dense_chol: null pointer");
        if (b < 1 || b > 2048) return fail(MMW_ERR_ARG, "mmw_dense_chol: b must be in [1, 2048]");
        auto run = [&](hipStream_t st) { return dense_chol_impl(st, b, G, L_out, dscale_out, dinv_out, ok); };
        return dense_call("mmw_dense_chol", device, MMW_F64, run, run);
    });
}
int mmw_dense_orth(int device, int dtype, int32_t K, int32_t b, int32_t ld, const double* V, double eps, double* Q_out, int32_t path_out[2]) {
    return guarded("mmw_dense_orth", [&]() -> int {
        if (!V || !Q_out || !path_out) return fail(MMW_ERR_ARG, "mmw_dense_orth: null pointer");
        MMW_TRY(dense_shape("mmw_dense_orth", K, b, ld));
        return dense_call("mmw_dense_orth", device, dtype, [&](hipStream_t st) { return dense_orth_impl<float>(st, K, b, ld, V, eps, Q_out, path_out); },
                          [&](hipStream_t st) { return dense_orth_impl<double>(st, K, b, ld, V, eps, Q_out, path_out); });
    });
}
// ---- problem generator and scorer on the device (include/mmw_hip.h) ----------------------------------------
int mmw_env_create(mmw_env** out, int device, int32_t K, int32_t A, const double* sta_xy, const double* ap_xy, double fre_Hz, double txp_offset,
                   double min_s_n_ratio, double min_sinr, double noise_floor_dbm) {
    return guarded("mmw_env_create", [&]() -> int {
        if (!out || !sta_xy || !ap_xy) return fail(MMW_ERR_ARG, "mmw_env_create: null pointer");
        *out = nullptr;
        if (K < 1 || A < 1) return fail(MMW_ERR_ARG, "mmw_env_create: K and A must be positive");
        if (!(min_sinr > 0.0) || !(txp_offset > 0.0) || !(fre_Hz > 0.0)) return fail(MMW_ERR_ARG, "mmw_env_create: min_sinr, txp_offset and fre_Hz must be positive");
        MMW_TRY(check_device("mmw_env_create", device, DEV_ID_VISIBLE));
        auto h = std::make_unique<mmw_env>();
        const int rc = h->e.init(device, K, A, sta_xy, ap_xy, fre_Hz, txp_offset, min_s_n_ratio, min_sinr, noise_floor_dbm);
        if (rc == MMW_OK) *out = h.release();
        return rc;
    });
}
int mmw_env_destroy(mmw_env* e) { return guarded("mmw_env_destroy", [&]() -> int { delete e; return MMW_OK; }); }
int mmw_env_sizes(mmw_env* e, int64_t out[4]) {
    return guarded("mmw_env_sizes", [&]() -> int {
        if (!e || !out) return fail(MMW_ERR_ARG, "null pointer");
        out[0] = e->e.K; out[1] = e->e.A; out[2] = e->e.nnzS; out[3] = e->e.nnzQ;
        return MMW_OK;
    });
}
int mmw_env_state(mmw_env* e, int32_t* S_indptr, int32_t* S_indices, double* S_data, int32_t* Q_indptr, int32_t* Q_indices, double* Q_data,
                  double* h_max) {
    return entry("mmw_env_state", !e || !S_indptr || !S_indices || !S_data || !Q_indptr || !Q_indices || !Q_data || !h_max, "mmw_env_state: null pointer", [&] { return e->e.state(S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max); });
}
int mmw_env_evaluate(mmw_env* e, const double* z_vec, int32_t Z, double packet_bit, double bandwidth, double slot_time, double* sinr_out,
                     double* bler_out) {
    return entry("mmw_env_evaluate", !e || !z_vec || !sinr_out, "mmw_env_evaluate: null pointer", [&] { return e->e.evaluate(z_vec, Z, packet_bit, bandwidth, slot_time, sinr_out, bler_out); });
}
int mmw_env_move(mmw_env* e, const double* sta_xy) { return entry("mmw_env_move", !e || !sta_xy, "mmw_env_move: null pointer", [&] { return e->e.move(sta_xy); }); }
int mmw_round_env(mmw_solver* s, mmw_env* e, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out, int32_t* rem_out) {
    return entry("mmw_round_env", !s, "null solver handle", [&] { return s->round_env(e, Zr, Dp, gX, nbatch, randv, z_out, rem_out); });
}
// ---- all attempts of one rounding() call drawn, run and chosen among on the device (solver_extras.h, kernels_round_draw.h)
int mmw_round_attempts(mmw_solver* s, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out, int32_t* rem_out,
                       int32_t* pick_out, int32_t* z_all) {
    return entry("mmw_round_attempts", !s, "null solver handle", [&] { return s->round_attempts(nullptr, false, Zr, Dp, gX, nattempt, seed, pick_rule, z_out, rem_out, pick_out, z_all); });
}
int mmw_round_env_attempts(mmw_solver* s, mmw_env* e, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out,
                           int32_t* rem_out, int32_t* pick_out, int32_t* z_all) {
    return entry("mmw_round_env_attempts", !s, "null solver handle", [&] { return s->round_attempts(e, true, Zr, Dp, gX, nattempt, seed, pick_rule, z_out, rem_out, pick_out, z_all); });
}
int mmw_round_randv(mmw_solver* s, int32_t Zr, int32_t Dp, uint64_t seed, int32_t attempt, double* out, int64_t n) {
    return entry("mmw_round_randv", !s, "null solver handle", [&] { return s->round_randv(Zr, Dp, seed, attempt, out, n); });
}
int mmw_gm_create(mmw_gm** out, int device, int32_t K, const int32_t* S_indptr, const int32_t* S_indices, const double* S_data,
                  const int32_t* Q_indptr, const int32_t* Q_indices, const double* Q_data, const double* h_max) {
    return guarded("mmw_gm_create", [&]() -> int {
        if (!out || !S_indptr || !S_indices || !S_data || !Q_indptr || !Q_indices || !Q_data || !h_max) return fail(MMW_ERR_ARG, "mmw_gm_create: null pointer");
        *out = nullptr;
        if (K < 1) return fail(MMW_ERR_ARG, "mmw_gm_create: K must be >= 1");
        if (device != -1) MMW_TRY(check_device("mmw_gm_create", device, DEV_ID_VISIBLE));
        auto g = std::make_unique<mmw_gm>();
        const std::string err = g->S.build(K, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max);
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_gm_create: " + err);
        MMW_TRY(g->init(device));
        *out = g.release();
        return MMW_OK;
    });
}
int mmw_gm_create_from_env(mmw_gm** out, mmw_env* e) {
    return guarded("mmw_gm_create_from_env", [&]() -> int {
        if (!out || !e) return fail(MMW_ERR_ARG, "mmw_gm_create_from_env: null pointer");
        *out = nullptr;
        auto g = std::make_unique<mmw_gm>();
        MMW_TRY(g->init_from_env(e->e.list_source()));
        *out = g.release();
        return MMW_OK;
    });
}
int mmw_gm_key(mmw_gm* g, int kind, double* key_out) { return entry("mmw_gm_key", !g || !key_out, "mmw_gm_key: null pointer", [&] { return g->get_key(kind, key_out); }); }
int mmw_gm_destroy(mmw_gm* g) { return guarded("mmw_gm_destroy", [&]() -> int { delete g; return MMW_OK; }); }
int mmw_gm_sizes(mmw_gm* g, int64_t out[4]) {
    return guarded("mmw_gm_sizes", [&]() -> int {
        if (!g || !out) return fail(MMW_ERR_ARG, "null pointer");
        out[0] = g->S.K; out[1] = g->S.clique ? g->S.G : -1; out[2] = g->nnz_so(); out[3] = g->nnz_q();
        return MMW_OK;
    });
}
int mmw_gm_pass(mmw_gm* g, const int32_t* order, int32_t n, int32_t nattempt, int32_t* list_out, int32_t* nlist) {
    return entry("mmw_gm_pass", !g || (!order && n) || (!list_out && n) || !nlist, "mmw_gm_pass: null pointer", [&] { return g->pass(order, n, nattempt, list_out, nlist); });
}
int mmw_gm_run(mmw_gm* g, const double* key, int32_t Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out, int32_t* rem_out) {
    return entry("mmw_gm_run", !g || !key || !z_out || !zz_out || !rem_out, "mmw_gm_run: null pointer", [&] { return g->run(key, Z, nattempt, z_out, zz_out, rem_out); });
}
int mmw_gm_assign(mmw_gm* g, int32_t Z, const int32_t* order, const int32_t* pref, int32_t* z_out, int32_t* rem_out) {
    return entry("mmw_gm_assign", !g || !order || !pref || !z_out || !rem_out, "mmw_gm_assign: null pointer", [&] { return g->assign(Z, order, pref, z_out, rem_out); });
}
int mmw_gm_rand(mmw_gm* g, int32_t Z, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out, int32_t* rem_out, int32_t* pick_out) {
    return entry("mmw_gm_rand", !g, "mmw_gm_rand: null pointer", [&] { return g->rand(Z, nattempt, seed, pick_rule, z_out, rem_out, pick_out); });
}
int mmw_gm_rand_draw(mmw_gm* g, int32_t Z, uint64_t seed, int32_t attempt, double* pref_val_out, double* order_key_out) {
    return entry("mmw_gm_rand_draw", !g, "mmw_gm_rand_draw: null pointer", [&] { return g->rand_draw(Z, seed, attempt, pref_val_out, order_key_out); });
}
// ---- the batched solver (batch_handle.h): its entries report an exception under the handle's name, "mmw_batch"
int mmw_batch_create(mmw_batch** out, int device, int32_t B, const int32_t* K, const int32_t* Z, int32_t rank_radio, double eta,
                     const int32_t* nit, const int32_t* const* S_indptr, const int32_t* const* S_indices, const double* const* S_data,
                     const int32_t* const* Q_indptr, const int32_t* const* Q_indices, const double* const* Q_data, const double* const* h_max) {
    return guarded("mmw_batch", [&]() -> int {
        if (!out || !K || !Z || !nit || !S_indptr || !S_indices || !S_data || !Q_indptr || !Q_indices || !Q_data || !h_max)
            return fail(MMW_ERR_ARG, "mmw_batch_create: null pointer");
        *out = nullptr;
        if (B < 1) return fail(MMW_ERR_ARG, "mmw_batch_create: B must be >= 1");
        if (B > 65535) return fail(MMW_ERR_ARG, "mmw_batch_create: at most 65535 instances per batch");
        if (rank_radio < 1) return fail(MMW_ERR_ARG, "rank_radio must be >= 1");
        if (!(eta >= 0.0)) return fail(MMW_ERR_ARG, "eta must be non-negative");
        auto bt = std::make_unique<mmw_batch>();
        MMW_TRY(bt->init(device, B, K, Z, rank_radio, eta, nit, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max));
        *out = bt.release();
        return MMW_OK;
    });
}
int mmw_batch_destroy(mmw_batch* b) { return guarded("mmw_batch", [&]() -> int { delete b; return MMW_OK; }); }
int mmw_batch_sizes(mmw_batch* b, int32_t inst, int64_t out[10]) { return entry("mmw_batch", !b || !out, "null pointer", [&] { return b->sizes(inst, out); }); }
int mmw_batch_set_slots(mmw_batch* b, const int32_t* Z, int32_t nit) { return entry("mmw_batch", !b || !Z, "null pointer", [&] { return b->set_slots(Z, nit, false); }); }
int mmw_batch_set_slots_warm(mmw_batch* b, const int32_t* Z, int32_t nit) { return entry("mmw_batch", !b || !Z, "null pointer", [&] { return b->set_slots(Z, nit, true); }); }
int mmw_batch_carry(mmw_batch* dst, mmw_batch* src, const int32_t* take) { return entry("mmw_batch", !dst || !src, "null batch handle", [&] { return batch_carry(dst, src, take); }); }
int mmw_batch_carry_map(mmw_batch* dst, mmw_batch* src, int32_t inst, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc) {
    return entry("mmw_batch", !dst || !src || (!lmap && nl) || (!cmap && nc), "null pointer", [&] { return batch_carry_map(dst, src, inst, lmap, nl, cmap, nc); });
}
int mmw_batch_reset(mmw_batch* b, int32_t nit) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->reset(nit); }); }
int mmw_batch_set_eta(mmw_batch* b, const double* eta) { return entry("mmw_batch", !b || !eta, "null pointer", [&] { return b->set_eta(eta); }); }
int mmw_batch_set_expm(mmw_batch* b, int max_order, double tol) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->set_expm(max_order, tol); }); }
int mmw_batch_set_gap(mmw_batch* b, int enabled, int32_t m_cap) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->set_gap(enabled, m_cap); }); }
int mmw_batch_read_gap(mmw_batch* b, int32_t inst, double* out, int64_t n) { return entry("mmw_batch", !b || (!out && n), "null pointer", [&] { return b->read_gap(inst, out, n); }); }
int mmw_batch_set_split(mmw_batch* b, const int32_t* parts) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->set_split(parts); }); }
int mmw_batch_set_row_split(mmw_batch* b, const int32_t* rows) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->set_row_split(rows); }); }
int mmw_batch_row_ranges(mmw_batch* b, int32_t inst, int32_t rows, int32_t* out) { return entry("mmw_batch", !b || !out, "null pointer", [&] { return b->row_ranges(inst, rows, out); }); }
int mmw_batch_set_head_split(mmw_batch* b, const int32_t* parts) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->set_head_split(parts); }); }
int mmw_batch_head_ranges(mmw_batch* b, int32_t inst, int32_t parts, int32_t* out) { return entry("mmw_batch", !b || !out, "null pointer", [&] { return b->head_ranges(inst, parts, out); }); }
int mmw_batch_set_factor_split(mmw_batch* b, const int32_t* parts) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->set_factor_split(parts); }); }
int mmw_batch_iterate(mmw_batch* b, int32_t n, const double* randv, const uint64_t* seeds) { return entry("mmw_batch", !b, "null batch handle", [&] { return b->iterate(n, randv, seeds); }); }
int mmw_batch_read_f64(mmw_batch* b, int32_t inst, int which, double* out, int64_t n) { return entry("mmw_batch", !b || (!out && n), "null pointer", [&] { return b->read_f64(inst, which, out, n); }); }
int mmw_batch_read_i32(mmw_batch* b, int32_t inst, int which, int32_t* out, int64_t n) { return entry("mmw_batch", !b || (!out && n), "null pointer", [&] { return b->read_i32(inst, which, out, n); }); }
int mmw_batch_sketch(mmw_batch* b, int32_t inst, uint64_t seed, int32_t iteration, double* out, int64_t n) { return entry("mmw_batch", !b || !out, "null pointer", [&] { return b->sketch(inst, seed, iteration, out, n); }); }
int mmw_batch_export(mmw_batch* b, int32_t inst, mmw_solver* h) {
    return guarded("mmw_batch", [&]() -> int {
        if (!b || !h) return fail(MMW_ERR_ARG, "null pointer");
        MMW_TRY(b->core.check_inst(inst));
        auto* s = dynamic_cast<Solver<double>*>(h);
        if (!s) return fail(MMW_ERR_ARG, "mmw_batch_export: the handle is not an fp64 handle");
        return batch_export_into(b, inst, s);
    });
}
int mmw_batch_factor(mmw_batch* b, const int32_t* take, const int32_t* rank, const double* const* xavg) {
    return entry("mmw_batch", !b, "null batch handle", [&] { return b->factor(take, rank, xavg); });
}
int mmw_batch_round(mmw_batch* b, const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out,
                    int32_t* rem_out, int32_t* used_out) {
    return entry("mmw_batch", !b || !seeds || !z_out || !rem_out || !used_out, "null pointer",
                 [&] { return b->round(take, nattempt, stop_at_first, seeds, z_out, rem_out, used_out); });
}
int mmw_batch_round_randv(mmw_batch* b, int32_t inst, uint64_t seed, int32_t attempt, double* out, int64_t n) {
    return entry("mmw_batch", !b || !out, "null pointer", [&] { return b->round_randv(inst, seed, attempt, out, n); });
}
int mmw_batch_factor_random(mmw_batch* b, const int32_t* take, const uint64_t* seeds) {
    return entry("mmw_batch", !b || !seeds, "null pointer", [&] { return b->factor_random(take, seeds); });
}
int mmw_batch_factor_spectral(mmw_batch* b, const int32_t* take, const int32_t* Z) {
    return entry("mmw_batch", !b, "null batch handle", [&] { return b->factor_spectral(take, Z); });
}
int mmw_batch_gm(mmw_batch* b, int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out,
                 int32_t* rem_out, double* key_out) {
    return entry("mmw_batch", !b || !Z || !z_out || !zz_out || !rem_out, "null pointer",
                 [&] { return b->gm(kind, take, Z, nattempt, z_out, zz_out, rem_out, key_out); });
}
int mmw_batch_gm_rand(mmw_batch* b, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds,
                      int32_t* z_out, int32_t* rem_out, int32_t* used_out) {
    return entry("mmw_batch", !b, "mmw_batch_gm_rand: null pointer", [&] { return b->gm_rand(take, Z, nattempt, stop_at_first, seeds, z_out, rem_out, used_out); });
}
// ---- the batched generator and scorer (batch_env_handle.h): the online sweeps' state per time point
int mmw_batch_env_create(mmw_batch_env** out, int device, int32_t B, const int32_t* K, const int32_t* A, const double* const* ap_xy, double fre_Hz,
                         double txp_offset, double min_s_n_ratio, double min_sinr, double noise_floor_dbm) {
    return guarded("mmw_batch_env", [&]() -> int {
        if (!out || !K || !A || !ap_xy) return fail(MMW_ERR_ARG, "mmw_batch_env_create: null pointer");
        *out = nullptr;
        if (B < 1 || B > 65535) return fail(MMW_ERR_ARG, "mmw_batch_env_create: B must be in [1, 65535]");
        if (!(min_sinr > 0.0) || !(txp_offset > 0.0) || !(fre_Hz > 0.0)) return fail(MMW_ERR_ARG, "mmw_batch_env_create: min_sinr, txp_offset and fre_Hz must be positive");
        for (int b = 0; b < B; ++b) {
            const std::string who = "mmw_batch_env_create: instance " + std::to_string(b);
            if (!ap_xy[b]) return fail(MMW_ERR_ARG, who + ": null pointer");
            if (K[b] < 1 || A[b] < 1) return fail(MMW_ERR_ARG, who + ": K and A must be positive");
            if (K[b] > EPI_MAX_K) return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(K[b]) + " exceeds the limit " + std::to_string(EPI_MAX_K) + " (run it on mmw_env_create)");
            if (A[b] > BENV_MAX_A) return fail(MMW_ERR_ARG, who + ": A = " + std::to_string(A[b]) + " exceeds the limit " + std::to_string(BENV_MAX_A) + " (run it on mmw_env_create)");
        }
        if (device == -1) return fail(MMW_ERR_ARG, "mmw_batch_env_create: device -1 (host only) is not served: the generator and the scorer run on the device");
        MMW_TRY(check_device("mmw_batch_env_create", device, DEV_ID));
        auto h = std::make_unique<mmw_batch_env>();
        MMW_TRY(h->init(device, B, K, A, ap_xy, fre_Hz, txp_offset, min_s_n_ratio, min_sinr, noise_floor_dbm));
        *out = h.release();
        return MMW_OK;
    });
}
int mmw_batch_env_destroy(mmw_batch_env* e) { return guarded("mmw_batch_env", [&]() -> int { delete e; return MMW_OK; }); }
int mmw_batch_env_move(mmw_batch_env* e, const double* const* sta_xy) {
    return guarded("mmw_batch_env", [&]() -> int {
        if (!e || !sta_xy) return fail(MMW_ERR_ARG, "mmw_batch_env_move: null pointer");
        for (int b = 0; b < e->B; ++b)
            if (!sta_xy[b]) return fail(MMW_ERR_ARG, "mmw_batch_env_move: instance " + std::to_string(b) + ": null pointer");
        return e->move(sta_xy);
    });
}
int mmw_batch_env_sizes(mmw_batch_env* e, int32_t inst, int64_t out[4]) { return entry("mmw_batch_env", !e || !out, "null pointer", [&] { return e->sizes(inst, out); }); }
int mmw_batch_env_state(mmw_batch_env* e, int32_t inst, int32_t* S_indptr, int32_t* S_indices, double* S_data, int32_t* Q_indptr, int32_t* Q_indices,
                        double* Q_data, double* h_max) {
    return entry("mmw_batch_env", !e || !S_indptr || !S_indices || !S_data || !Q_indptr || !Q_indices || !Q_data || !h_max, "mmw_batch_env_state: null pointer",
                 [&] { return e->state(inst, S_indptr, S_indices, S_data, Q_indptr, Q_indices, Q_data, h_max); });
}
int mmw_batch_env_evaluate(mmw_batch_env* e, const double* const* z_vec, const int32_t* Z, double packet_bit, double bandwidth, double slot_time,
                           double* const* sinr_out, double* const* bler_out) {
    return entry("mmw_batch_env", !e || !z_vec || !Z || !sinr_out, "mmw_batch_env_evaluate: null pointer",
                 [&] { return e->evaluate(z_vec, Z, packet_bit, bandwidth, slot_time, sinr_out, bler_out); });
}
int mmw_batch_create_from_env(mmw_batch** out, mmw_batch_env* env, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit) {
    return guarded("mmw_batch", [&]() -> int {
        if (!out || !env || !Z || !nit) return fail(MMW_ERR_ARG, "mmw_batch_create_from_env: null pointer");
        if (rank_radio < 1) return fail(MMW_ERR_ARG, "rank_radio must be >= 1");
        if (!(eta >= 0.0)) return fail(MMW_ERR_ARG, "eta must be non-negative");
        auto bt = std::make_unique<mmw_batch>();
        MMW_TRY(batch_init_from_env(*bt, *env, Z, rank_radio, eta, nit));
        *out = bt.release();
        return MMW_OK;
    });
}
int mmw_batch_create_from_csr(mmw_batch** out, int32_t B, mmw_csr* const* csr, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit) {
    return guarded("mmw_batch", [&]() -> int {
        if (!out || !csr || !Z || !nit) return fail(MMW_ERR_ARG, "mmw_batch_create_from_csr: null pointer");
        if (B < 1) return fail(MMW_ERR_ARG, "mmw_batch_create_from_csr: B must be >= 1");
        if (B > 65535) return fail(MMW_ERR_ARG, "mmw_batch_create_from_csr: at most 65535 instances per batch");
        if (rank_radio < 1) return fail(MMW_ERR_ARG, "rank_radio must be >= 1");
        if (!(eta >= 0.0)) return fail(MMW_ERR_ARG, "eta must be non-negative");
        auto bt = std::make_unique<mmw_batch>();
        MMW_TRY(batch_init_from_csr(*bt, B, csr, Z, rank_radio, eta, nit));
        *out = bt.release();
        return MMW_OK;
    });
}
int mmw_batch_env_gm(mmw_batch_env* e, int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out,
                     int32_t* rem_out, double* key_out) {
    return entry("mmw_batch_env", !e || !Z || !z_out || !zz_out || !rem_out, "null pointer",
                 [&] { return e->gm(kind, take, Z, nattempt, z_out, zz_out, rem_out, key_out); });
}
int mmw_batch_env_gm_rand(mmw_batch_env* e, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds,
                          int32_t* z_out, int32_t* rem_out, int32_t* used_out) {
    return entry("mmw_batch_env", !e, "mmw_batch_env_gm_rand: null pointer", [&] { return e->gm_rand(take, Z, nattempt, stop_at_first, seeds, z_out, rem_out, used_out); });
}
int mmw_batch_round_env(mmw_batch* b, mmw_batch_env* e, const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds,
                        int32_t* z_out, int32_t* rem_out, int32_t* used_out) {
    return entry("mmw_batch", !b || !e || !seeds || !z_out || !rem_out || !used_out, "null pointer",
                 [&] { return batch_round_env(b, e, take, nattempt, stop_at_first, seeds, z_out, rem_out, used_out); });
}
}  // extern "C"
