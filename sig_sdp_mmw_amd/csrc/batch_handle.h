// Batched solver (mmw_batch_*): many small fp64 instances, one workgroup each (csrc/kernels_batch.h).  The handle holds a core
// (batch_core.h: patterns, counters, the two arenas) and four parts by value, each with the state and the device buffers of one feature:
// gap and split (batch_iterate.h), head (batch_head.h), rows (batch_rows.h), epi (batch_epilogue.h), greedy (batch_gm.h), and sequences them.  Whatever a part holds that a new
// run invalidates, it drops in its on_restart: reset and set_slots call those and name no field of a part.  Two entries work on a
// pair of batches and stand below the handle: batch_export_into (an fp64 handle) and batch_carry (another batch, on moved states).
#pragma once
#include "batch_epilogue.h"
#include "batch_gm.h"
#include "batch_iterate.h"
#include "batch_rows.h"

struct mmw_batch {
    BatchCore core;
    BatchGap gap;
    BatchSplit split;
    BatchRows rows;
    BatchHead head;
    BatchEpilogue epi;
    BatchGm greedy;
    DevBuf<double> rbuf, skbuf;  // the call's sketches (iterate), the block handed out (sketch)
    ~mmw_batch() {
        if (core.host_only || !core.st) return;
        (void)hipSetDevice(core.device);
        (void)hipStreamDestroy(core.st);
    }
    // mmw_batch_create after its null and range checks
    int init(int device, int32_t B, const int32_t* K, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit,
             const int32_t* const* S_indptr, const int32_t* const* S_indices, const double* const* S_data, const int32_t* const* Q_indptr,
             const int32_t* const* Q_indices, const double* const* Q_data, const double* const* h_max) {
        core.device = device; core.host_only = device == -1; core.B = B; core.rank_radio = rank_radio;
        core.eta.assign(B, eta); core.nit.assign(nit, nit + B); core.iter.assign(B, 0); core.active.assign(B, 1);
        core.H.resize(B);
        greedy.gmx.resize(B);
        for (int b = 0; b < B; ++b) {
            const std::string who = "mmw_batch_create: instance " + std::to_string(b);
            if (nit[b] < 1) return fail(MMW_ERR_ARG, who + ": nit must be >= 1");
            if (!S_indptr[b] || !S_indices[b] || !S_data[b] || !Q_indptr[b] || !Q_indices[b] || !Q_data[b] || !h_max[b]) return fail(MMW_ERR_ARG, who + ": null pointer");
            if (K[b] > BATCH_MAX_K)
                return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(K[b]) + " exceeds the batch limit " + std::to_string(BATCH_MAX_K) + " (run it on a handle)");
            const std::string err = build_pattern(core.H[b], K[b], Z[b], S_indptr[b], S_indices[b], S_data[b], Q_indptr[b], Q_indices[b], Q_data[b], h_max[b]);
            if (!err.empty()) return fail(MMW_ERR_ARG, who + ": " + err);
            greedy.extra(b, K[b], Q_indptr[b], Q_indices[b], Q_data[b]);
        }
        if (!core.host_only) {
            MMW_TRY(check_device("mmw_batch_create", device, DEV_ID));
            MMW_HIP(hipSetDevice(device));
            MMW_HIP(hipStreamCreateWithFlags(&core.st, hipStreamNonBlocking));
        }
        MMW_TRY(core.layout());
        if (!core.host_only)
            for (int b = 0; b < B; ++b) MMW_TRY(core.reset_one(b));
        return MMW_OK;
    }
    int sizes(int b, int64_t out[10]) const {
        MMW_TRY(core.check_inst(b));
        const HostPattern& P = core.pat(b);
        const BatchDesc& d = core.desc[b];
        const int64_t v[10] = {P.K, P.Z, d.D, d.D, P.nnzL(), P.nnzST(), P.E_gain(), P.E_asso(), P.C(), core.iter[b]};
        for (int i = 0; i < 10; ++i) out[i] = v[i];
        return MMW_OK;
    }
    int set_eta(const double* eta) {
        for (int i = 0; i < core.B; ++i)
            if (!(eta[i] >= 0.0)) return fail(MMW_ERR_ARG, "eta must be non-negative");
        core.eta.assign(eta, eta + core.B);
        return MMW_OK;
    }
    int set_expm(int max_order, double tol) {
        if (max_order < 1 || max_order > MAX_ORDER) return fail(MMW_ERR_ARG, "max_order must be in [1, 16]");
        if (!(tol > 0.0)) return fail(MMW_ERR_ARG, "tol must be positive");
        core.max_order = max_order; core.tol = tol;
        return MMW_OK;
    }
    int on_restart() {  // every part drops what a new run invalidates
        MMW_TRY(gap.on_restart(core));
        epi.on_restart();
        return MMW_OK;
    }
    // the reference's initial point (mmw.py:62-73): Y = 1/C, X = I, L = 0, sums zero
    int reset(int32_t nit_) {
        if (core.host_only) return BatchCore::host_only_batch();
        if (nit_ < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        MMW_HIP(hipSetDevice(core.device));
        for (int b = 0; b < core.B; ++b) {
            core.nit[b] = nit_;
            if (!core.on_device) MMW_TRY(core.reset_one(b));
        }
        if (core.on_device) MMW_TRY(core.init_point());
        return on_restart();
    }
    // Same states, new slot counts: the Z-dependent scalars on the host (update_slots), the arena on the device (BatchCore::relayout).
    // Cold, every instance restarts at the initial point.  Warm (mmw_batch_set_slots_warm), an instance that has iterated keeps
    // (e_accu, L, X, Y) and restarts its sums; one that has not falls back to cold, as Solver::set_slots does; one with Z[b] <= 0 sits
    // out with its iterate and its counters carried over, so a later warm call can pick it up.
    int set_slots(const int32_t* Z, int32_t nit_, bool warm) {
        if (core.host_only) return BatchCore::host_only_batch();
        if (nit_ < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        const std::string who = warm ? "mmw_batch_set_slots_warm" : "mmw_batch_set_slots";
        std::vector<HostPattern>& H = core.H;
        std::vector<HostPattern> keep = H;  // a refused slot count leaves the batch as it was
        for (int b = 0; b < core.B; ++b) {
            if (Z[b] <= 0) continue;
            const std::string err = update_slots(H[b], Z[b]);
            if (!err.empty()) { H = std::move(keep); return fail(MMW_ERR_ARG, who + ": instance " + std::to_string(b) + ": " + err); }
            const std::string lerr = BatchCore::check_limits(H[b], Z[b] * core.rank_radio);
            if (!lerr.empty()) { H = std::move(keep); return fail(MMW_ERR_ARG, who + ": instance " + std::to_string(b) + ": " + lerr + " (run it on a handle)"); }
        }
        std::vector<int> mode((size_t)core.B);
        for (int b = 0; b < core.B; ++b) mode[b] = !warm ? RELAYOUT_COLD : Z[b] <= 0 ? RELAYOUT_OUT : core.iter[b] == 0 ? RELAYOUT_COLD : RELAYOUT_WARM;
        const int rc = core.relayout(mode);
        if (rc != MMW_OK) { H = std::move(keep); return rc; }
        for (int b = 0; b < core.B; ++b) {
            core.active[b] = Z[b] > 0;
            if (mode[b] == RELAYOUT_OUT) continue;
            core.nit[b] = nit_;
            core.iter[b] = 0;
        }
        return on_restart();
    }
    int iterate(int32_t n, const double* randv, const uint64_t* seeds) {
        if (core.host_only) return BatchCore::host_only_batch();
        if (n < 1) return fail(MMW_ERR_ARG, "mmw_batch_iterate: n must be >= 1");
        if (!randv && !seeds) return fail(MMW_ERR_ARG, "mmw_batch_iterate: give either the sketches or one seed per instance");
        MMW_HIP(hipSetDevice(core.device));
        const int B = core.B;
        hipStream_t st = core.st;
        std::vector<BatchDesc> dd = core.desc;
        int64_t off = 0;
        int runs = 0;
        for (int b = 0; b < B; ++b) {
            BatchDesc& d = dd[b];
            d.nrun = core.active[b] ? std::min(n, core.nit[b] - core.iter[b]) : 0;
            d.iter0 = core.iter[b];
            d.eta = core.eta[b]; d.tol = core.tol; d.max_order = core.max_order;
            d.seed = seeds ? seeds[b] : 0;
            if (randv && d.nrun > 0) { d.o_randv = off; off += (int64_t)d.nrun * d.K * d.D; }
            runs += d.nrun > 0;
        }
        if (!runs) return fail(MMW_ERR_STATE, "mmw_batch_iterate: every instance has run its announced iterations");
        if (randv) MMW_TRY(rbuf.alloc((size_t)off));
        if (randv) MMW_TRY(copy_h2d(rbuf.p, randv, (size_t)off * sizeof(double), st));
        MMW_TRY(copy_h2d(core.d_desc.p, dd.data(), dd.size() * sizeof(BatchDesc), st));
        const double* rv = randv ? rbuf.p : (const double*)nullptr;
        MMW_TRY(gap.stage(core));
        int nmax = 0;
        for (int b = 0; b < B; ++b) nmax = std::max(nmax, dd[b].nrun);
        // the head split rides on the split paths: alone it is the column split's path with one slice per instance
        BatchHead* hd = head.wanted(dd) ? &head : nullptr;
        if (hd) MMW_TRY(head.stage(core, dd));
        else head.off();
        if (rows.wanted(dd)) {
            MMW_TRY(rows.run(core, gap, split.parts, dd, rv, hd));
        } else if (hd) {
            MMW_TRY(split.run(core, gap, dd, rv, hd));
            rows.record(1, (int64_t)nmax + head.launches, 0, std::max<int64_t>(std::max<int64_t>(split.d_wexpm.n, head.widest), std::max<int64_t>(split.d_wx.n, B)));
        } else if (split.wanted(dd)) {
            MMW_TRY(split.run(core, gap, dd, rv));
            rows.record(1, 3 * (int64_t)nmax, 0, std::max<int64_t>(split.d_wexpm.n, std::max<int64_t>(split.d_wx.n, B)));
        } else {
            if (gap.on)
                hipLaunchKernelGGL(k_mmw_batch<true>, dim3(B), dim3(BATCH_THREADS), 0, st, core.d_desc.p, core.ia.p, core.fa.p, rv, gap.d_gdesc.p, gap.ga.p);
            else
                hipLaunchKernelGGL(k_mmw_batch<false>, dim3(B), dim3(BATCH_THREADS), 0, st, core.d_desc.p, core.ia.p, core.fa.p, rv, (const GapDesc*)nullptr, (double*)nullptr);
            rows.record(0, 1, 0, B);
        }
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        if (hd) head.done();
        for (int b = 0; b < B; ++b) core.iter[b] += dd[b].nrun;
        return MMW_OK;
    }
    int read_dev(int64_t o, int64_t len, double* out, int64_t n) {
        if (n != len) return fail(MMW_ERR_ARG, "mmw_batch_read_f64: wrong length " + std::to_string(n) + ", expected " + std::to_string(len));
        MMW_HIP(hipSetDevice(core.device));
        return copy_d2h(out, core.fa.p + o, (size_t)len * sizeof(double), core.st);
    }
    static int read_host(const std::vector<double>& v, double* out, int64_t n) { return export_vec(v, out, n, "mmw_batch_read_f64"); }
    int read_f64(int b, int which, double* out, int64_t n) {
        MMW_TRY(core.check_inst(b));
        const HostPattern& P = core.pat(b);
        switch (which) {
            case MMW_F_S_SUM: return read_host(P.S_sum, out, n);
            case MMW_F_NORM_H: return read_host(P.norm_H, out, n);
            case MMW_F_ST_DATA: return read_host(core.full(b).st_data, out, n);
            case MMW_F_BUILD_INFO: return read_host({core.on_device ? 1.0 : 0.0, core.on_device && core.lazy[b] ? 0.0 : 1.0}, out, n);
            case MMW_F_FACTOR_CALL: return read_host(std::vector<double>(epi.fs.call, epi.fs.call + 4), out, n);
            case MMW_F_SPLIT_CALL: return read_host(std::vector<double>(rows.call, rows.call + 4), out, n);
            case MMW_F_HEAD_CALL: return read_host(std::vector<double>(head.call, head.call + 4), out, n);
            default: break;
        }
        if (core.host_only) return BatchCore::host_only_batch();
        const BatchDesc& d = core.desc[b];
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
                if (core.iter[b] == 0) return fail(MMW_ERR_STATE, "mmw_batch_read_f64: no iteration has run on this instance");
                return read_dev(d.o_R, KD, out, n);
            case MMW_F_EXPM_INFO: return read_dev(d.o_info, 4, out, n);
            case MMW_F_PATTERN: return read_dev(d.o_sab, 2 * (int64_t)d.nnzL + 4 * (int64_t)d.K, out, n);
            case MMW_F_FACTOR:
            case MMW_F_FACTOR_ROWNORM:
            case MMW_F_FACTOR_INFO: return epi.read(core, b, which, out, n);
            default: return fail(MMW_ERR_ARG, "mmw_batch_read_f64: field not held by a batch");
        }
    }
    int read_i32(int b, int which, int32_t* out, int64_t n) {
        MMW_TRY(core.check_inst(b));
        if (which == MMW_I_PATTERN) {
            if (core.host_only) return BatchCore::host_only_batch();
            const BatchDesc& d = core.desc[b];
            const int64_t len = d.o_apos + d.E_asso - d.o_indptr;
            if (n != len) return fail(MMW_ERR_ARG, "mmw_batch_read_i32: wrong length " + std::to_string(n) + ", expected " + std::to_string(len));
            MMW_HIP(hipSetDevice(core.device));
            return copy_d2h(out, core.ia.p + d.o_indptr, (size_t)len * sizeof(int32_t), core.st);
        }
        if (!host_list_i32(core.pat(b), which)) return fail(MMW_ERR_ARG, "mmw_batch_read_i32: unknown field");  // before a pattern is completed for it
        const std::vector<int32_t>* v = host_list_i32(which == MMW_I_L_INDPTR ? core.pat(b) : core.full(b), which);
        return v ? export_vec(*v, out, n, "mmw_batch_read_i32") : fail(MMW_ERR_ARG, "mmw_batch_read_i32: unknown field");
    }
    int sketch(int b, uint64_t seed, int32_t iteration, double* out, int64_t n) {
        MMW_TRY(core.check_inst(b));
        if (core.host_only) return BatchCore::host_only_batch();
        if (iteration < 0) return fail(MMW_ERR_ARG, "mmw_batch_sketch: iteration must be >= 0");
        const BatchDesc& d = core.desc[b];
        const int64_t KD = (int64_t)d.K * d.D;
        if (n != KD) return fail(MMW_ERR_ARG, "mmw_batch_sketch: wrong length for a K x D block");
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(skbuf.alloc((size_t)KD));
        hipLaunchKernelGGL(k_batch_sketch, dim3(1), dim3(BATCH_THREADS), 0, core.st, d.K, d.D, seed, (uint32_t)iteration, skbuf.p);
        MMW_HIP(hipGetLastError());
        return copy_d2h(out, skbuf.p, (size_t)KD * sizeof(double), core.st);
    }
    // ---- the parts' entries
    int set_gap(int enabled, int32_t m_cap) { return gap.set(core, enabled, m_cap); }
    int read_gap(int b, double* out, int64_t n) { return gap.read(core, b, out, n); }
    int set_split(const int32_t* p) { return split.set(core, p); }
    int set_row_split(const int32_t* p) { return rows.set(core, p); }
    int row_ranges(int b, int32_t nrows, int32_t* out) const {
        MMW_TRY(core.check_inst(b));
        if (nrows < 1 || nrows > MMW_BATCH_MAX_ROW_PARTS)
            return fail(MMW_ERR_ARG, "mmw_batch_row_ranges: rows = " + std::to_string(nrows) + " is outside [1, " + std::to_string(MMW_BATCH_MAX_ROW_PARTS) + "]");
        batch_row_bounds(core.pat(b).l_indptr.data(), core.pat(b).K, nrows, out);
        return MMW_OK;
    }
    int set_head_split(const int32_t* p) { return head.set(core, p); }
    int head_ranges(int b, int32_t nparts, int32_t* out) const {
        MMW_TRY(core.check_inst(b));
        if (nparts < 1 || nparts > MMW_BATCH_MAX_HEAD_PARTS)
            return fail(MMW_ERR_ARG, "mmw_batch_head_ranges: parts = " + std::to_string(nparts) + " is outside [1, " + std::to_string(MMW_BATCH_MAX_HEAD_PARTS) + "]");
        batch_row_bounds(core.pat(b).l_indptr.data(), core.pat(b).K, nparts, out);
        return MMW_OK;
    }
    int set_factor_split(const int32_t* p) { return epi.set_split(core, p); }
    int factor(const int32_t* take, const int32_t* rank, const double* const* xavg) { return epi.factor(core, take, rank, xavg); }
    int factor_random(const int32_t* take, const uint64_t* seeds) { return epi.factor_random(core, take, seeds); }
    int factor_spectral(const int32_t* take, const int32_t* Z) { return epi.factor_spectral(core, take, Z); }
    int round(const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out, int32_t* rem_out, int32_t* used_out,
              const BatchEpilogue::RoundSource* src = nullptr) {
        return epi.round(core, take, nattempt, stop_at_first, seeds, z_out, rem_out, used_out, src);
    }
    int round_randv(int b, uint64_t seed, int32_t attempt, double* out, int64_t n) { return epi.round_randv(core, b, seed, attempt, out, n); }
    int gm(int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out, int32_t* rem_out, double* key_out) {
        return greedy.run(core, epi, kind, take, Z, nattempt, z_out, zz_out, rem_out, key_out);
    }
    int gm_rand(const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out, int32_t* rem_out,
                int32_t* used_out) {
        return greedy.rand(core, epi, take, Z, nattempt, stop_at_first, seeds, z_out, rem_out, used_out);
    }
};
// mmw_batch_export: the instance's iterate into an fp64 handle of the same (state, Z), as if the handle had run those iterations.
inline int batch_export_into(mmw_batch* bt, int b, Solver<double>* s) {
    const BatchDesc& d = bt->core.desc[b];
    if (s->core.host_only || bt->core.host_only) return fail(MMW_ERR_STATE, "mmw_batch_export: host-only batch or handle");
    if (s->core.device != bt->core.device) return fail(MMW_ERR_ARG, "mmw_batch_export: the handle lives on another device");
    if (s->core.K != d.K || s->core.Z != d.Z || s->core.D != d.D || s->core.H.nnzL() != (int64_t)d.nnzL || s->core.H.C() != (int64_t)d.C)
        return fail(MMW_ERR_ARG, "mmw_batch_export: the handle's K / Z / nnzL do not match the instance's");
    const HostPattern& P = bt->core.full(b);
    if (s->core.H.l_indices != P.l_indices || s->core.H.l_indptr != P.l_indptr) return fail(MMW_ERR_ARG, "mmw_batch_export: the handle's pattern is not the instance's");
    MMW_HIP(hipSetDevice(s->core.device));
    MMW_TRY(s->settle());
    MMW_HIP(hipStreamSynchronize(bt->core.st));
    MMW_HIP(hipStreamSynchronize(s->core.st));
    // the state a reset leaves (plans, lagged history, chains, timers), then the iterate on top
    MMW_TRY(s->reset(std::max(1, bt->core.nit[b])));
    const size_t nnz = (size_t)d.nnzL, C = (size_t)d.C;
    const double* f = bt->core.fa.p;
    const struct { double* dst; int64_t off; size_t n; } parts[7] = {{s->core.lval.p, d.o_lval, nnz}, {s->core.xval.p, d.o_xval, nnz}, {s->core.xavg.p, d.o_xavg, nnz}, {s->core.Y.p, d.o_Y, C},
                                                                     {s->core.yavg.p, d.o_yavg, C}, {s->core.e_accu.p, d.o_eaccu, C}, {s->core.e_this.p, d.o_ethis, C}};
    for (const auto& p : parts) MMW_HIP(hipMemcpyAsync(p.dst, f + p.off, p.n * sizeof(double), hipMemcpyDeviceToDevice, s->core.st));
    // The batch adds X_i / Y_i to the running sums when iteration i starts; a handle adds them as soon as they are made while
    // iterations remain (mmw_gap reads iter + 1 terms then).  Before the last iteration the handle's sums hold the current X / Y too.
    if (bt->core.iter[b] < bt->core.nit[b]) {
        const unsigned gx = (unsigned)std::min<size_t>((nnz + BLOCK - 1) / BLOCK, 4096), gy = (unsigned)std::min<size_t>((C + BLOCK - 1) / BLOCK, 4096);
        hipLaunchKernelGGL((k_accumulate<double>), dim3(gx), dim3(BLOCK), 0, s->core.st, nnz, s->core.xval.p, s->core.xavg.p);
        hipLaunchKernelGGL((k_accumulate<double>), dim3(gy), dim3(BLOCK), 0, s->core.st, C, s->core.Y.p, s->core.yavg.p);
        MMW_HIP(hipGetLastError());
    }
    // derived copies: L in the LDS-staged SpMM's traversal order (when the handle's blocking is attached; a later attach gathers it
    // from lval itself)
    if (s->core.bt.lval_blk.p && s->core.bt.HB.nent > 0) {
        hipLaunchKernelGGL((k_gather_blocked<double>), dim3(grid_elems((size_t)s->core.bt.HB.nent)), dim3(BLOCK), 0, s->core.st, (size_t)s->core.bt.HB.nent,
                           s->core.bt.b_bepos.p, s->core.lval.p, s->core.bt.lval_blk.p);
        MMW_HIP(hipGetLastError());
    }
    s->core.lblk_stale = false;
    s->core.iter = bt->core.iter[b];
    MMW_HIP(hipStreamSynchronize(s->core.st));
    return MMW_OK;
}
// what mmw_batch_carry and mmw_batch_carry_map ask of one instance of the pair before either looks at its patterns
inline int batch_carry_pair(const char* who, const mmw_batch* dst, const mmw_batch* src, int b) {
    if (dst->core.pat(b).K != src->core.pat(b).K)
        return fail(MMW_ERR_ARG, std::string(who) + ": instance " + std::to_string(b) + ": K = " + std::to_string(dst->core.pat(b).K) + " here, K = " +
                                     std::to_string(src->core.pat(b).K) + " in the source (a carry keeps the users and moves them)");
    return MMW_OK;
}
// mmw_batch_carry_map: the two index maps of one instance (carry_maps, pattern.h); host patterns only, so device -1 batches answer too
inline int batch_carry_map(mmw_batch* dst, mmw_batch* src, int b, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc) {
    MMW_TRY(dst->core.check_inst(b));
    MMW_TRY(src->core.check_inst(b));
    MMW_TRY(batch_carry_pair("mmw_batch_carry_map", dst, src, b));
    const HostPattern& N = dst->core.full(b);
    if (nl != N.nnzL() || nc != N.C())
        return fail(MMW_ERR_ARG, "mmw_batch_carry_map: instance " + std::to_string(b) + ": wrong lengths " + std::to_string(nl) + ", " + std::to_string(nc) +
                                     ", expected nnzL = " + std::to_string(N.nnzL()) + " and C = " + std::to_string(N.C()));
    carry_maps(N, src->core.full(b), lmap, cmap);
    return MMW_OK;
}
// mmw_batch_carry: (e_accu, L, X, Y) of `src`, a batch on the old states that has iterated, re-indexed onto `dst`, a batch on the new
// states that has not (kernels_batch_carry.h).  Every refusal comes before anything is written.  An instance whose source has run
// no iteration is left as creation made it (cold), as mmw_batch_set_slots_warm leaves one.  dst's counters do not change: its
// iterations done stay 0, so a later mmw_batch_set_slots_warm still treats a carried instance that has not iterated as cold.
inline int batch_carry(mmw_batch* dst, mmw_batch* src, const int32_t* take) {
    const char* who = "mmw_batch_carry";
    BatchCore& D = dst->core;
    BatchCore& S = src->core;
    if (dst == src) return fail(MMW_ERR_ARG, "mmw_batch_carry: the batch cannot carry from itself");
    if (D.host_only || S.host_only) return fail(MMW_ERR_STATE, "mmw_batch_carry: host-only batch (created with device -1)");
    if (D.device != S.device) return fail(MMW_ERR_ARG, "mmw_batch_carry: the source lives on device " + std::to_string(S.device) + ", this batch on device " + std::to_string(D.device));
    if (D.B != S.B) return fail(MMW_ERR_ARG, "mmw_batch_carry: the source holds " + std::to_string(S.B) + " instances, this batch " + std::to_string(D.B));
    std::vector<int> tk;
    MMW_TRY(D.takers(who, take, tk));
    for (int b : tk) {
        MMW_TRY(batch_carry_pair(who, dst, src, b));
        if (D.iter[b] != 0)
            return fail(MMW_ERR_STATE, std::string(who) + ": instance " + std::to_string(b) + " has run " + std::to_string(D.iter[b]) + " iterations (carry into a batch that has not iterated)");
    }
    std::vector<int> go;
    for (int b : tk)
        if (S.iter[b] > 0) go.push_back(b);
    if (go.empty()) return MMW_OK;
    constexpr size_t DW = sizeof(BatchDesc) / sizeof(double), IW = sizeof(CarryItem) / sizeof(double);
    static_assert(sizeof(CarryItem) % sizeof(double) == 0, "the staging buffer is one array of doubles");
    const size_t n = go.size();
    int64_t words = 0;  // int32 map entries of the call
    for (int b : go) words += D.pat(b).nnzL() + D.pat(b).C();
    const size_t w_src = 0, w_dst = w_src + DW * n, w_item = w_dst + DW * n, w_map = w_item + IW * n;
    std::vector<double> stage(w_map + (size_t)((words + 1) / 2), 0.0);
    int32_t* maps = reinterpret_cast<int32_t*>(stage.data() + w_map);
    int64_t om = 0;
    for (size_t t = 0; t < n; ++t) {
        const int b = go[t];
        const HostPattern& N = D.full(b);
        std::memcpy(stage.data() + w_src + DW * t, &S.desc[b], sizeof(BatchDesc));
        std::memcpy(stage.data() + w_dst + DW * t, &D.desc[b], sizeof(BatchDesc));
        const CarryItem it{om, om + N.nnzL()};
        std::memcpy(stage.data() + w_item + IW * t, &it, sizeof it);
        carry_maps(N, S.full(b), maps + it.o_lmap, maps + it.o_cmap);
        om += N.nnzL() + N.C();
    }
    MMW_HIP(hipSetDevice(D.device));
    MMW_HIP(hipStreamSynchronize(S.st));  // the source's iterations have landed
    MMW_TRY(D.rl.upload(stage, D.st));
    hipLaunchKernelGGL(k_batch_carry, dim3((unsigned)n), dim3(BATCH_THREADS), 0, D.st, (const BatchDesc*)(D.rl.p + w_src), (const BatchDesc*)(D.rl.p + w_dst),
                       (const CarryItem*)(D.rl.p + w_item), (const int*)(D.rl.p + w_map), (const double*)S.fa.p, D.fa.p);
    MMW_HIP(hipGetLastError());
    MMW_HIP(hipStreamSynchronize(D.st));
    return MMW_OK;
}
