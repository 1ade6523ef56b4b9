// The device-resident MMW solver behind the C ABI: `mmw_solver` is the opaque handle, `Solver<T>` its fp32 / fp64 body (unnamed namespace:
// mmw_api.hip includes this once).  The body holds a core (solver_core.h: device, pattern, iterate, engine, blockings, timers) and its
// parts by value, each with the state and the device buffers of one concern: loop (solver_loop.h: the phases, their scratch, the chunk
// policy), pending and emax (solver_replay.h: the chunk not yet settled, the riding MMW_F_E_MAX), reads (solver_read.h), envl
// (solver_create.h: the lists a handle built on the device -- from a generator or from CSR arrays -- still holds there), extras (solver_extras.h),
// carried (solver_carry.h: the plan a carry brought along).  An ABI method is the
// device guard, `settle`, and one call into a part; whatever a new run invalidates in a part goes through on_restart.
#pragma once
#include "solver_bench.h"
#include "solver_carry.h"
#include "solver_create.h"
#include "solver_loop.h"
#include "solver_read.h"
#include "solver_replay.h"

struct mmw_env {
    mmw::EnvDevice e;
};
struct mmw_csr {
    mmw::CsrDevice c;
};
struct mmw_solver {
    virtual ~mmw_solver() {}
    virtual CarryInfo carry_info() = 0;
    virtual int carry_pattern(const mmw::HostPattern** out) = 0;  // the host pattern with the lists carry_maps merges (fetched if they still lie on the device)
    virtual int carry(mmw_solver* src) = 0;
    virtual int sizes(int64_t out[10]) = 0;
    virtual int set_expm(int method, int max_order, double tol) = 0;
    virtual int set_timing(int enabled) = 0;
    virtual int set_profile(int enabled) = 0;
    virtual int bench_spmm(int blocked, int reps, double* avg_us) = 0;
    virtual int reset(int32_t nit) = 0;
    virtual int set_slots(int32_t Z, int32_t nit, int warm) = 0;
    virtual int set_eta(double eta) = 0;
    virtual int iterate(int32_t n, const double* randv, uint64_t seed) = 0;
    virtual int sync() = 0;
    virtual int sketch(uint64_t seed, int32_t iteration, double* out, int64_t n) = 0;
    virtual int read_f64(int which, double* out, int64_t n) = 0;
    virtual int read_i32(int which, int32_t* out, int64_t n) = 0;
    virtual int gap(double out[3]) = 0;
    virtual int set_gap(int enabled, int32_t m_cap, int32_t first_steps) = 0;
    virtual int read_gap(double* out, int64_t n) = 0;
    virtual int factor(int32_t rank, double* out, uint64_t seed) = 0;
    virtual int factor_spectral(int32_t Z, int32_t index_order, double* out, uint64_t seed) = 0;
    virtual int factor_random(int32_t cols, int32_t index_order, double* out, uint64_t seed) = 0;
    virtual int round(int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out,
                      int32_t* rem_out) = 0;
    virtual int round_env(mmw_env* env, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out,
                          int32_t* rem_out) = 0;
    virtual int round_attempts(mmw_env* env, bool with_env, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule,
                               int32_t* z_out, int32_t* rem_out, int32_t* pick_out, int32_t* z_all) = 0;
    virtual int round_randv(int32_t Zr, int32_t Dp, uint64_t seed, int32_t attempt, double* out, int64_t n) = 0;
};
namespace {
// the two refusals of a handle made with device -1
inline int host_only_handle() { return fail(MMW_ERR_STATE, "host-only handle"); }
inline int host_only_pattern() { return fail(MMW_ERR_STATE, "this handle was created with device -1 (host pattern only)"); }
template <typename T> struct Solver final : mmw_solver {
    SolverCore<T> core;
    SolverLoop<T> loop;
    PendingChunk<T> pending;
    EmaxRecord emax;
    SolverReads<T> reads;
    DeviceLists envl;
    Extras<T> extras;
    CarriedPlan carried;
    explicit Solver(const Switches& s) : core(s), loop(core.sw), extras(core.sw) {}
    ~Solver() override {
        core.bt.join();  // the build thread works on this handle's members
        if (core.host_only) return;
        (void)hipSetDevice(core.device);
        if (core.st) (void)hipStreamDestroy(core.st);
    }
    using Create = SolverCreate<T>;  // mmw_create / mmw_create_from_env / mmw_create_from_csr call Create::init / init_env / init_csr on a fresh handle
    int sizes(int64_t out[10]) override {
        const HostPattern& H = core.H;
        out[0] = core.K; out[1] = core.Z; out[2] = core.D; out[3] = core.eng.lay.Dpad; out[4] = H.nnzL(); out[5] = H.nnzST();
        out[6] = H.E_gain(); out[7] = H.E_asso(); out[8] = H.C(); out[9] = core.iter;
        return MMW_OK;
    }
    int set_expm(int method, int max_order, double tol) override {
        if (method != MMW_EXPM_LANCZOS && method != MMW_EXPM_TAYLOR) return fail(MMW_ERR_ARG, "unknown expm method");
        if (max_order < 1 || max_order > MAX_ORDER) return fail(MMW_ERR_ARG, "max_order must be in [1,16]");
        if (!(tol > 0)) return fail(MMW_ERR_ARG, "tol must be positive");
        core.eng.method = method; core.eng.max_order = max_order; core.eng.tol = tol;
        return MMW_OK;
    }
    int set_timing(int enabled) override {
        core.pt.timing = enabled != 0;
        core.pt.timing_stride = enabled > 1 ? enabled : 1;
        return MMW_OK;
    }
    // SpMM micro-benchmark on the current L values: Tm = 0.5 * L * start_block, `reps` launches
    int bench_spmm(int blocked, int reps, double* avg_us) override {
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        if (blocked && !core.bt.HB.usable) return fail(MMW_ERR_STATE, "no locality blocking for this pattern");
        MMW_TRY(sync());
        return solver_bench_spmm(core, loop, blocked, reps, avg_us);
    }
    int set_profile(int enabled) override {
        if (core.host_only) return host_only_handle();
        MMW_TRY(sync());
        KernelTimers& kt = core.kt;
        kt.on = enabled != 0;
        core.kt_shipped = enabled == 2;  // 2: time the launches of the shipped path (chunks without readback, riding workgroups) as they are
        kt.attach = core.kt_shipped && !core.sw.kt_markers;  // ... the matrix-core product by the events its launch carries itself
        core.eng.kt_exact = kt.on && !core.kt_shipped;
        kt.clear();
        return MMW_OK;
    }
    int set_eta(double eta_) override {
        if (!(eta_ >= 0.0)) return fail(MMW_ERR_ARG, "eta must be non-negative");
        if (!core.host_only) {
            MMW_HIP(hipSetDevice(core.device));
            MMW_TRY(settle());  // a pending chunk was enqueued with the old step size; a replay must use it too
        }
        core.eta = eta_;
        return MMW_OK;
    }
    // same state, new slot count: only the Z-dependent scalars and the D-wide blocks change
    int set_slots(int32_t Z_, int32_t nit_, int warm) override {
        if (core.host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());
        MMW_HIP(hipStreamSynchronize(core.st));
        if (warm && core.iter == 0) warm = 0;  // nothing to continue from
        if (Z_ >= 2) {  // a width the kernels do not cover is refused before anything of the handle changes: it stays on its slot count
            BlockLayout probe{};
            std::string lerr;
            if ((int64_t)Z_ * core.rank_radio > INT32_MAX || make_layout(Z_ * core.rank_radio, V16<T>::N, probe, lerr) != MMW_OK)
                return fail(MMW_ERR_ARG, "mmw_set_slots: " + (lerr.empty() ? std::string("sketch width D too large for this build") : lerr));
        }
        std::string err = update_slots(core.H, Z_);
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_set_slots: " + err);
        core.Z = Z_;
        core.D = core.Z * core.rank_radio;
        MMW_TRY(core.upload_slot_scalars());
        MMW_TRY(core.eng.resize(core.D));
        MMW_TRY(core.Xh.alloc(core.eng.bs));
        MMW_TRY(reads.resize(core));
        MMW_TRY(loop.resize(core));
        MMW_TRY(on_restart(nit_, warm != 0));
        return warm ? core.sums_from_current() : core.initial_point();
    }
    // What a cold and a warm start of a run share, and the one place a new run reaches the parts through: the counters, the policy's
    // history (chunk_policy.h says what each kind keeps), the riding maximum, the pending chunk, the plans.
    int on_restart(int32_t nit_, bool warm) {
        if (nit_ < 1) return fail(MMW_ERR_ARG, "nit must be >= 1");
        core.nit = nit_;
        loop.on_restart(warm, core.iter, nit_);
        core.iter = 0;
        emax.drop();
        pending.clear();
        carried.drop();
        if (core.eng.viol_d.p) MMW_TRY(core.eng.clear_violation());
        return core.eng.reset_plan_history(warm);
    }
    int reset(int32_t nit_) override {
        if (core.host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(on_restart(nit_, false));
        return core.initial_point();
    }
    // a batch enqueued without plan readbacks is verified here; a violated batch is replayed synchronously
    // A chunk that ends with a violation is discarded and run again from its snapshot.  The second attempt is still a chunk without
    // readbacks, but a cautious one: Lanczos steps (no first-order form) at the a-priori order plus one, an exact plan in front of every
    // exponential (no extrapolated ones), the softmax in its two passes for the first iteration.  Only if that one is refused as well --
    // or the matrix has outgrown the 16-bit split of the matrix-core product, which only the per-iteration readback steps around --
    // do the iterations run synchronously (~2.5x the time per iteration).  Hard probes of a bisection (slot counts at the edge of
    // feasibility: the matrix grows faster than any history predicts) took 3 replays per 150 iterations, 29 ms instead of 13.
    int restore_pending() {
        loop.pol.on_discard();
        emax.drop();  // (the reduction enqueued behind the discarded chunk saw its e_this)
        MMW_TRY(core.eng.clear_violation());
        MMW_TRY(pending.restore(core));
        loop.gap.drop_pending();  // the discarded chunk's gap rows: the replay enqueues them again
        core.iter = pending.iter0;
        return core.pt.drop_since(pending.events0, core.st);  // the timers of the discarded chunk (earlier chunks keep theirs)
    }
    void say_replay(int viol, const char* how) const {
        if (!live_switch(LIVE_VERBOSE)) return;
        const ExpmPlan& p = core.eng.last;
        const ChunkPolicy& pol = loop.pol;
        fprintf(stderr, "[replay] iterations %d..%d (Z %d) %s: reason bits %d (1 order, 2 lagged plan, 4 plan, 8 softmax, 16 operands, 32 first-order certificate); launched m %d, first-order %d, one-half %d; "
                        "plan m %d m_eff %d apriori %d rho %.3g absn %.3g est %.2e first_est %.2e tol %.1e\n",
                pending.iter0, pending.iter0 + pending.n - 1, (int)core.H.Z, how, viol, pol.m_guess, (int)pol.first_guess, (int)pol.first_a16_guess, p.m, p.m_eff, p.m_apriori, p.rho, p.absn,
                plan_estimate(p.conv[std::max(0, std::min(p.m_eff, MAX_ORDER))]), plan_estimate(p.first_est), p.tol);
    }
    void accept_plan() {  // a chunk was settled without a violation: eng.last is its last plan
        ChunkPolicy& pol = loop.pol;
        pol.plan_seen = true;
        pol.note_plan(core.eng.last, core.iter);
        pol.m_guess = pol.next_launch_order(core.eng.last, core.eng.max_order, core.iter);
    }
    // the pending chunk, then the gap rows that rode with it (solver_gap.h): read back behind the synchronisation the chunk's plan took
    int settle() {
        MMW_TRY(settle_chunk());
        return loop.gap.collect(core.st, core.d_indptr.p, core.d_col.p);
    }
    int settle_chunk() {
        if (!pending.live) return MMW_OK;
        pending.clear();
        ChunkPolicy& pol = loop.pol;
        ExpmEngine<T>& eng = core.eng;
        int viol = 0;
        MMW_TRY(eng.fetch_plan(&viol));
        if (!viol) {
            accept_plan();
            return MMW_OK;
        }
        ++pol.replays;
        const bool operands_only = (viol & VIOL_OPERANDS) && !pol.first_guess;  // the bf16 split's gate: the fp32 kernel has to take over
        if (viol & VIOL_LAGGED) pol.lagged_missed = true;  // (er-50k: a second chunk missed the same way 32 iterations later)
        say_replay(viol, "discarded");
        MMW_TRY(restore_pending());
        if (core.sw.cautious_replay && !operands_only && eng.method == MMW_EXPM_LANCZOS && pending.n > 1) {
            pol.plan_cautious(eng.last, eng.max_order);
            pol.exact_plans_only = true;
            const int rc = loop.iterate_impl(core, pending.n, nullptr, pending.seed, true);
            pol.exact_plans_only = false;
            MMW_TRY(rc);
            viol = 0;
            MMW_TRY(eng.fetch_plan(&viol));
            if (!viol) {
                accept_plan();
                say_replay(0, "cautious attempt accepted");
                return MMW_OK;
            }
            ++pol.replays;
            say_replay(viol, "cautious attempt discarded");
            MMW_TRY(restore_pending());
        }
        say_replay(0, "replayed synchronously");
        return loop.iterate_impl(core, pending.n, nullptr, pending.seed, false);
    }
    int iterate(int32_t n, const double* randv, uint64_t seed) override {
        if (core.host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(core.device));
        if (n < 0) return fail(MMW_ERR_ARG, "n must be >= 0");
        MMW_TRY(settle());
        if (core.iter + n > core.nit) return fail(MMW_ERR_STATE, "mmw_iterate: more iterations than announced to mmw_create/mmw_reset");
        ChunkPolicy& pol = loop.pol;
        const bool optimistic = randv == nullptr && n > 1 && !core.kt_exact() && !core.sw.sync_plan;  // profiling mode 1 counts exact launches
        if (!optimistic) {
            pol.chain_ok = false;
            MMW_TRY(loop.iterate_impl(core, n, randv, seed, false));
            carried.drop();  // (these iterations read their plans back: eng.last is the run's own now)
            return emax.enqueue(core);
        }
        // Chunks enqueued without plan readbacks.  Each chunk starts from a device snapshot; before the next one starts the
        // plan of the previous is looked at (one sync): a chunk that needed more steps than were launched is restored and
        // replayed with per-iteration readback, and the launch order follows the device.  The last chunk is settled by the
        // next call.  How long a chunk is and what it is launched with: ChunkPolicy::chunk_length / plan_chunk.
        int left = n;
        while (left > 0) {
            MMW_TRY(settle());
            const ExpmPlan& hist = carried.or_last(core.eng.last);  // (after mmw_carry: the source's last plan, for the first chunk)
            const int chunk = pol.chunk_length(hist, core.sw, core.iter, left);
            pol.plan_chunk(hist, core.sw, core.eng.max_order, core.iter, chunk, sizeof(T) == 4, core.bt.afrag16.p != nullptr, loop.plane_rounding());
            MMW_TRY(pending.save(core));
            const int iter0 = core.iter;
            const size_t events0 = core.pt.mark();
            MMW_TRY(loop.iterate_impl(core, chunk, nullptr, seed, chunk > 1));
            pol.warm_fresh = false;
            carried.drop();
            if (chunk > 1) pending.begin(iter0, chunk, seed, events0);
            left -= chunk;
        }
        return emax.enqueue(core);
    }
    // ---- mmw_carry (solver_carry.h): this handle, on the state after the stations moved, takes over the iterate `src_` reached on the
    // state before.  Every refusal comes before anything of either handle is touched; a source that never iterated leaves this handle cold.
    CarryInfo carry_info() override { return CarryInfo{core.host_only, core.device, sizeof(T) == 4 ? MMW_F32 : MMW_F64, core.K, core.iter}; }
    int carry_pattern(const HostPattern** out) override {
        MMW_TRY(envl.ensure_host(core));
        *out = &core.H;
        return MMW_OK;
    }
    int carry(mmw_solver* src_) override {
        if (src_ == this) return fail(MMW_ERR_ARG, "mmw_carry: the handle cannot carry from itself");
        MMW_TRY(carry_refusal("mmw_carry", carry_info(), src_->carry_info(), true));
        Solver<T>* src = static_cast<Solver<T>*>(src_);  // (same dtype: checked)
        if (src->core.iter == 0) return MMW_OK;  // nothing to continue from: the fallback of mmw_set_slots_warm
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(src->settle());
        MMW_TRY(src->core.x.csr_view(src->core));
        MMW_HIP(hipStreamSynchronize(src->core.st));
        MMW_TRY(SolverCarry<T>::gather(core, src->core));
        MMW_TRY(SolverCarry<T>::derived(core));
        emax.drop();
        pending.clear();
        MMW_TRY(SolverCarry<T>::history(core, loop, carried, src->core, src->loop));
        // the gather reads the source's buffers from THIS handle's stream, which nothing orders against the source's: it has to be over
        // before the caller may continue, reset or destroy the source (mmw_batch_carry ends the same way)
        MMW_HIP(hipStreamSynchronize(core.st));
        return MMW_OK;
    }
    int sync() override {
        if (core.host_only) return host_only_pattern();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());
        MMW_TRY(emax.fetch_at_sync(core));
        MMW_TRY(core.kt.flush());
        return core.pt.flush(core.iter, core.st);
    }
    int sketch(uint64_t seed, int32_t iteration, double* out, int64_t n) override {
        if (core.host_only) return host_only_pattern();
        if (iteration < 0) return fail(MMW_ERR_ARG, "mmw_sketch: iteration must be >= 0");
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(sync());
        return reads.sketch(core, seed, iteration, out, n);
    }
    int read_f64(int which, double* out, int64_t n) override {
        // the fields a host-only handle holds too
        const HostPattern& H = core.H;
        const std::vector<double>* hv = which == MMW_F_S_SUM ? &H.S_sum : which == MMW_F_NORM_H ? &H.norm_H : which == MMW_F_ST_DATA ? &H.st_data : nullptr;
        if (core.host_only && which == MMW_F_LAPLACIAN) {  // kernels_spectral.h's row function in a plain loop
            if (n != H.nnzL()) return fail(MMW_ERR_ARG, "mmw_read_f64(LAPLACIAN): wrong length " + std::to_string(n) + ", expected " + std::to_string(H.nnzL()));
            for (int r = 0; r < core.K; ++r) lap_row(H.l_indptr.data(), H.l_indices.data(), H.so_indptr.data(), H.so_indices.data(), H.so_data.data(), r, out);
            return MMW_OK;
        }
        if (core.host_only) return hv ? export_vec(*hv, out, n, "mmw_read_f64") : host_only_pattern();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(sync());
        if (which == MMW_F_ST_DATA) MMW_TRY(envl.ensure_host(core));
        if (hv) return export_vec(*hv, out, n, "mmw_read_f64");
        if (which == MMW_F_LAPLACIAN) return extras.read_laplacian(core.d_indptr.p, core.d_col.p, core.d_diag.p, (size_t)H.nnzL(), out, n);
        return reads.read_f64(core, loop, emax, extras, which, out, n);
    }
    int read_i32(int which, int32_t* out, int64_t n) override {
        if (which == MMW_I_ROUND_LIST_BUILDS) {  // a counter, not a list: nothing is fetched for it
            if (n != 1) return fail(MMW_ERR_ARG, "mmw_read_i32(ROUND_LIST_BUILDS): wrong length");
            out[0] = extras.env_builds;
            return MMW_OK;
        }
        MMW_TRY(envl.ensure_host(core));
        const std::vector<int32_t>* v = host_list_i32(core.H, which);
        return v ? export_vec(*v, out, n, "mmw_read_i32") : fail(MMW_ERR_ARG, "mmw_read_i32: unknown field");
    }
    int gap(double out[3]) override {
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());
        if (core.iter >= core.nit) return fail(MMW_ERR_STATE, "mmw_gap: call it before an iteration (the running sums then hold iter+1 terms)");
        MMW_TRY(core.x.csr_view(core));
        PatternDev<T> Pc = core.pat();  // the gap's kernels walk the CSR copy
        Pc.e2w = nullptr; Pc.xasso = nullptr; Pc.xdiag_base = -1;
        return extras.gap(Pc, core.d_lrow.p, core.xavg.p, core.yavg.p, core.iter + 1, out);
    }
    // ---- mmw_set_gap / mmw_read_gap: the gap row of every iteration, logged inside the loop (solver_gap.h, kernels_gap.h)
    int set_gap(int enabled, int32_t m_cap, int32_t first_steps) override {
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());  // rows in flight belong to the old setting
        return loop.gap.configure(enabled, m_cap, first_steps, core.K, (size_t)core.H.nnzL(), core.nit);
    }
    int read_gap(double* out, int64_t n) override {
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());
        return loop.gap.read(core.iter, out, n);
    }
    int factor(int32_t rank, double* out, uint64_t seed) override {
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());
        if (core.iter < core.nit) return fail(MMW_ERR_STATE, "mmw_factor: run all announced iterations first (the average divides by nit)");
        MMW_TRY(core.x.csr_view(core));
        return extras.factor(core.d_indptr.p, core.d_col.p, core.xavg.p, core.nit, rank, out, seed);
    }
    // sdp_solver.spectral_sdp_solver.run_with_state on the handle's state: the factor's iteration on the Laplacian (solver_extras.h).  The
    // iterate, its sums and the handle's slot count play no part.
    int factor_spectral(int32_t Z, int32_t index_order, double* out, uint64_t seed) override {
        if (Z < 1 || Z > core.K) return fail(MMW_ERR_ARG, "mmw_factor_spectral: Z = " + std::to_string(Z) + " must be in [1, K = " + std::to_string(core.K) + "]");
        if (index_order != 0 && index_order != 1) return fail(MMW_ERR_ARG, "mmw_factor_spectral: index_order must be 0 or 1");
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        MMW_TRY(settle());
        return extras.factor_spectral(core.d_indptr.p, core.d_col.p, core.d_diag.p, (size_t)core.H.nnzL(), Z, index_order, out, seed);
    }
    // rand_sdp_solver.run_with_state as the handle's resident factor (solver_extras.h, factor_random).  The iterate, its sums and a chunk in
    // flight play no part: nothing is settled, the draw queues behind the chunk on the handle's stream.
    int factor_random(int32_t cols, int32_t index_order, double* out, uint64_t seed) override {
        if (cols < 1) return fail(MMW_ERR_ARG, "mmw_factor_random: cols = " + std::to_string(cols) + " must be >= 1");
        if (index_order != 0 && index_order != 1) return fail(MMW_ERR_ARG, "mmw_factor_random: index_order = " + std::to_string(index_order) + " must be 0 or 1");
        if (cols > MMW_FACTOR_RANDOM_MAX_COLS)
            return fail(MMW_ERR_ARG, "mmw_factor_random: cols = " + std::to_string(cols) + " exceeds " + std::to_string(MMW_FACTOR_RANDOM_MAX_COLS) +
                                         ", the widest D' the rounding's projection walks in its 64-column slabs");
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        return extras.factor_random(cols, index_order, out, seed);
    }
    int round(int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out, int32_t* rem_out) override {
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        return extras.round(Zr, Dp, gX, nbatch, randv, z_out, rem_out);
    }
    // mmw_round against the state `env` holds now (solver_extras.h, round_env).  What cannot run is refused before the device is touched.
    int round_env(mmw_env* env, int32_t Zr, int32_t Dp, const double* gX, int32_t nbatch, const double* randv, int32_t* z_out, int32_t* rem_out) override {
        if (core.host_only) return host_only_handle();
        if (!env) return fail(MMW_ERR_ARG, "mmw_round_env: null environment");
        const EnvDevice& E = env->e;
        if (E.K != core.K)
            return fail(MMW_ERR_ARG, "mmw_round_env: the environment has K = " + std::to_string(E.K) + " stations, the handle K = " + std::to_string(core.K));
        if (E.device != core.device)
            return fail(MMW_ERR_ARG, "mmw_round_env: the environment lies on device " + std::to_string(E.device) + ", the handle on device " + std::to_string(core.device));
        MMW_HIP(hipSetDevice(core.device));
        return extras.round_env(E.list_source(), Zr, Dp, gX, nbatch, randv, z_out, rem_out);
    }
    // mmw_round_attempts (with_env = false) and mmw_round_env_attempts: all attempts of one rounding() call, drawn and chosen among on the
    // device (solver_extras.h, round_attempts_on).  The refusals come first, those that read the arguments only before the handle's own.
    int round_attempts(mmw_env* env, bool with_env, int32_t Zr, int32_t Dp, const double* gX, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out,
                       int32_t* rem_out, int32_t* pick_out, int32_t* z_all) override {
        const std::string who = with_env ? "mmw_round_env_attempts" : "mmw_round_attempts";
        MMW_TRY(Extras<T>::attempts_check(who, Zr, Dp, nattempt, pick_rule, z_out, rem_out, pick_out));
        if (core.K > ROUND_PICK_MAX_K) return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(core.K) + " exceeds " + std::to_string(ROUND_PICK_MAX_K) + ", the most users the pick's key holds");
        if (core.host_only) return host_only_handle();
        if (!with_env) {
            MMW_HIP(hipSetDevice(core.device));
            return extras.round_attempts(Zr, Dp, gX, nattempt, seed, pick_rule, z_out, rem_out, pick_out, z_all);
        }
        if (!env) return fail(MMW_ERR_ARG, who + ": null environment");
        const EnvDevice& E = env->e;
        if (E.K != core.K)
            return fail(MMW_ERR_ARG, who + ": the environment has K = " + std::to_string(E.K) + " stations, the handle K = " + std::to_string(core.K));
        if (E.device != core.device)
            return fail(MMW_ERR_ARG, who + ": the environment lies on device " + std::to_string(E.device) + ", the handle on device " + std::to_string(core.device));
        MMW_HIP(hipSetDevice(core.device));
        return extras.round_env_attempts(E.list_source(), Zr, Dp, gX, nattempt, seed, pick_rule, z_out, rem_out, pick_out, z_all);
    }
    int round_randv(int32_t Zr, int32_t Dp, uint64_t seed, int32_t attempt, double* out, int64_t n) override {
        if (Zr < 1 || Dp < 1) return fail(MMW_ERR_ARG, "mmw_round_randv: Z and D' must be positive");
        if (attempt < 0) return fail(MMW_ERR_ARG, "mmw_round_randv: attempt must be >= 0");
        if (!out || n != (int64_t)Zr * Dp) return fail(MMW_ERR_ARG, "mmw_round_randv: out must hold Z x D' values");
        if (core.host_only) return host_only_handle();
        MMW_HIP(hipSetDevice(core.device));
        return extras.round_randv(Zr, Dp, seed, attempt, out);
    }
};
template <typename T>
int expm_apply_impl(const Switches& sw, int device, int method, int max_order, double tol, int32_t K, int32_t D, const int32_t* indptr,
                    const int32_t* indices, const double* data, const double* B, double* out, double info[4], int32_t reps,
                    double* kernel_us) {
    MMW_HIP(hipSetDevice(device));
    hipStream_t st;
    MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    ScopedStream guard{st};
    const int64_t nnz = indptr[K];
    std::vector<int32_t> ip(indptr, indptr + K + 1), ci(indices, indices + nnz);
    std::vector<double> vv(data, data + nnz);
    DevBuf<int> d_ip, d_ci;
    DevBuf<T> d_v, d_out;
    DevBuf<double> d_b64, d_o64;
    MMW_TRY(d_ip.upload(ip, st));
    MMW_TRY(d_ci.upload(ci, st));
    MMW_TRY(d_v.upload_cast(vv, st));
    ExpmEngine<T> eng(sw);
    MMW_TRY(eng.init(st, K, D, d_ip.p, d_ci.p, d_v.p));
    eng.method = method; eng.max_order = max_order; eng.tol = tol;
    MMW_TRY(d_out.alloc(eng.bs));
    MMW_TRY(d_b64.alloc((size_t)K * D));
    MMW_TRY(d_o64.alloc((size_t)K * D));
    MMW_TRY(copy_h2d(d_b64.p, B, (size_t)K * D * sizeof(double), st));
    hipEvent_t e0, e1;
    MMW_HIP(hipEventCreate(&e0));
    MMW_HIP(hipEventCreate(&e1));
    double us = 0.0;
    if (reps < 1) reps = 1;
    for (int r = 0; r < reps; ++r) {
        hipLaunchKernelGGL((k_import_block<T>), dim3(grid_elems(eng.bs)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, d_b64.p, eng.start_block());
        MMW_HIP(hipEventRecord(e0, st));
        int rc = eng.apply(d_out.p, 1.0);
        if (rc != MMW_OK) return rc;
        MMW_HIP(hipEventRecord(e1, st));
        MMW_HIP(hipStreamSynchronize(st));
        float ms = 0;
        MMW_HIP(hipEventElapsedTime(&ms, e0, e1));
        us += ms * 1e3;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    hipLaunchKernelGGL((k_export_block<T>), dim3(grid_elems((size_t)K * D)), dim3(BLOCK), 0, st, K, D, eng.lay.Dpad, d_out.p, d_o64.p);
    MMW_HIP(hipGetLastError());
    MMW_TRY(copy_d2h(out, d_o64.p, (size_t)K * D * sizeof(double), st));
    if (info) {
        info[0] = eng.last.rho; info[1] = eng.last.m_eff > 0 ? eng.last.m_eff : eng.last.m; info[2] = eng.last.nsub; info[3] = eng.last.mu;
    }
    if (kernel_us) *kernel_us = us / reps;
    return MMW_OK;
}
// mmw_create / mmw_create_from_env / mmw_create_from_csr: a handle of the asked dtype, initialised by `init` (SolverCreate<T>::init, init_env or init_csr), handed out on success
template <typename Init> int create_solver(mmw_solver** out, int dtype, bool host_only, Init&& init) {
    auto make = [&](auto s) {
        s->core.host_only = host_only;
        const int rc = init(*s);
        if (rc == MMW_OK) *out = s.release();
        return rc;
    };
    if (dtype == MMW_F32) return make(std::make_unique<Solver<float>>(Switches::from_env()));
    if (dtype == MMW_F64) return make(std::make_unique<Solver<double>>(Switches::from_env()));
    return fail(MMW_ERR_ARG, "dtype must be MMW_F32 or MMW_F64");
}
}  // namespace
