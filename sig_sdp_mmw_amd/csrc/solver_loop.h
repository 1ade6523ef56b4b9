// The loop of the solver handle (solver.h): one call of iterate_impl enqueues `n` iterations -- per call a ChunkRun, per iteration the
// phases DUAL, LOSS, sketch + exponential, X on the pattern -- on the iterate the core holds (solver_core.h).  SolverLoop owns what only
// the phases touch: their scratch, the chunk policy, the sketch an earlier launch drew, the counters of MMW_F_DUAL_INFO.
// While mmw_set_gap is on, every iteration is preceded by its LOG_GAP row (solver_gap.h), enqueued in front of the phase timers' events.
//   discard of a chunk   nothing here is restored: the scratch is rewritten by the replay, `carry` is forgotten by every iterate_impl
//   reset / warm restart on_restart: the policy's history (chunk_policy.h says what each kind keeps); the counters run on
#pragma once
#include "solver_core.h"
#include "solver_gap.h"

namespace {
// The sketch that rode in an earlier launch (a LOSS pass or the previous SDDMM launch drew it into the start block), and where the last
// sketch came from (MMW_F_SKETCH draws it again).
struct SketchCarry {
    int64_t done_for = -1;  // iteration whose sketch the start block already holds
    uint64_t done_seed = 0;
    int slabs = 0;          // norm slabs that launch left
    uint64_t last_seed = 0;
    bool last_was_rng = false;
    template <typename Run> bool drawn(const Run& c, int iter) const { return !c.randv && done_for == (int64_t)iter && done_seed == c.seed; }
    void note(int64_t iter, uint64_t seed, int nslabs) { done_for = iter; done_seed = seed; slabs = nslabs; }
    void forget() { done_for = -1; }
    void used(uint64_t seed) { forget(); last_was_rng = true; last_seed = seed; }  // a device-drawn sketch went into an exponential
    void uploaded() { last_was_rng = false; }
};
template <typename T> struct SolverLoop {
    using Core = SolverCore<T>;
    explicit SolverLoop(const Switches& sw)
        : dual_gap(std::isnan(sw.dual_gap) ? (sizeof(T) == 4 ? 60.0 : 600.0) : sw.dual_gap), fv_measure(!sw.fv_worstcase), rs_enabled(!sw.no_sddmm_rowsums) {}
    ChunkPolicy pol;  // the run's planning history and the next chunk's guesses (chunk_policy.h)
    SketchCarry carry;
    DevBuf<T> rsum, drow;
    DevBuf<double> max_part, sum_part, scal, tr_part, stage64;
    DevBuf<T> wH;  // Y_H / norm_H
    DevBuf<T> yun;  // the fused DUAL pass's unnormalised exponentials (see iterate_impl)
    // how far e_accu's maximum may run ahead of the fused pass's shift before its exponentials are distrusted (exp overflows T
    // near 88 / 709); MMW_DUAL_GAP is for the tests, which force the replay with it
    const double dual_gap;
    static constexpr int LOSS_GRID_MAX = 4096;
    DevBuf<unsigned short> xh_planes;
    DevBuf<long long> rsfx;  // [2K] 2^-40 fixed-point totals: [0, K) row sums of the off-diagonal X, left by the matrix-core SDDMM; [K, 2K) row norms of
                             // y = exp(L/2)R from the first-order product (kernels_mfma.h).  Zeroed by every LOSS pass.
    DevBuf<double> tr1_part; // trace shares of the first-order product's workgroups (zero where none works)
    // the rounding of the first-order product's fp16 plane: measured by the sketch kernel (default), or the format's worst case
    const bool fv_measure;
    double plane_rounding() const { return fv_measure ? F16_PLANE_EXPECT : 1.02 * F16_UNIT; }
    bool rs_last = false;    // the last iteration enqueued left rsfx for the X the next one starts from
    const bool rs_enabled;
    long long n_rs_iters = 0, n_fused_iters = 0, n_first_iters = 0, n_first16_iters = 0;  // MMW_F_DUAL_INFO
    GapPhase<T> gap;  // the logged duality gap (mmw_set_gap; solver_gap.h): reads the iterate, writes its own buffers
    // init_common (solver_create.h), in its order of allocation
    int alloc_scratch(const Core& co) {
        const int K = co.K;
        MMW_TRY(rsum.alloc(K)); MMW_TRY(drow.alloc(K));
        MMW_TRY(max_part.alloc(ROW_GRID_MAX)); MMW_TRY(sum_part.alloc(4 * (size_t)std::max(2048, ROW_GRID_MAX))); MMW_TRY(scal.alloc(8));
        MMW_TRY(tr_part.alloc(ROW_GRID_MAX)); MMW_TRY(wH.alloc(K));
        return MMW_OK;
    }
    int resize(const Core& co) { return stage64.alloc((size_t)co.K * co.D); }  // the uploaded sketch's staging block follows K x D
    void on_restart(bool warm, int iter, int nit) {
        if (warm) pol.on_warm_restart(iter);
        else pol.on_reset();
        if (gap.ever) gap.clear_log(nit);
    }
    int sketch_slabs(const Core& co) const { return std::min(grid_rows(co.K), co.sw.sk_slabs); }  // few slabs for the start-norm reduction
    int launch_sketch(Core& co, hipStream_t s, uint64_t seed, uint32_t it, bool planes_f16 = false) {
        const bool lz = co.eng.method == MMW_EXPM_LANCZOS;
        unsigned short* pl = co.eng.start_planes();
        hipLaunchKernelGGL((k_sketch_rng<T>), dim3(sketch_slabs(co)), dim3(BLOCK), lz ? (size_t)(WAVES_PER_BLOCK + 1) * co.eng.lay.Dpad * sizeof(double) : 0, s, co.K, co.D, co.eng.lay.Dpad,
                           seed, it, co.eng.start_block(), lz ? co.eng.partial_sq.p : (double*)nullptr, pl, planes_f16 ? 1 : 0,
                           planes_f16 && lz && fv_measure ? co.eng.partial_du.p : (double*)nullptr);
        co.eng.planes_ready[0] = pl != nullptr;
        co.eng.planes0_f16 = planes_f16 && pl != nullptr;
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    // One call of iterate_impl: what is fixed for its `n` iterations, then what one iteration leaves for the next.
    struct ChunkRun {
        int n; const double* randv; uint64_t seed; bool optimistic;
        bool lanczos;     // eng.method == MMW_EXPM_LANCZOS
        // X on the pattern comes from the matrix-core SDDMM in this call: it writes -- and the DUAL phase then reads -- X in tile order;
        // every other SDDMM form works on the CSR order
        bool sd_mf_call;
        PatternDev<T> P;
        const T* xcur;    // the X the DUAL phase reads (the layout does not change inside a call)
        int gr, gd, gc, gl, Dpad;  // grids of the row kernels, the DUAL pass, the softmax passes and the LOSS pass
        int m_launch;     // Lanczos steps launched per exponential (0: as the plan read back says)
        bool lag_chunk, chain, chain_plan, fuse_sketch;
        // carried from one iteration to the next
        bool xavg_deferred = false;  // the X just made is added to its running sum by the next iteration's LOSS pass
        bool rs_ok = false;          // rsfx holds the row sums of the X the next DUAL phase starts from
        FirstVerify fv_pending;      // the first-order exponential of the previous iteration of this call still waits for its check
    };
    // what the phases of ONE iteration hand each other
    struct IterRun {
        int it, acc;  // index within the call; 1: X / Y of this iteration go into the running sums
        bool lagged_it = false, fused_dual = false, rs_zeroed = false, first_it = false;
        PlanArgs pa;
        int ntr1 = 0;
    };
    template <int NCH, bool POW2 = true> void launch_sddmm(Core& co, const ChunkRun& c, int acc) {
        hipLaunchKernelGGL((k_sddmm<T, NCH, POW2>), dim3(c.gr), dim3(BLOCK), 0, co.st, c.P, c.Dpad, co.eng.lay.LPR, co.eng.lay.G, co.Xh.p, drow.p, tr_part.p, c.gr, co.xval.p, co.xavg.p, acc);
    }
    template <int MT, int NB>
    int launch_sddmm_mfma(Core& co, const ChunkRun& c, dim3 grid, const SdMfmaDev& SM, const double* trp, int ntr, int acc, long long* rs_out, const long long* dfx,
                          unsigned long long* stamps, const FirstVerify& fv) {
        MMW_TRY(set_max_lds(reinterpret_cast<const void*>(&k_sddmm_mfma<MT, NB>), sdm_lds_bytes<MT, NB>()));
        hipLaunchKernelGGL((k_sddmm_mfma<MT, NB>), grid, dim3(256 * MT), (sdm_lds_bytes<MT, NB>()), co.st, co.eng.mf, SM, co.K, c.Dpad,
                           reinterpret_cast<const char*>(xh_planes.p), drow.p, trp, ntr, co.x.xs_val.p, co.x.xs_avg.p, acc, rs_out, dfx, stamps, fv);
        return MMW_OK;
    }
    int iterate_impl(Core& co, int32_t n, const double* randv, uint64_t seed, bool optimistic) {
        ChunkRun c{n, randv, seed, optimistic, co.eng.method == MMW_EXPM_LANCZOS};
        c.sd_mf_call = sizeof(T) == 4 && co.bt.sddmm_mfma && co.eng.use_blk && c.lanczos && (co.eng.lay.Dpad % 32) == 0 && co.bt.b_e2w.p != nullptr;
        if (n > 0) MMW_TRY(c.sd_mf_call ? co.x.to_tiles(co) : co.x.to_csr(co));
        c.P = co.pat();
        c.xcur = co.x.live(co).val->p;
        c.gr = grid_rows(co.K);
        // the DUAL pass's grid: its workgroups stride over the row pairs, and the slabs it leaves (maxima, softmax sums, |L| row sums) are
        // folded by one workgroup afterwards.  One resident round of workgroups (five per CU at the pass's 86 registers) instead of one per
        // eight rows: half the slabs to fold and no second round's tail -- DUAL 21.0 -> 20.0 us per step at the benchmark (640: 22.3; 1920: 20.2)
        c.gd = std::min(c.gr, 5 * device_cus());
        c.gc = grid_elems((size_t)co.H.C());
        c.gl = (int)std::min<size_t>(((size_t)co.H.nnzL() + BLOCK - 1) / BLOCK, (size_t)LOSS_GRID_MAX);  // LOSS: one thread per stored entry, grid-stride
        c.Dpad = co.eng.lay.Dpad;
        c.m_launch = optimistic ? pol.m_guess : 0;
        // from the plan the last settled chunk ended on; not in the first chunk after a warm restart: with another slot count the matrix grows
        // at another rate than the history the extrapolation rests on (its bound was missed and the chunk replayed, measured)
        // (after mmw_carry the plan the chunk was planned on lies in Solver::carried and eng.last is still zero: this and plan_has_room below
        // read eng.last, which is right only because warm_fresh masks the first chunk here and chain_ok is false until a chunk has settled)
        c.lag_chunk = optimistic && pol.lagged_ok(co.eng.last, co.sw) && !pol.warm_fresh && !pol.exact_plans_only;
        c.chain = optimistic && pol.chain_ok;      // this chunk continues the previous one (see ChunkPolicy::chain_ok)
        pol.chain_ok = false;
        // the plan is chained only while a single step is accepted with a factor 8 to spare: near a change of order an exact plan at
        // the start of every chunk keeps the a-priori order down (er-1pct: 5 127 it/s with it, 4 495 without)
        c.chain_plan = c.chain && pol.plan_has_room(co.eng.last);
        // the row sums of X the DUAL phase starts from: left by the last matrix-core SDDMM (this call's previous iteration, or the chunk
        // this one continues), otherwise taken by k_dual_rows
        c.rs_ok = c.chain && rs_last && rs_enabled && rsfx.p != nullptr;
        rs_last = false;
        // drawing the next sketch in extra workgroups of the SDDMM launch paid off with 8-wave SDDMM workgroups (+3.7 %); with
        // 16-wave ones (two per CU, every wave slot taken) it costs 1.5 %, so it is opt-in
        c.fuse_sketch = !co.kt_exact() && !co.pt.timing && co.sw.fused_sketch;
        carry.forget();  // whatever an earlier batch left in the start block is not trusted
        for (int it = 0; it < n; ++it) {
            IterRun s;
            s.it = it;
            s.acc = (co.iter + 1 < co.nit) ? 1 : 0;  // the last X / Y are not averaged (mmw.py:77-78,203)
            // LOG_GAP (mmw.py:79-117): the row of the iteration that starts, in front of the phase timers' first event
            if (gap.on) MMW_TRY(gap.enqueue_row(co.st, co.H, c.P, co.d_lrow.p, co.x.live(co).avg->p, c.xavg_deferred ? c.xcur : (const T*)nullptr, co.yavg.p, co.iter));
            MMW_TRY(co.pt.record(0, co.iter, co.st));
            MMW_TRY(phase_dual(co, c, s));
            MMW_TRY(phase_loss(co, c, s));
            MMW_TRY(phase_expm(co, c, s));
            MMW_TRY(phase_x(co, c, s));
            ++co.iter;
            if (!optimistic) MMW_TRY(gap.collect(co.st, co.d_indptr.p, co.d_col.p));  // (this path reads its plans back every iteration)
        }
        MMW_TRY(chunk_tail(co, c));
        return gap.queue_copy(co.st);
    }
    // ---- DUAL: the violations of the current X, their softmax, and (lagged) the plan of this iteration's exponential
    int phase_dual(Core& co, ChunkRun& c, IterRun& s) {
        MMW_TRY(co.kt.begin(KT_DUAL));
        const long long* rs_it = c.rs_ok ? rsfx.p : nullptr;
        const FirstVerify fv = c.fv_pending;
        c.fv_pending = FirstVerify{};
        if (rs_it) ++n_rs_iters;
        if (!rs_it) hipLaunchKernelGGL((k_dual_rows<T>), dim3(c.gr), dim3(BLOCK), 0, co.st, c.P, c.xcur, rsum.p, co.e_this.p);
        // Lagged planning inside a chunk (not the first iteration of a run, a replay or after a change of the iterate, which plan exactly): k_dual_h also takes the row sums of the
        // L it walks over anyway -- last iteration's -- and one extra workgroup of k_softmax_b turns them into this iteration's plan
        // (extrapolated bounds, checked by the next plan): k_rowsums + k_plan leave the critical path.
        s.lagged_it = c.optimistic && (s.it > 0 || c.chain_plan) && c.lanczos && c.lag_chunk;
        if (s.lagged_it) {
            s.pa.plan = co.eng.plan_d.p; s.pa.part = co.eng.row_part.p; s.pa.viol = co.eng.viol_d.p; s.pa.tol = co.eng.tol; s.pa.K = co.K; s.pa.method = co.eng.method;
            s.pa.max_order = co.eng.max_order; s.pa.np = c.gd; s.pa.m_launch = c.m_launch; s.pa.apost = co.eng.apost() ? 1 : 0; s.pa.iter_seen = pol.age(co.iter) - 1;
        }
        // Inside a chunk (not its first iteration) the softmax rides in k_dual_h, shifted by the previous iteration's maximum
        // instead of this one's: one small workgroup then folds the sums, and the LOSS pass normalises where it reads
        // (kernels_loop.h, k_dual_h / k_dual_scal).  Two launches of the dependent chain fewer.
        s.fused_dual = c.optimistic && (s.it > 0 || c.chain) && !co.sw.no_fused_dual;
        if (s.fused_dual) {
            ++n_fused_iters;
            if (yun.n < (size_t)co.H.C()) MMW_TRY(yun.alloc((size_t)co.H.C()));
            // MMW_DUAL_STAMPS=1 (developer aid): per-wave phase clocks of the last iteration's launch, printed to stderr
            StampBuf dh_stamps;
            const bool want_dst = s.it + 1 == c.n && live_switch(LIVE_DUAL_STAMPS);
            MMW_TRY(dh_stamps.request(want_dst, (size_t)c.gd * WAVES_PER_BLOCK * 8, co.st));
            hipLaunchKernelGGL((k_dual_h<T>), dim3(c.gd), dim3(BLOCK), 0, co.st, c.P, rsum.p, co.e_this.p, co.e_accu.p, co.eta, max_part.p,
                               (const T*)(s.lagged_it ? co.lval.p : nullptr), 0.5, co.eng.row_part.p, (const double*)(scal.p + 4), yun.p, wH.p, sum_part.p,
                               rs_it, c.xcur, FirstVerify{}, dh_stamps.p());
            if (want_dst) MMW_TRY(dump_dual_stamps(co.st, dh_stamps.p(), c.gd));
            hipLaunchKernelGGL(k_dual_scal, dim3(1 + fv.nwg), dim3(DSCAL_THREADS), 0, co.st, sum_part.p, max_part.p, c.gd, scal.p,
                               dual_gap, co.eng.viol_d.p, fv);
        } else {
            hipLaunchKernelGGL((k_dual_h<T>), dim3(c.gd + fv.nwg), dim3(BLOCK), 0, co.st, c.P, rsum.p, co.e_this.p, co.e_accu.p, co.eta, max_part.p,
                               (const T*)(s.lagged_it ? co.lval.p : nullptr), 0.5, co.eng.row_part.p, (const double*)nullptr, (T*)nullptr, (T*)nullptr,
                               (double*)nullptr, rs_it, c.xcur, fv);
            hipLaunchKernelGGL((k_softmax_a<T>), dim3(c.gc), dim3(BLOCK), 0, co.st, c.P, co.e_accu.p, co.Y.p, max_part.p, c.gd, sum_part.p);
            hipLaunchKernelGGL((k_softmax_b<T>), dim3(c.gc + (s.lagged_it ? 1 : 0)), dim3(BLOCK), 0, co.st, (int)co.H.C(), co.Y.p, co.yavg.p, s.acc, sum_part.p, c.gc, scal.p,
                               co.K + (int)co.H.E_asso(), co.d_invn.p, wH.p, s.pa, max_part.p, c.gd);
        }
        MMW_TRY(co.kt.end());
        MMW_TRY(co.pt.record(1, co.iter, co.st));
        return MMW_OK;
    }
    // ---- LOSS: L += eta * loss(Y); this iteration's sketch rides in its launch
    int phase_loss(Core& co, ChunkRun& c, IterRun& s) {
        MMW_TRY(co.kt.begin(KT_LOSS));
        // the X of the previous iteration of this chunk is added to the running sum inside this pass (xavg_deferred), and
        // this iteration's sketch is drawn by leading workgroups of the same launch (VALU work under a memory-bound pass)
        s.rs_zeroed = rs_enabled && rsfx.p != nullptr && co.bt.sddmm_mfma;  // the coming SDDMM may add its row sums to zeroed totals
        // the exponential of this iteration as one first-order product (decided per chunk, first_order_ok)
        const bool sketch_have = carry.drawn(c, co.iter);
        // (a sketch an earlier launch already drew came without the fp16 plane and the measure of its rounding: no first-order form then)
        s.first_it = c.optimistic && pol.first_guess && c.m_launch == 1 && !c.randv && s.rs_zeroed && sizeof(T) == 4 && co.eng.mfma_now() &&
                              c.lanczos && co.eng.use_blk && (c.Dpad % 32) == 0 && !sketch_have;
        SketchArgs<T> skl{};
        // (with the per-iteration phase events of mmw_set_timing on as well: the draw then counts into the LOSS phase's microseconds
        // instead of the exponential's -- the reference draws inside mmw.py:172-181 -- and the iteration's total is unchanged; a launch of
        // its own cost the class path 14 us per iteration)
        if (!c.randv && !sketch_have && !co.kt_exact() && !co.sw.no_loss_sketch) {
            skl.nblocks = sketch_slabs(co); skl.K = co.K; skl.D = co.D; skl.seed = c.seed; skl.iter = (uint32_t)co.iter;
            skl.R = co.eng.start_block();
            skl.colsq_part = c.lanczos ? co.eng.partial_sq.p : nullptr;
            skl.planes = co.eng.start_planes();
            skl.planes_f16 = s.first_it ? 1 : 0;
            skl.dusq_part = s.first_it && fv_measure ? co.eng.partial_du.p : nullptr;
            co.eng.planes_ready[0] = skl.planes != nullptr;
            co.eng.planes0_f16 = s.first_it && skl.planes != nullptr;
            carry.note((int64_t)co.iter, c.seed, skl.nblocks);
        }
        // the blocked copy of L feeds the fp32 LDS kernel only: while the matrix-core kernel runs the products it is left stale
        const bool mf_it = co.eng.mfma_now() && c.lanczos;
        if (mf_it) co.lblk_stale = true;
        const PlanArgs pl_loss = s.fused_dual ? s.pa : PlanArgs{};  // the fused pass has no softmax pass B to lend the planning a workgroup
        hipLaunchKernelGGL((k_loss<T>), dim3(c.gl + skl.nblocks + (pl_loss.plan ? 1 : 0)), dim3(BLOCK), skl.nblocks && c.lanczos ? (size_t)(WAVES_PER_BLOCK + 1) * c.Dpad * sizeof(double) : 0,
                           co.st, c.P, co.d_lrow.p, s.fused_dual ? yun.p : co.Y.p, wH.p, scal.p, co.lval.p, co.eta,
                           (const int*)(co.eng.use_blk && !mf_it ? co.bt.b_bpos.p : nullptr), co.bt.lval_blk.p,
                           (const T*)(c.xavg_deferred ? co.xval.p : nullptr), c.xavg_deferred ? co.xavg.p : (T*)nullptr, skl, c.Dpad,
                           (const int*)(co.eng.use_mfma ? co.bt.b_fpos.p : nullptr), co.bt.afrag.p, s.fused_dual ? co.Y.p : (T*)nullptr, co.yavg.p, s.acc, pl_loss,
                           s.rs_zeroed ? rsfx.p : (long long*)nullptr, s.rs_zeroed ? (s.first_it ? 2 * co.K : co.K) : 0, s.first_it ? 1 : 0,
                           s.first_it && pol.first_a16_guess ? co.bt.afrag16.p : (unsigned short*)nullptr);
        c.xavg_deferred = false;
        MMW_TRY(co.kt.end());
        MMW_TRY(co.pt.record(2, co.iter, co.st));
        return MMW_OK;
    }
    // ---- the sketch (unless it rode) and exp(L/2) applied to it
    int phase_expm(Core& co, ChunkRun& c, IterRun& s) {
        const bool sketch_rode = carry.drawn(c, co.iter);  // by this iteration's LOSS pass or the previous SDDMM launch: nothing to launch, nothing to time
        if (!sketch_rode) MMW_TRY(co.kt.begin(KT_SKETCH));
        if (c.randv) {
            MMW_TRY(copy_h2d(stage64.p, c.randv + (size_t)s.it * co.K * co.D, (size_t)co.K * co.D * sizeof(double), co.st));  // page-locked staging (runtime.h)
            hipLaunchKernelGGL((k_import_block<T>), dim3(grid_elems(co.eng.bs)), dim3(BLOCK), 0, co.st, co.K, co.D, c.Dpad, stage64.p, co.eng.start_block());
            co.eng.planes_ready[0] = false;  // an uploaded sketch is split by a pass of its own
            carry.uploaded();
        } else {
            if (!sketch_rode) MMW_TRY(launch_sketch(co, co.st, c.seed, (uint32_t)co.iter, s.first_it));
            co.eng.start_colsq_ready = c.lanczos;  // the Lanczos start norms come out of the sketch kernel
            co.eng.npart_start = sketch_rode ? carry.slabs : sketch_slabs(co);
            carry.used(c.seed);
        }
        if (!sketch_rode) MMW_TRY(co.kt.end());
        MMW_HIP(hipGetLastError());
        // X on the pattern runs on the matrix cores too when the exponential did: the combination then also writes y's planes
        co.eng.out_planes = nullptr;
        if constexpr (sizeof(T) == 4) {
            if (c.sd_mf_call) {
                if (xh_planes.n < 2 * co.eng.bs) MMW_TRY(xh_planes.alloc(2 * co.eng.bs));
                co.eng.out_planes = xh_planes.p;
            }
        }
        // inside a chunk only the SDDMM reads X_half; the chunk's last iteration leaves the fp32 copy the API hands out
        co.eng.planes_only = co.eng.out_planes != nullptr && c.optimistic && s.it + 1 < c.n && !co.sw.keep_xhalf;
        co.eng.rownorm_d = drow.p;  // the Lanczos combination also emits the row norms and the trace slabs
        co.eng.rownorm_part = tr_part.p;
        co.eng.plan_iter = pol.age(co.iter);
        if (s.first_it) {
            const size_t need = (size_t)co.eng.first_grid_max();
            if (tr1_part.n < need) {
                MMW_TRY(tr1_part.alloc(need));
                MMW_HIP(hipMemsetAsync(tr1_part.p, 0, need * sizeof(double), co.st));
            }
            MMW_TRY(co.eng.apply_first(co.eng.planes_only ? (T*)nullptr : co.Xh.p, 0.5, c.m_launch, s.lagged_it, xh_planes.p, rsfx.p + co.K, tr1_part.p, &s.ntr1,
                                    pol.first_a16_guess ? co.bt.afrag16.p : (const unsigned short*)nullptr));
            ++n_first_iters;
            if (pol.first_a16_guess) ++n_first16_iters;
        } else
            MMW_TRY(co.eng.apply(co.Xh.p, 0.5, c.m_launch, s.lagged_it));
        return MMW_OK;
    }
    // ---- X on the pattern from exp(L/2)R, and its running sum
    int phase_x(Core& co, ChunkRun& c, IterRun& s) {
        MMW_TRY(co.kt.begin(KT_SDDMM));
        if (!c.lanczos)
            hipLaunchKernelGGL((k_rownorm2<T>), dim3(c.gr), dim3(BLOCK), 0, co.st, co.K, c.Dpad, co.Xh.p, drow.p, tr_part.p);
        bool sd_done = false;
        c.rs_ok = false;
        if constexpr (sizeof(T) == 4) {
            if (c.sd_mf_call) {
                const SdMfmaDev SM = co.bt.sd_mfma_dev();
                const long long* dfx = s.first_it ? rsfx.p + co.K : nullptr;
                const double* trp = s.first_it ? tr1_part.p : tr_part.p;
                const int ntr = s.first_it ? s.ntr1 : c.gr;
                // the certificate of this iteration's first-order exponential rides in this launch (8 more columns of workgroups)
                FirstVerify fv_now;
                if (s.first_it) {
                    fv_now.plan = co.eng.plan_d.p; fv_now.viol = co.eng.viol_d.p; fv_now.o2 = co.eng.partial_o2.p; fv_now.n_o2 = co.eng.mf.nb;
                    fv_now.u2 = co.eng.partial_sq.p; fv_now.du2 = fv_measure ? co.eng.partial_du.p : nullptr; fv_now.rows = co.K; fv_now.n_u2 = co.eng.npart_start; fv_now.Dpad = c.Dpad;
                    fv_now.nwg = c.Dpad / FV_COLS;
                    fv_now.cA = pol.first_a16_guess ? F16_UNIT : F16_CA_TWO;
                    fv_now.du_scale = co.sw.fv_du_scale;
                }
                const bool fv_rides = s.first_it && co.sw.fv_in_sddmm;
                const dim3 grid((co.bt.HB.nbm() + 7) / 8 * 8 + (fv_rides ? 8 : 0), (co.bt.HB.m_ntile_max + SDM_GT - 1) / SDM_GT);
                long long* rs_out = s.rs_zeroed ? rsfx.p : nullptr;  // this iteration's LOSS pass zeroed the totals
                // MMW_SD_STAMPS=1 (developer aid): per-wave phase clocks of the last iteration's launch, printed to stderr
                StampBuf sdm_stamps;
                const size_t n_st = (size_t)grid.x * grid.y * 16 * 8;
                const bool want_st = s.it + 1 == c.n && live_switch(LIVE_SD_STAMPS);
                MMW_TRY(sdm_stamps.request(want_st, n_st, co.st));
                // two chunks resident per workgroup (three were built and measured 1 % slower)
                if (co.bt.HB.mfma_mt == 2) MMW_TRY((launch_sddmm_mfma<2, 2>(co, c, grid, SM, trp, ntr, s.acc, rs_out, dfx, sdm_stamps.p(), fv_rides ? fv_now : FirstVerify{})));
                else MMW_TRY((launch_sddmm_mfma<1, 2>(co, c, grid, SM, trp, ntr, s.acc, rs_out, dfx, sdm_stamps.p(), fv_rides ? fv_now : FirstVerify{})));
                if (want_st) MMW_TRY(dump_sddmm_stamps(co.st, sdm_stamps.p(), n_st, grid, co.bt.HB.mfma_mt));
                sd_done = true;
                // (MMW_FV_IN_SDDMM=0: certified by spare workgroups of the next iteration's DUAL phase, or by a launch of its own after the chunk's last)
                if (s.first_it && !fv_rides) c.fv_pending = fv_now;
                c.rs_ok = rs_out != nullptr;
            }
        }
        if (!sd_done && co.eng.use_blk) MMW_TRY(co.bt.ensure_sd(co.st, co.H, co.K, co.eng.lay.Dpad, co.sw.full_tile));
        if (sd_done) {
        } else if (co.bt.sddmm_blk2 && co.eng.use_blk) {
            StampBuf sd_stamps;  // MMW_SD_STAMPS=1: phase stamps of the last iteration's SDDMM
            MMW_TRY(sd_stamps.request(s.it + 1 == c.n && live_switch(LIVE_SD_STAMPS), (size_t)16 * 8192, co.st));
            const Sd2Dev S = co.bt.sd2_dev();
            constexpr int CT2 = B2_ROW_BYTES / (int)sizeof(T);
            const int per = (co.bt.sd2_nitems + 7) / 8;
            SketchArgs<T> sk{};
            const size_t sd_lds = std::max((size_t)co.bt.HB.un8_max * B2_ROW_BYTES, std::min((size_t)(SD2_THREADS / WAVE) * c.Dpad * sizeof(double), (size_t)65536));
            if (c.fuse_sketch && !c.randv && s.it + 1 < c.n && (size_t)(SD2_THREADS / WAVE) * c.Dpad * sizeof(double) <= sd_lds) {
                // the start block and its norm slabs are free once the combination has run: draw the next iteration's sketch here
                constexpr int VBW = SD2_THREADS / BLOCK;  // a workgroup here stands for this many of the stand-alone kernel's
                sk.nblocks = (sketch_slabs(co) + VBW - 1) / VBW;
                sk.K = co.K; sk.D = co.D; sk.seed = c.seed; sk.iter = (uint32_t)(co.iter + 1);
                sk.R = co.eng.start_block();
                sk.colsq_part = c.lanczos ? co.eng.partial_sq.p : nullptr;
                sk.planes = co.eng.start_planes();
                sk.planes_f16 = 0;
                co.eng.planes_ready[0] = sk.planes != nullptr;
                co.eng.planes0_f16 = false;
                carry.note((int64_t)co.iter + 1, c.seed, sk.nblocks * VBW);
            }
            hipLaunchKernelGGL((k_sddmm_blk2<T>), dim3(per * 8 + sk.nblocks), dim3(SD2_THREADS), sd_lds, co.st, co.blkdev(), S, c.P, c.Dpad,
                               (c.Dpad + CT2 - 1) / CT2, co.Xh.p, drow.p, tr_part.p, c.gr, co.xval.p, co.xavg.p, s.acc, sk, sd_stamps.p());
            if (sd_stamps.p()) MMW_TRY(dump_stamps(co.st, sd_stamps.p()));
        } else if (co.bt.sddmm_blk && co.eng.use_blk) {
            const SdDev S = co.bt.sd_dev();
            constexpr int CT = BLK_TILE_BYTES / (int)sizeof(T);
            const int ntiles = (c.Dpad + CT - 1) / CT;
            const int per = (co.bt.HB.nb() + 7) / 8;
            hipLaunchKernelGGL((k_sddmm_blk<T>), dim3(per * 8), dim3(BLK_THREADS), (size_t)BLK_UNION_ROWS * BLK_TILE_BYTES, co.st, co.blkdev(), S, c.P, c.Dpad,
                               ntiles, co.Xh.p, drow.p, tr_part.p, c.gr, co.xval.p, co.xavg.p, s.acc);
        } else
            switch (co.eng.lay.NCH) {
                case 1:
                    if ((co.eng.lay.LPR & (co.eng.lay.LPR - 1)) == 0) launch_sddmm<1>(co, c, s.acc);
                    else launch_sddmm<1, false>(co, c, s.acc);  // 40, 48, 56 lanes: no transposed reduction
                    break;
                case 2: launch_sddmm<2>(co, c, s.acc); break;
                case 3: launch_sddmm<3>(co, c, s.acc); break;
                default: launch_sddmm<4>(co, c, s.acc); break;
            }
        // the running sum of X (mmw.py:77-78): one coalesced pass; none of the SDDMM kernels read-modify-writes xavg
        if (sd_done) {  // the matrix-core SDDMM added X to its running sum itself (tile order)
        } else if (s.acc && s.it + 1 < c.n && !co.kt_exact()) c.xavg_deferred = true;  // the next iteration's LOSS pass adds it
        else if (s.acc) hipLaunchKernelGGL((k_accumulate<T>), dim3((unsigned)std::min<size_t>(((size_t)co.H.nnzL() + BLOCK - 1) / BLOCK, 4096)), dim3(BLOCK), 0, co.st, (size_t)co.H.nnzL(), co.xval.p, co.xavg.p);
        MMW_TRY(co.kt.end());
        MMW_HIP(hipGetLastError());
        MMW_TRY(co.pt.record(3, co.iter, co.st));
        return MMW_OK;
    }
    // ---- after the call's last iteration: the certificate and the lagged plan that no later iteration checks
    int chunk_tail(Core& co, ChunkRun& c) {
        if (c.fv_pending.plan) {  // the chunk's last first-order exponential
            hipLaunchKernelGGL(k_first_verify, dim3(c.fv_pending.nwg), dim3(BLOCK), 0, co.st, c.fv_pending);
            MMW_HIP(hipGetLastError());
        }
        if (c.optimistic && c.n > 1 && c.lag_chunk && c.lanczos) {
            // the chunk's last plan was extrapolated and no later plan of the chunk sees its matrix: check it here
            hipLaunchKernelGGL((k_rowsums<T>), dim3(co.eng.nwide), dim3(BLOCK), 0, co.st, co.K, co.d_indptr.p, co.d_col.p, co.lval.p, 0.5, co.eng.row_part.p);
            hipLaunchKernelGGL(k_plan_verify, dim3(1), dim3(PLAN_THREADS), 0, co.st, co.K, co.eng.row_part.p, co.eng.nwide, co.eng.plan_d.p, co.eng.viol_d.p, pol.age(co.iter) - 1);
            MMW_HIP(hipGetLastError());
        }
        // until settle() finds a violation or something touches the iterate.  A handle that has had to replay a chunk keeps restarting
        // its chunks exactly (measured on er-1pct, whose order rises during the run: 5 100 it/s so, 4 500 chained)
        pol.chain_ok = c.optimistic && c.n > 1 && pol.replays == 0 && !co.sw.no_chunk_chain;
        rs_last = c.rs_ok;
        return MMW_OK;
    }
};
}  // namespace
