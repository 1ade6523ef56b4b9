// The two records the solver handle (solver.h) keeps about work it enqueued without waiting for it: the chunk of iterations whose plans
// were not read back yet, with the snapshot it is run again from when the device refuses it, and the MMW_F_E_MAX reduction that rides
// behind a call.  Solver<T>::settle decides about the chunk; restore_pending is the discard path of both.
#pragma once
#include "solver_core.h"

namespace {
// An optimistic chunk (no per-iteration readback) and the device snapshot taken before it.
//   begin: a chunk is enqueued        clear: it is being settled, or a new run starts (its fields stay readable for the replay)
//   save / restore: the iterate (L, the live X pair, Y, the sums, e_accu) and the plan with its history, out of / back into the core
template <typename T> struct PendingChunk {
    DevBuf<T> sn_lval, sn_xval, sn_xavg, sn_Y, sn_yavg, sn_eaccu;
    DevBuf<ExpmPlan> sn_plan;  // plan (with its history) at the start of the pending chunk
    bool sn_tiles = false;     // which pair of buffers the snapshot of X was taken from
    bool live = false;
    int iter0 = 0, n = 0;
    size_t events0 = 0;  // phase-timer events recorded before the pending chunk (PhaseTimers::mark)
    uint64_t seed = 0;
    void begin(int iter0_, int n_, uint64_t seed_, size_t events0_) { live = true; iter0 = iter0_; n = n_; seed = seed_; events0 = events0_; }
    void clear() { live = false; }
    int copy_state(SolverCore<T>& co, bool save) {
        const size_t nnz = (size_t)co.H.nnzL(), C = (size_t)co.H.C();
        if (save) sn_tiles = co.x.tiles;
        else co.x.tiles = sn_tiles;  // the snapshot goes back into the buffers it was taken from
        const typename XLayout<T>::Pair xl = co.x.live(co);
        DevBuf<T>* snap[6] = {&sn_lval, &sn_xval, &sn_xavg, &sn_Y, &sn_yavg, &sn_eaccu};
        DevBuf<T>* cur[6] = {&co.lval, xl.val, xl.avg, &co.Y, &co.yavg, &co.e_accu};
        const size_t len[6] = {nnz, xl.n, xl.n, C, C, C};
        CopySet<T> cs;
        for (int i = 0; i < 6; ++i) {
            if (snap[i]->n < len[i]) MMW_TRY(snap[i]->alloc(len[i]));
            cs.dst[i] = save ? snap[i]->p : cur[i]->p;
            cs.src[i] = save ? cur[i]->p : snap[i]->p;
            cs.n[i] = len[i];
        }
        if (sn_plan.n < 1) MMW_TRY(sn_plan.alloc(1));
        cs.plan_dst = save ? sn_plan.p : co.eng.plan_d.p;
        cs.plan_src = save ? co.eng.plan_d.p : sn_plan.p;
        hipLaunchKernelGGL((k_copy_state<T>), dim3(256, 6), dim3(BLOCK), 0, co.st, cs);  // one launch instead of seven copies
        MMW_HIP(hipGetLastError());
        if (!save && co.bt.lval_blk.p) co.lblk_stale = true;  // rebuilt from the restored values when the fp32 kernel next needs it
        if (!save && co.bt.afrag.p) {  // the fragment image follows the restored values
            hipLaunchKernelGGL((k_refrag<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, co.st, nnz, co.lval.p, co.bt.b_fpos.p, co.bt.afrag.p);
            MMW_HIP(hipGetLastError());
        }
        return MMW_OK;
    }
    int save(SolverCore<T>& co) { return copy_state(co, true); }
    int restore(SolverCore<T>& co) { return copy_state(co, false); }
};
// The objective record's one number -- the largest violation of the last iteration (MMW_F_E_MAX) -- is reduced right behind the call's
// work and copied out by the mmw_sync that waits for it anyway: reading it afterwards is free (its launch + copy + wait were a third
// of what a 20-step timed region spends on its record).  A replay of the last chunk changes `iter` back and forth but ends at the same
// e_this only after re-running, so the value is tied to the iteration count AND dropped whenever a chunk is discarded: `drop` is the one
// place that invalidates it (a new run, a discarded chunk).
struct EmaxRecord {
    DevBuf<double> d;
    double h = 0.0;
    int enq_iter = -1, got_iter = -1;  // iteration count the enqueued / fetched maximum violation belongs to
    template <typename T> int enqueue(SolverCore<T>& co) {
        if (co.iter <= 0) return MMW_OK;
        if (!d.p) MMW_TRY(d.alloc(1));
        hipLaunchKernelGGL((k_max_of<T>), dim3(1), dim3(1024), 0, co.st, (size_t)co.H.C(), co.e_this.p, d.p);
        MMW_HIP(hipGetLastError());
        enq_iter = co.iter;
        got_iter = -1;
        return MMW_OK;
    }
    // mmw_sync's wait for the stream, with the copy of a value enqueued for this iteration count in front of it
    template <typename T> int fetch_at_sync(SolverCore<T>& co) {
        const bool want = enq_iter == co.iter && got_iter != co.iter && d.p != nullptr;
        if (want) MMW_HIP(hipMemcpyAsync(&h, d.p, sizeof(double), hipMemcpyDeviceToHost, co.st));
        MMW_HIP(hipStreamSynchronize(co.st));
        if (want) got_iter = co.iter;
        return MMW_OK;
    }
    void drop() { enq_iter = got_iter = -1; }
    bool value_if_current(int iter, double* out) const {
        if (got_iter != iter || got_iter < 0) return false;
        *out = h;
        return true;
    }
};
}  // namespace
