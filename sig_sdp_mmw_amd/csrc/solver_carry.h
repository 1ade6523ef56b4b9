// mmw_carry / mmw_carry_map of the solver handle (solver.h): the iterate of a handle that has iterated on the state before the stations
// moved, taken over by a handle on the state after, which has not.  Three concerns, in the order Solver<T>::carry goes through them:
//   carry_refusal   every refusal, before either handle is touched (CarryInfo is what a handle of either dtype says about itself)
//   SolverCarry     the gather on the device (kernels_carry.h), the destination's derived copies of the iterate (X's tile order, L's
//                   traversal-order and fragment images), and the run history mmw_set_slots_warm would have kept on the source
//   CarriedPlan     the source's last plan, which plans the destination's first chunk
// The source is read only: it is settled, its X is given a CSR view (a scratch copy while the iterate lives in tile order) and its stream
// is waited for; after the call it reads the same and continues the same.  Ordering: the source's stream is synchronised before the
// gather is launched and the destination's before mmw_carry returns, so when the call is back nothing reads the source any more -- it
// may be iterated, reset or destroyed at once -- and the destination holds the carried values.
#pragma once
#include "kernels_carry.h"
#include "solver_loop.h"
#include "solver_replay.h"

namespace {
struct CarryInfo {
    bool host_only; int device, dtype, K, iter;
};
inline int carry_refusal(const std::string& who, const CarryInfo& d, const CarryInfo& s, bool on_device) {
    if (on_device) {
        if (d.host_only || s.host_only) return fail(MMW_ERR_STATE, who + ": host-only handle (created with device -1)");
        if (d.device != s.device) return fail(MMW_ERR_ARG, who + ": the source lives on device " + std::to_string(s.device) + ", this handle on device " + std::to_string(d.device));
        if (d.dtype != s.dtype) return fail(MMW_ERR_ARG, who + ": the source is an " + (s.dtype == MMW_F32 ? "fp32" : "fp64") + " handle, this one " + (d.dtype == MMW_F32 ? "fp32" : "fp64"));
    }
    if (d.K != s.K)
        return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(d.K) + " here, K = " + std::to_string(s.K) + " in the source (a carry keeps the users and moves them)");
    if (on_device && d.iter != 0) return fail(MMW_ERR_STATE, who + ": this handle has run " + std::to_string(d.iter) + " iterations (carry into a handle that has not iterated)");
    return MMW_OK;
}
// The plan the destination's first chunk is planned on (ChunkPolicy::chunk_length / plan_chunk): the source's last one, as the first chunk
// after mmw_set_slots_warm is planned on the previous probe's.  It is kept beside the engine's `last`, which stays the record of the
// destination's own exponentials (MMW_F_EXPM_INFO: none yet), and is dropped by the first iterations enqueued and by every new run.
struct CarriedPlan {
    ExpmPlan plan{};
    bool live = false;
    const ExpmPlan& or_last(const ExpmPlan& last) const { return live ? plan : last; }
    void drop() { live = false; }
};
template <typename T> struct SolverCarry {
    using Core = SolverCore<T>;
    // (L, X, Y, e_accu) of `s` re-indexed onto `d`'s pattern, with the sums in the handle's warm convention (xavg = xval, yavg = Y); on d's
    // stream, which the caller (Solver<T>::carry) waits for before it hands `s` back
    static int gather(Core& d, Core& s) {
        CarrySrc<T> S{s.d_indptr.p, s.d_col.p, s.d_pid.p, s.lval.p, s.xval.p, s.Y.p, s.e_accu.p, (int)s.H.E_asso()};
        CarryDst<T> D{d.d_indptr.p, d.d_col.p, d.d_pid.p, d.lval.p, d.xval.p, d.xavg.p, d.Y.p, d.yavg.p, d.e_accu.p, (int)d.H.E_asso()};
        hipLaunchKernelGGL((k_carry_rows<T>), dim3(grid_rows(d.K)), dim3(BLOCK), 0, d.st, d.K, S, D);
        MMW_HIP(hipGetLastError());
        d.pt.clear_samples();
        return MMW_OK;
    }
    // What the handle derives from the iterate follows the carried values: X is in CSR order (the first matrix-core SDDMM call moves it),
    // L's traversal-order image is rebuilt when the fp32 kernel next needs it, the fragment image now, as after a snapshot restore.
    // bt.afrag16 needs nothing: it is read only by a first-order product whose own iteration's LOSS pass has just rewritten every word
    // that is not a hole (kernels_loop.h, k_loss), and the holes are zero since creation.
    static int derived(Core& d) {
        d.x.tiles = false;
        if (d.bt.lval_blk.p) d.lblk_stale = true;
        if (d.bt.afrag.p) {
            const size_t nnz = (size_t)d.H.nnzL();
            hipLaunchKernelGGL((k_refrag<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, d.st, nnz, d.lval.p, d.bt.b_fpos.p, d.bt.afrag.p);
            MMW_HIP(hipGetLastError());
        }
        return MMW_OK;
    }
    // The run history: what mmw_set_slots_warm keeps on one handle moves from `s` to `d` -- the policy's fields, warm-restarted at the
    // source's iteration count, the last plan and what it said about the matrix-core split.  The device plan record needs no copy: a
    // slot change zeroes it (ExpmEngine::resize) before k_plan_reset(keep) runs, and d's is as zero as that since its creation.
    static int history(Core& d, SolverLoop<T>& dl, CarriedPlan& dplan, const Core& s, const SolverLoop<T>& sl) {
        dl.pol = sl.pol;
        dl.pol.on_warm_restart(s.iter);
        dplan.plan = s.eng.last;
        dplan.live = true;
        d.eng.last_mfma_ok = s.eng.last_mfma_ok;
        if (d.eng.viol_d.p) MMW_TRY(d.eng.clear_violation());
        return d.eng.reset_plan_history(true);
    }
};
}  // namespace
