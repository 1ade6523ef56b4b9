// A change of slot counts on the device (mmw_batch_set_slots, mmw_batch_set_slots_warm): the fp64 arena is packed, so a new
// D = Z * rank_radio of one instance moves the offsets of every later one.  k_batch_relayout writes every instance of the NEW arena
// from the OLD one, one workgroup per instance, in the batch's idiom: no atomics, nothing waits across workgroups, plain copies and
// fills in a fixed order.  The two arenas are different allocations (batch_core.h keeps two and swaps them after the launch); the
// int32 arena never changes and is read for the diagonal positions only.
//
//   pattern data (sab / sba, h_max, S_sum)   copied old -> new: they do not depend on Z
//   1 / norm_H, cH                           placed from the call's upload: update_slots (pattern.h) computes them on the host, so
//                                            their bits are the ones mmw_batch_create uploads
//   RELAYOUT_COLD                            the reference's initial point (mmw.py:62-73) as BatchCore::reset_one writes it: everything
//                                            from lval to info zero, X = I on the pattern, Y = y0 (1.0 / (double)C, divided on the host)
//   RELAYOUT_WARM                            lval, xval, Y and e_accu from the old offsets; the sums, e_this, the per-row scalars, the
//                                            K x D blocks and info zero.  Iteration i adds X_i / Y_i to the sums when it starts, so
//                                            after n warm iterations they hold the kept X / Y and n - 1 new terms: the n terms a
//                                            handle holds after sums_from_current and n iterations.
//   RELAYOUT_OUT                             the instance sits out of a warm call: every array from lval to info copied as it is (its
//                                            D did not change), so a later warm call can pick it up
#pragma once
#include "kernels_batch.h"

namespace mmw {

enum { RELAYOUT_OUT = 0, RELAYOUT_COLD = 1, RELAYOUT_WARM = 2 };

struct RelayoutItem {
    int mode, pad0;
    int64_t o_scal;  // the instance's K values in each of the call's two scalar arrays
    double y0;       // Y of the initial point
};

__device__ __forceinline__ void relayout_copy(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
    for (int64_t i = threadIdx.x; i < n; i += BATCH_THREADS) dst[i] = src[i];
}
__device__ __forceinline__ void relayout_fill(double* __restrict__ dst, int64_t n, double v) {
    for (int64_t i = threadIdx.x; i < n; i += BATCH_THREADS) dst[i] = v;
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_relayout(const BatchDesc* __restrict__ odescs, const BatchDesc* __restrict__ ndescs,
                                                                  const RelayoutItem* __restrict__ items, const double* __restrict__ invn,
                                                                  const double* __restrict__ cH, const int* __restrict__ ia,
                                                                  const double* __restrict__ fo, double* __restrict__ fn) {
    const BatchDesc& o = odescs[blockIdx.x];
    const BatchDesc& d = ndescs[blockIdx.x];
    const RelayoutItem& t = items[blockIdx.x];
    const int64_t K = d.K, nnz = d.nnzL, C = d.C;
    relayout_copy(fn + d.o_sab, fo + o.o_sab, 2 * nnz);
    relayout_copy(fn + d.o_hmax, fo + o.o_hmax, K);
    relayout_copy(fn + d.o_ssum, fo + o.o_ssum, K);
    relayout_copy(fn + d.o_invn, invn + t.o_scal, K);
    relayout_copy(fn + d.o_cH, cH + t.o_scal, K);
    if (t.mode == RELAYOUT_OUT) {  // same sizes, so the same span relative to lval
        relayout_copy(fn + d.o_lval, fo + o.o_lval, d.o_info + 4 - d.o_lval);
        return;
    }
    relayout_fill(fn + d.o_lval, d.o_info + 4 - d.o_lval, 0.0);
    __syncthreads();  // the values below land in the span just cleared
    if (t.mode == RELAYOUT_COLD) {
        const int* __restrict__ diag = ia + d.o_diag;
        for (int k = threadIdx.x; k < d.K; k += BATCH_THREADS) fn[d.o_xval + diag[k]] = 1.0;
        relayout_fill(fn + d.o_Y, C, t.y0);
    } else {
        relayout_copy(fn + d.o_lval, fo + o.o_lval, nnz);
        relayout_copy(fn + d.o_xval, fo + o.o_xval, nnz);
        relayout_copy(fn + d.o_Y, fo + o.o_Y, C);
        relayout_copy(fn + d.o_eaccu, fo + o.o_eaccu, C);
    }
}

}  // namespace mmw
