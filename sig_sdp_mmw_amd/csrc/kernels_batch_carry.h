// The iterate of one batch taken over into another batch on other states (mmw_batch_carry): the stations have moved, so the new
// batch's L / X pattern and its association pairs differ from the old one's, and (e_accu, L, X, Y) are re-indexed, not copied.
// k_batch_carry writes the four arrays of every taking instance of the NEW batch's fp64 arena from the OLD batch's, one workgroup per
// taking instance, in the batch's idiom: no atomics, nothing waits across workgroups, one writer per address, plain gathers and
// fills in a fixed order.  The two arenas belong to two batches and are different allocations.
//
//   lmap[nnzL_new]   position in the old L / X value arrays of the new pattern's entry (row, col), -1 where the old pattern does not
//                    store it.  The diagonal is in both patterns, so X's diagonal always carries.
//   cmap[C_new]      position in the old constraint vector [D-part K | F-part E_asso | H-part K]: the D- and the H-part by user
//                    index (K is the same on both sides), the F-part by pair (asso_x, asso_y), -1 for a pair the old state lacks.
//   -1               reads as 0.0: an entry of L that did not exist has accumulated no loss, an X entry outside the old pattern
//                    was never sampled, a constraint that did not exist has accumulated no violation and carries no weight.
//
// Both maps are computed on the host by merging sorted rows (carry_maps in pattern.h) and arrive in the call's upload.
// Y is NOT renormalised: with pairs lost or gained its sum is no longer 1.  The first iteration's softmax rewrites Y from e_accu;
// before that only the first term of the running sum of Y and the first row of the gap log read it.
// Everything else of the new instance stays as its creation left it (sums, e_this, the per-row scalars, the K x D blocks and the
// info record zero), which is what RELAYOUT_WARM (kernels_batch_relayout.h) leaves too.
#pragma once
#include "kernels_batch.h"

namespace mmw {

struct CarryItem {
    int64_t o_lmap, o_cmap;  // the instance's two maps in the call's int32 map array
};

__device__ __forceinline__ void carry_gather(double* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ map, int64_t n) {
    for (int64_t i = threadIdx.x; i < n; i += BATCH_THREADS) {
        const int m = map[i];
        dst[i] = m < 0 ? 0.0 : src[m];
    }
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_carry(const BatchDesc* __restrict__ sdescs, const BatchDesc* __restrict__ ddescs,
                                                               const CarryItem* __restrict__ items, const int* __restrict__ maps,
                                                               const double* __restrict__ fs, double* __restrict__ fd) {
    const BatchDesc& s = sdescs[blockIdx.x];
    const BatchDesc& d = ddescs[blockIdx.x];
    const CarryItem& t = items[blockIdx.x];
    const int* __restrict__ lmap = maps + t.o_lmap;
    const int* __restrict__ cmap = maps + t.o_cmap;
    carry_gather(fd + d.o_lval, fs + s.o_lval, lmap, d.nnzL);
    carry_gather(fd + d.o_xval, fs + s.o_xval, lmap, d.nnzL);
    carry_gather(fd + d.o_Y, fs + s.o_Y, cmap, d.C);
    carry_gather(fd + d.o_eaccu, fs + s.o_eaccu, cmap, d.C);
}

}  // namespace mmw
