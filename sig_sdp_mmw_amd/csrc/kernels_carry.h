// The iterate of one solver handle taken over by a handle on another state of the same users (mmw_carry, solver_carry.h): the stations
// have moved, the destination's L / X pattern and its association pairs differ from the source's, and (L, X, Y, e_accu) are re-indexed.
// The rule is the batch's (kernels_batch_carry.h): an entry (row, col) the source's pattern does not store is 0, the D- and the H-part of
// the constraint vector [D-part K | F-part E_asso | H-part K] carry by user, the F-part by pair, 0 for a pair the source lacks, and Y is
// not renormalised.  Unlike the batch no index map is made on the host and uploaded: at the benchmark's size that would be 1.4 M merged
// entries per time point, and a handle built on the device has no host lists to merge.  The two patterns are matched here, on the
// device, inside the pass that gathers; mmw_carry_map (the host merge, pattern.h) states the same maps for the tests.
//
// k_carry_rows: one wavefront per row of the DESTINATION's pattern (grid_rows), lanes over the row's entries, looping for rows longer
// than 64.  Each lane looks its column up in the source's row by binary search: both rows are ascending, a source row is a few hundred
// bytes that the wave's first probes pull into cache, and the search's trip count is uniform enough (log2 of one row length) that the
// lanes diverge only at its last step.  It writes lval, xval and xavg (= xval: the handle's warm convention, SolverCore::sums_from_current)
// in CSR order.  The F-part rides on the same pass: the upper entry of a pair (col > row, the entry asso_pos names) also writes the
// pair's Y, yavg (= Y) and e_accu from the source's pair pid_src[m] of the matched entry m -- 0 when the entry is absent, and 0 as well
// when the source stores it as a plain GAIN entry (pid_src[m] < 0): L and X then carry a value while the pair's constraint did not
// exist.  Lane 0 of a row's wave copies the user's D- and H-part entries; the H-part sits behind each side's own E_asso.
// One writer per address, no atomics, nothing waits across workgroups; every index is bounded by the row pointers of its own side.
#pragma once
#include "device_utils.h"

namespace mmw {

template <typename T> struct CarrySrc {
    const int* indptr; const int* col; const int* pid;
    const T* lval; const T* xval; const T* Y; const T* e_accu;
    int E_asso;
};
template <typename T> struct CarryDst {
    const int* indptr; const int* col; const int* pid;
    T* lval; T* xval; T* xavg; T* Y; T* yavg; T* e_accu;
    int E_asso;
};

template <typename T> __global__ __launch_bounds__(BLOCK) void k_carry_rows(int K, CarrySrc<T> S, CarryDst<T> D) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int row = blockIdx.x * WAVES_PER_BLOCK + wib; row < K; row += gridDim.x * WAVES_PER_BLOCK) {
        const int s0 = S.indptr[row], s1 = S.indptr[row + 1];
        for (int e = D.indptr[row] + lane; e < D.indptr[row + 1]; e += WAVE) {
            const int c = D.col[e];
            int lo = s0, hi = s1;
            while (lo < hi) {  // first source entry of the row with column >= c
                const int mid = (lo + hi) >> 1;
                if (S.col[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            const bool hit = lo < s1 && S.col[lo] == c;
            const T l = hit ? S.lval[lo] : T(0), x = hit ? S.xval[lo] : T(0);
            D.lval[e] = l;
            D.xval[e] = x;
            D.xavg[e] = x;
            const int j = D.pid[e];
            if (j >= 0 && c > row) {  // the pair's upper entry writes the pair
                const int js = hit ? S.pid[lo] : -1;
                const T y = js >= 0 ? S.Y[K + js] : T(0), a = js >= 0 ? S.e_accu[K + js] : T(0);
                D.Y[K + j] = y;
                D.yavg[K + j] = y;
                D.e_accu[K + j] = a;
            }
        }
        if (lane == 0) {
            const int hs = K + S.E_asso + row, hd = K + D.E_asso + row;
            const T yd = S.Y[row], yh = S.Y[hs];
            D.Y[row] = yd; D.yavg[row] = yd; D.e_accu[row] = S.e_accu[row];
            D.Y[hd] = yh; D.yavg[hd] = yh; D.e_accu[hd] = S.e_accu[hs];
        }
    }
}

}  // namespace mmw
