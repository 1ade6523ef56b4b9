// The spectral baseline on a solver handle (mmw_factor_spectral; sdp_solver.spectral_sdp_solver, sim_src/alg/sdp_solver.py:165-185):
//   k_lap_fill       the Laplacian of S_gain + S_gain^T as a second value vector on the handle's L pattern, fp64.  The pattern
//                    (pattern.h: diag + sym(pattern(S_T')) + pattern(Q)) holds every off-diagonal non-zero of S + S^T: an entry of S
//                    either survives into S_T' or its transpose lies in nz(Q).  One wavefront per row: each lane looks its entry's two
//                    values up in the rounding side's S_gain (so_*: no diagonal, no stored zeros, rows sorted) by binary search and
//                    writes -(a + b); a + b is commutative, so the mirror entry gets the same bits, and an entry that is in the
//                    pattern through Q alone gets a zero.  The diagonal is the row's degree, summed in ascending column order by a
//                    chain every lane runs alike (the lanes' values broadcast one by one): nothing depends on the launch geometry, no atomics, and
//                    lap_row below -- what a device -1 handle runs in a plain loop -- states the same sum with the same lap_pair.
//   k_lap_narrow     the values in the handle's T for the factor's products.
//   k_export_eigvec  one wavefront per user: the user's row of V[:, top Z] in ascending eigenvalue (eigsh's order), its norm by the
//                    fixed-order wave reduction, the norm stored, the row divided by it (a row of norm exactly 0 stays 0) and, in
//                    index order, the quotient times 1 - k 2^-32 -- divide, then multiply, each rounded: rand_sdp_solver.index_ordered
//                    of the plain block, bit for bit.
#pragma once
#include "device_utils.h"
#include "pattern_csr_device.h"

namespace mmw {

// S[r, c] + S[c, r] from the sorted rows of S_gain without its diagonal and stored zeros (0 where an entry is absent)
__host__ __device__ inline double lap_pair(const int* so_ptr, const int* so_idx, const double* so_val, int r, int c) {
    double a = 0.0, b = 0.0;
    const int wa = csr_lower(so_idx, so_ptr[r], so_ptr[r + 1], c);
    if (wa < so_ptr[r + 1] && so_idx[wa] == c) a = so_val[wa];
    const int wb = csr_lower(so_idx, so_ptr[c], so_ptr[c + 1], r);
    if (wb < so_ptr[c + 1] && so_idx[wb] == r) b = so_val[wb];
    return a + b;
}
// row r of the Laplacian on the L pattern, sequentially (device -1; the kernel below spreads the entries over a wave and runs the same sum)
inline void lap_row(const int* l_ptr, const int* l_idx, const int* so_ptr, const int* so_idx, const double* so_val, int r, double* lap) {
    double deg = 0.0;
    int dpos = -1;
    for (int e = l_ptr[r]; e < l_ptr[r + 1]; ++e) {
        const int c = l_idx[e];
        if (c == r) {
            dpos = e;
            continue;
        }
        const double w = lap_pair(so_ptr, so_idx, so_val, r, c);
        lap[e] = -w;
        deg += w;
    }
    if (dpos >= 0) lap[dpos] = deg;
}

__global__ __launch_bounds__(BLOCK) void k_lap_fill(int K, const int* __restrict__ l_ptr, const int* __restrict__ l_idx, const int* __restrict__ diag_pos,
                                                  const int* __restrict__ so_ptr, const int* __restrict__ so_idx, const double* __restrict__ so_val,
                                                  double* __restrict__ lap) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int r = blockIdx.x * WAVES_PER_BLOCK + wib; r < K; r += gridDim.x * WAVES_PER_BLOCK) {
        const int e0 = l_ptr[r], e1 = l_ptr[r + 1];
        double deg = 0.0;
        for (int base = e0; base < e1; base += WAVE) {  // (wave-uniform bounds: every lane reaches the readlanes below)
            const int e = base + lane;
            const bool off = e < e1 && l_idx[e] != r;
            double w = 0.0;
            if (off) {
                w = lap_pair(so_ptr, so_idx, so_val, r, l_idx[e]);
                lap[e] = -w;
            }
            const unsigned long long offs = __ballot(off);
            const int live = min(WAVE, e1 - base);
            for (int l = 0; l < live; ++l) {
                const double wl = __shfl(w, l);
                if ((offs >> l) & 1ull) deg += wl;
            }
        }
        if (lane == 0) lap[diag_pos[r]] = deg;
    }
}

template <typename T> __global__ __launch_bounds__(BLOCK) void k_lap_narrow(size_t n, const double* __restrict__ a, T* __restrict__ b) {
    for (size_t o = (size_t)blockIdx.x * BLOCK + threadIdx.x; o < n; o += (size_t)gridDim.x * BLOCK) b[o] = (T)a[o];
}

// out[k, c] = V[k, Z - 1 - c] / ||V[k, 0..Z)|| (x (1 - k 2^-32) in index order); V's columns are in descending eigenvalue
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_export_eigvec(int K, int Z, int ld, const T* __restrict__ V, int index_order, double* __restrict__ rownorm,
                                                       double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int k = blockIdx.x * WAVES_PER_BLOCK + wib; k < K; k += gridDim.x * WAVES_PER_BLOCK) {
        const T* row = V + (size_t)k * ld;
        double s = 0.0;
        for (int c = lane; c < Z; c += WAVE) {
            const double x = (double)row[Z - 1 - c];
            s += x * x;
        }
        const double nrm = sqrt(wave_sum(s));
        if (lane == 0) rownorm[k] = nrm;
        const double f = 1.0 - (double)k * 0x1p-32;
        for (int c = lane; c < Z; c += WAVE) {
            double q = 0.0;
            if (nrm > 0.0) q = (double)row[Z - 1 - c] / nrm;
            if (index_order) q = q * f;
            out[(size_t)k * Z + c] = q;
        }
    }
}

}  // namespace mmw
