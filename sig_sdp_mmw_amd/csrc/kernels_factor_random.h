// The random embedding as a solver handle's resident factor (mmw_factor_random; rand_sdp_solver.run_with_state,
// sim_src/alg/sdp_solver.py:109-114): K x cols standard normals, every row divided by its norm, float64 whatever the handle's dtype.
// The draw is the sketch's ("The generator as a contract"): row r, group p holds the columns 2p and 2p + 1, from
// Philox4x32-10 with counter (r, p, 0, "MMWS") under the key (seed low word, seed high word), fp64 Box-Muller.  So the block is the fp64
// sketch of (seed, iteration 0): bitwise what sketch_rows<double> (kernels_loop.h) writes for D = cols <= 512 and what
// batch_sketch_rows (kernels_batch.h) leaves for mmw_batch_factor_random -- lane l of the row's wavefront takes the groups l + 64 i,
// i ascending, adds the squares of what it drew in that order (a column >= cols counts as 0), and the 64 partial sums meet in the same
// wave reduction.  Past 512 columns the rule simply goes on with i = 4, 5, ...: the sketch's four passes belong to the loop's LDS
// layout, which this kernel does not have.
//
// k_factor_random: one wavefront per row (grid_rows), grid-stride over the rows.  A lane writes what it drew as it draws it and, once
// the row's norm is known, scales ITS OWN entries in place (x 1/norm, then x (1 - row 2^-32) in index order: the two roundings of
// rand_sdp_solver.index_ordered applied to the normalised block) -- no lane reads what another wrote, so nothing has to be made
// visible in between and the width is not bounded by registers.  One writer per address, no atomics, no LDS, nothing waits across
// workgroups; every index is row * cols + c with row < K and c < cols.
#pragma once
#include "device_utils.h"

namespace mmw {

__global__ __launch_bounds__(BLOCK) void k_factor_random(int K, int cols, uint64_t seed, int index_order, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int ngroups = (cols + 1) >> 1;
    for (int row = blockIdx.x * WAVES_PER_BLOCK + wib; row < K; row += gridDim.x * WAVES_PER_BLOCK) {
        double* r = out + (size_t)row * cols;
        double ssl = 0.0;
        for (int p = lane; p < ngroups; p += WAVE) {
            uint32_t w[4];
            philox4x32_10((uint32_t)row, (uint32_t)p, 0u, 0x4d4d5753u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
            double n[2];
            box_muller(w, n[0], n[1]);
            if (p * 2 + 1 >= cols) n[1] = 0.0;  // (p < ngroups: column 2p exists)
            // The sum of squares with its roundings spelled out, because bits hang on them: the sketch's unrolled first pass starts
            // from 0 and compiles to fma(n0, n0, n1 * n1) -- the second square rounded, the first fused --, its later passes add
            // square by square, fused: fma(n1, n1, fma(n0, n0, sum)).  A loop-carried sum would make the first pass fuse the other way round
            // and differ from mmw_sketch / mmw_batch_factor_random in the last bit of about one row in thirty.
            if (p == lane) ssl = fma(n[0], n[0], __dmul_rn(n[1], n[1]));
            else ssl = fma(n[1], n[1], fma(n[0], n[0], ssl));
            r[2 * p] = n[0];
            if (2 * p + 1 < cols) r[2 * p + 1] = n[1];
        }
        const double ss = wave_sum(ssl);  // (all 64 lanes are back here: the loop above is the only divergence)
        const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
        const double f = 1.0 - (double)row * 0x1p-32;
        for (int p = lane; p < ngroups; p += WAVE) {
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                if (p * 2 + v < cols) {
                    double q = r[2 * p + v] * inv;
                    if (index_order) q = q * f;
                    r[2 * p + v] = q;
                }
            }
        }
    }
}

}  // namespace mmw
