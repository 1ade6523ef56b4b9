// The rounding's own draws and its choice among attempts, on the device (mmw_round_attempts, include/mmw_hip.h): the Z x D' directions
// of attempt a from Philox keyed by (seed, a) -- the one statement of that draw, shared with the batch (k_batch_round, k_batch_randv:
// kernels_batch_epilogue.h) -- and the rule of sdp_solver.rounding (sim_src/alg/sdp_solver.py:18-25) applied to the attempts'
// counts of users left over, so that only the winner's slots cross to the host.
#pragma once
#include "device_utils.h"

namespace mmw {

// randv row `row` of (seed, attempt) (sdp_solver.py:48-49), by one wavefront: lane l draws the column pairs l + 64 i from the counter
// (row, pair, attempt, "RNDV") under the key (seed low word, seed high word); the squared norm per lane in ascending pair, then the
// fixed-order wave reduction; every lane scales what it drew.  `r` is the row's D' doubles; all 64 lanes of the wave must call.
__device__ __forceinline__ void randv_row(int row, int Dp, uint64_t seed, uint32_t attempt, int lane, double* r) {
    const int ngroups = (Dp + 1) >> 1;
    double ssl = 0.0;
    for (int p = lane; p < ngroups; p += WAVE) {
        uint32_t w[4];
        philox4x32_10((uint32_t)row, (uint32_t)p, attempt, 0x524e4456u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        double n0, n1;
        box_muller(w, n0, n1);
        ssl += n0 * n0;
        r[2 * p] = n0;
        if (2 * p + 1 < Dp) {
            ssl += n1 * n1;
            r[2 * p + 1] = n1;
        }
    }
    const double ss = wave_sum(ssl);
    const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
    for (int p = lane; p < ngroups; p += WAVE) {
        r[2 * p] *= inv;
        if (2 * p + 1 < Dp) r[2 * p + 1] *= inv;
    }
}

// ---- randv[nattempt][Z][D'] of (seed, attempt0 + a): one wavefront per (attempt, row), grid = ceil(nattempt Z / 4) workgroups of four
// waves (1 860 waves at Z = 186 x 10 attempts: seven per CU).  One writer per address, no LDS beyond the wave sum's, no atomics.
__global__ __launch_bounds__(BLOCK) void k_round_randv(int Z, int Dp, int nattempt, uint64_t seed, uint32_t attempt0, double* __restrict__ R) {
    const int lane = (int)threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * WAVES_PER_BLOCK + ((int)threadIdx.x >> 6);  // (wave-uniform)
    if (w >= (long long)nattempt * Z) return;
    const int a = (int)(w / Z), row = (int)(w % Z);
    randv_row(row, Dp, seed, attempt0 + (uint32_t)a, lane, R + (size_t)w * Dp);
}

// ---- the attempt a rounding call returns (sdp_solver.py:18-25), one launch after k_greedy_b.  rule 0, the reference's: the lowest
// attempt that left nobody over, else the last one.  rule 1 (not the reference's): the attempt with the fewest users left over, ties to
// the lower attempt.  Every workgroup derives the pick itself from the nattempt <= ROUND_MAX_ATTEMPTS counts -- nothing waits across
// workgroups -- and copies its stretch of that attempt's K slots (-1 = left over) to `win`; workgroup 0 writes {pick, rem[pick]}.
constexpr int ROUND_MAX_ATTEMPTS = 256;
constexpr int ROUND_PICK_MAX_K = (1 << 23) - 1;  // rule 1's key rem * ROUND_MAX_ATTEMPTS + a stays an int (the entries refuse a larger K)
static_assert(BLOCK >= ROUND_MAX_ATTEMPTS, "k_round_pick holds one attempt per thread of a workgroup");
static_assert((long long)ROUND_PICK_MAX_K * ROUND_MAX_ATTEMPTS + ROUND_MAX_ATTEMPTS - 1 <= 0x7fffffffLL, "k_round_pick's rule 1 key is an int");
__global__ __launch_bounds__(BLOCK) void k_round_pick(int K, int nattempt, int rule, const int* __restrict__ rem, const int* __restrict__ slot,
                                                      int* __restrict__ win, int* __restrict__ info) {
    __shared__ int key_w[WAVES_PER_BLOCK];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // one attempt per thread (BLOCK = ROUND_MAX_ATTEMPTS): the smallest key wins, and the keys are distinct
    //   rule 0: a feasible attempt a has key a, an infeasible one nattempt + (nattempt - 1 - a): the last attempt is the first of those
    //   rule 1: key = rem * ROUND_MAX_ATTEMPTS + a (rem <= K < 2^23)
    int key = 0x7fffffff;
    if (tid < nattempt) {
        const int r = rem[tid];
        key = rule == 0 ? (r == 0 ? tid : 2 * nattempt - 1 - tid) : r * ROUND_MAX_ATTEMPTS + tid;
    }
    key = -wave_max(-key);
    if (lane == 0) key_w[wv] = key;
    __syncthreads();
    key = key_w[0];
#pragma unroll
    for (int i = 1; i < WAVES_PER_BLOCK; ++i) key = min(key, key_w[i]);
    const int pick = rule == 0 ? (key < nattempt ? key : 2 * nattempt - 1 - key) : key % ROUND_MAX_ATTEMPTS;
    const int k = (int)blockIdx.x * BLOCK + tid;
    if (k < K) win[k] = slot[(size_t)pick * K + k];
    if (blockIdx.x == 0 && tid == 0) {
        info[0] = pick;
        info[1] = rem[pick];
    }
}

}  // namespace mmw
