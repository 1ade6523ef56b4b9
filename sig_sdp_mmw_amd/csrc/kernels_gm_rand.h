// MAX_RAND's draws where the state lies (mmw_gm_rand, mmw_batch_gm_rand; include/mmw_hip.h states the rule): the reference draws
// inprod = randn(Z, K) and rank = argsort(randn(K)) on the host (sim_src/alg/gm.py:148-150); here attempt a of a call with `seed` draws
//   pref_val[k][z]  a standard normal per (user, slot): the reference's inprod[z, k], user-major like k_slot_pref's input,
//   order_key[k]    a standard normal per user,
// from Philox4x32-10 under the key (seed low word, seed high word) with the counter (row, column pair, attempt, TAG): pref_val is a
// K x Z block with row = k and pairs of slots (an odd Z drops the second normal of the last pair), order_key a K x 1 block (the first
// normal of pair 0).  Users are visited by ascending order_key, ties to the lower user; a user prefers its slots by descending pref_val,
// ties to the lower slot (k_slot_pref's rule).  A value depends on (seed, attempt, k, z) alone.
//
// The uniforms are the sketch's (device_utils.h, box_muller): u1 = ((w0 << 21 ^ w1 >> 11) + 1) 2^-53 in (0, 1], u2 = (w2 + w3 2^-32) 2^-32
// in [0, 1); the normals are Box-Muller's r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2).  Unlike the sketch, whose values only have
// to agree to rounding error, these decide integers that a host-only handle (device -1) must give as well: ln and the sine / cosine are
// therefore NOT the math library's (the device's and the host's round differently in the last place) but the fixed sequences of IEEE
// additions, multiplications and one division below, without contraction -- the same bits on the device, on the host and in any
// restatement that follows the sequence (tests/helpers/gm_rand_cases.py).  Coefficients: the classic minimax polynomials of fdlibm's
// log, sin and cos kernels (below 1 ulp each on their ranges); the angle is reduced exactly to a quarter turn before it meets pi.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "device_utils.h"

namespace mmw {

constexpr uint32_t GMR_TAG_PREF = 0x47525046u;  // "GRPF": pref_val
constexpr uint32_t GMR_TAG_KEY = 0x47524b59u;   // "GRKY": order_key

// Philox4x32-10 (device_utils.h, philox4x32_10) in a form the host compiles too: the 32 x 32 products as 64-bit integers
__host__ __device__ inline void gmr_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    constexpr uint64_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = M0 * c0, p1 = M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// two standard normals from four words; every operation is one IEEE double operation in the order written
__host__ __device__ inline void gmr_normals(const uint32_t (&w)[4], double& n0, double& n1) {
#pragma clang fp contract(off)
    const double u1 = ((double)(((uint64_t)w[0] << 21) ^ (uint64_t)(w[1] >> 11)) + 1.0) * 0x1p-53;
    const double u2 = ((double)w[2] + (double)w[3] * 0x1p-32) * 0x1p-32;
    // ---- ln u1: u1 = m 2^e with m in [sqrt(1/2), sqrt 2) (u1 >= 2^-53 is a normal number), ln m by fdlibm's series in s = f / (2 + f)
    uint64_t bits;
    memcpy(&bits, &u1, sizeof bits);
    int e = (int)(bits >> 52) - 1022;
    const uint64_t mb = (bits & 0x000fffffffffffffull) | 0x3fe0000000000000ull;
    double m;
    memcpy(&m, &mb, sizeof m);  // in [1/2, 1)
    if (m < 0.7071067811865476) {
        m = m * 2.0;
        e -= 1;
    }
    const double f = m - 1.0, dk = (double)e;
    const double s = f / (2.0 + f), z = s * s, q = z * z;
    const double t1 = q * (3.999999999940941908e-01 + q * (2.222219843214978396e-01 + q * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + q * (2.857142874366239149e-01 + q * (1.818357216161805012e-01 + q * 1.479819860511658591e-01)));
    const double R = t2 + t1, hfsq = (0.5 * f) * f;
    const double lg = (((s * (hfsq + R) + dk * 1.90821492927058770002e-10) - hfsq) + f) + dk * 6.93147180369123816490e-01;
    const double r = sqrt(-2.0 * lg);
    // ---- cos and sin of 2 pi u2: x = 2 u2 half turns, j = the nearest quarter turn, t = x - j / 2 in [-1/4, 1/4] (exact), y = pi t
    const double x = 2.0 * u2;
    const double jf = floor(2.0 * x + 0.5);
    const double t = x - 0.5 * jf;
    const double y = t * 3.141592653589793;
    const double y2 = y * y, y3 = y2 * y;
    const double rs = 8.33333333332248946124e-03 + y2 * (-1.98412698298579493134e-04 + y2 * (2.75573137070700676789e-06 + y2 * (-2.50507602534068634195e-08 + y2 * 1.58969099521155010221e-10)));
    const double sn = y + y3 * (-1.66666666666666324348e-01 + y2 * rs);
    const double rc = y2 * (4.16666666666666019037e-02 + y2 * (-1.38888888888741095749e-03 + y2 * (2.48015872894767294178e-05 + y2 * (-2.75573143513906633035e-07 + y2 * (2.08757232129817482790e-09 + y2 * -1.13596475577881948265e-11)))));
    const double hz = 0.5 * y2, wc = 1.0 - hz;
    const double cs = wc + (((1.0 - wc) - hz) + y2 * rc);
    const int j = (int)jf & 3;
    const double c = j == 0 ? cs : j == 1 ? -sn : j == 2 ? -cs : sn;
    const double sv = j == 0 ? sn : j == 1 ? cs : j == 2 ? -sn : -cs;
    n0 = r * c;
    n1 = r * sv;
}

// the two preference values of user k's slot pair p (slots 2 p and 2 p + 1), and user k's order key
__host__ __device__ inline void gmr_pref_pair(int k, int p, uint64_t seed, uint32_t attempt, double& v0, double& v1) {
    uint32_t w[4];
    gmr_philox((uint32_t)k, (uint32_t)p, attempt, GMR_TAG_PREF, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    gmr_normals(w, v0, v1);
}
__host__ __device__ inline double gmr_order_key(int k, uint64_t seed, uint32_t attempt) {
    uint32_t w[4];
    gmr_philox((uint32_t)k, 0u, attempt, GMR_TAG_KEY, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    double v0, v1;
    gmr_normals(w, v0, v1);
    return v0;
}

// ---- pref_val[K][Z] of (seed, attempt), user-major: one thread per (user, slot pair), one writer per address
__global__ __launch_bounds__(BLOCK) void k_gm_rand_pref(int K, int Z, uint64_t seed, uint32_t attempt, double* __restrict__ P) {
    const int npair = (Z + 1) >> 1;
    const size_t n = (size_t)K * npair;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) {
        const int k = (int)(i / npair), p = (int)(i % npair);
        double v0, v1;
        gmr_pref_pair(k, p, seed, attempt, v0, v1);
        P[(size_t)k * Z + 2 * p] = v0;
        if (2 * p + 1 < Z) P[(size_t)k * Z + 2 * p + 1] = v1;
    }
}
// ---- order_key[K] of (seed, attempt), and its negation: k_rank_count ranks by DESCENDING key with ties to the lower index, so the
// ascending order with the same ties is its order of -key
__global__ __launch_bounds__(BLOCK) void k_gm_rand_key(int K, uint64_t seed, uint32_t attempt, double* __restrict__ key, double* __restrict__ neg) {
    for (int k = blockIdx.x * BLOCK + threadIdx.x; k < K; k += gridDim.x * BLOCK) {
        const double v = gmr_order_key(k, seed, attempt);
        key[k] = v;
        neg[k] = -v;
    }
}

// ---- the same on the host (device -1 handles, host-only batches)
inline void gm_rand_draw_host(int K, int Z, uint64_t seed, uint32_t attempt, double* pref_val, double* order_key) {
    const int npair = (Z + 1) >> 1;
    for (int k = 0; k < K; ++k) {
        if (order_key) order_key[k] = gmr_order_key(k, seed, attempt);
        if (!pref_val) continue;
        for (int p = 0; p < npair; ++p) {
            double v0, v1;
            gmr_pref_pair(k, p, seed, attempt, v0, v1);
            pref_val[(size_t)k * Z + 2 * p] = v0;
            if (2 * p + 1 < Z) pref_val[(size_t)k * Z + 2 * p + 1] = v1;
        }
    }
}
// order[K]: ascending order_key, ties to the lower user; pref[K][Z]: descending pref_val, ties to the lower slot
inline void gm_rand_order_host(int K, int Z, const double* pref_val, const double* order_key, int32_t* order, int32_t* pref) {
    std::iota(order, order + K, 0);
    std::stable_sort(order, order + K, [&](int32_t a, int32_t b) { return order_key[a] < order_key[b]; });
    for (int k = 0; k < K; ++k) {
        int32_t* row = pref + (size_t)k * Z;
        const double* v = pref_val + (size_t)k * Z;
        std::iota(row, row + Z, 0);
        std::stable_sort(row, row + Z, [&](int32_t a, int32_t b) { return v[a] > v[b]; });
    }
}
// k_round_pick's two rules on the host
inline int gm_rand_pick_host(const int32_t* rem, int nattempt, int rule) {
    int pick = rule == 0 ? nattempt - 1 : 0;
    for (int a = 0; a < nattempt; ++a) {
        if (rule == 0 && rem[a] == 0) return a;
        if (rule == 1 && rem[a] < rem[pick]) pick = a;
    }
    return pick;
}

}  // namespace mmw
