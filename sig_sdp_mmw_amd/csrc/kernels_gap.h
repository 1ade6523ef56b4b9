// The duality gap (mmw.py:79-117, LOG_GAP) inside the loop of a solver handle, at any K: the row batch_gap_row (kernels_batch.h)
// computes in one workgroup, spread over the chip as plain launches on the handle's stream.
//
// One row = the build (two launches), then per Lanczos step two launches, and one small launch per scheduled check:
//   k_gap_build_a   off-diagonal row sums of Xbar, the D / F violations' maxima as slab partials; one more workgroup folds Ybar
//                   into the LOSS constant and the H weights and opens the row's state
//   k_gap_build_b   L(Ybar) on the pattern (LOSS formulas, coefficient +1) into the row's own float64 buffer; the H violations'
//                   maxima; the Philox start vector of (row, K, nnzL), unscaled, its squared norm as slab partials
//   k_gap_mv        step j: folds the slabs of beta_{j-1}^2 (every workgroup, the same fixed order), w = L u / beta, v = u / beta,
//                   alpha_j as slab partials.  It multiplies with the UNSCALED previous vector, so no launch stands between the
//                   norm and the product
//   k_gap_up        folds alpha_j, u = w - alpha_j v - beta_{j-1} v_prev, beta_j^2 as slab partials
//   k_gap_check     at m = 10, 20, ... (gap_check_list): theta_min(T_m) by Sturm multisection and the last eigenvector component
//                   by three inverse iterations, as batch_gap_row does them, tridiagonal in LDS; writes the row and the done word
// Every kernel returns at once when the done word of its row is set: a word an EARLIER launch on the same stream stored.  No
// workgroup waits for another inside a kernel; every sum across workgroups is a fixed-order fold of slabs, so a row is a function of
// the sums it reads and of the cap only.  An invariant subspace (beta_j <= 1e-11 scale) is noticed by k_gap_mv of step j + 1 in every
// workgroup alike: it stores stop_m = j, the launches behind it return, and the next check solves T_j.
//
// The phase reads the iterate (through PatternDev's entry-to-slot map when X lies in tile order) and writes its own buffers only.
// The arithmetic is float64 whatever the handle's T: an fp32 handle's sums are widened as they are read.
#pragma once
#include "kernels_batch.h"
#include "kernels_loop.h"

namespace mmw {

constexpr int GAPH_CHECK_THREADS = 512;  // batch_gap_row's workgroup: the multisection's shifts per round
constexpr int GAPH_MAX_SLABS = 1024;

struct GapState {
    double emax, hprev;  // e_max of the row; the upper end of theta's bracket, carried from check to check
    double scf[2];       // max_i (|alpha_i| + beta_i) over the steps whose beta is known, double-buffered by step parity
    int done, stop_m;
};
// one slot of the ring: everything a row needs to be continued by a later launch
struct GapRowDev {
    double* gl;    // [nnzL] L(Ybar)
    double* u;     // [K] the unscaled next vector
    double* w;     // [K] L v_j
    double* v[2];  // [K] v_j in v[j & 1], v_{j-1} in the other
    double* ta;    // [GAP_MAX_M] alpha_1 ..
    double* tb;    // [GAP_MAX_M] beta_1 ..
    double* apart; // [slabs] of alpha_j
    double* bpart; // [slabs] of beta_j^2 (of |start|^2 before step 1)
    GapState* st;
    double* out;   // {e_max, K theta, e_max - K theta, steps, 1 once written}: the row's own record, read back by the host
};
// what the build shares between rows (rows follow each other on the stream): row sums, H weights, the Y scalars, the maxima's slabs
struct GapBuildDev {
    double* wrs;    // [K]
    double* wwH;    // [K]
    double* ysc;    // {dconst}
    double* mpart;  // [2 slabs + 1]
};

// the pattern's constants in float64: an fp64 handle's own arrays; on an fp32 handle copies of the host's doubles (solver_gap.h), so
// that its rows differ from an fp64 handle's only through the iterate
struct GapConsts {
    const double* sab; const double* sba; const double* h_max; const double* S_sum; const double* inv_norm_H; const double* cH;
};

// the sum of part[0 .. n) in an order that depends on n alone: thread t of the first 256 takes t, t + 256, ...; then block_sum
// (threads past 256 add zeros, so a 512-thread workgroup folds to the same bits)
__device__ __forceinline__ double gap_fold(const double* __restrict__ part, int n, double* sh) {
    double s = 0.0;
    if (threadIdx.x < 256)
        for (int i = (int)threadIdx.x; i < n; i += 256) s += part[i];
    return block_sum(s, sh);
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_gap_widen(size_t n, const T* __restrict__ a, const T* __restrict__ b, double* __restrict__ a64, double* __restrict__ b64) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) {
        a64[i] = (double)a[i];
        b64[i] = (double)b[i];
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_gap_build_a(PatternDev<T> P, const T* __restrict__ xavg, const T* __restrict__ xdef, const T* __restrict__ yavg,
                                                       double nterm, GapConsts Cn, GapBuildDev B, GapRowDev R, int slabs) {
    __shared__ double sh[WAVES_PER_BLOCK];
    const int K = P.K, EA = P.E_asso, baseH = K + EA;
    const double invK = 1.0 / (double)K, Zm1 = (double)(P.Z - 1);
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    if ((int)blockIdx.x == slabs) {  // Ybar: the LOSS constant and the H weights; the row's state
        double sD = 0.0, sF = 0.0, sW = 0.0;
        for (int c = (int)threadIdx.x; c < P.C; c += BLOCK) {
            const double y = (double)yavg[c] / nterm;
            if (c < K) sD += y;
            else if (c < baseH) sF += y;
            else {
                const double w = y * Cn.inv_norm_H[c - baseH];
                B.wwH[c - baseH] = w;
                sW += Cn.cH[c - baseH] * w;
            }
        }
        sD = block_sum(sD, sh);
        sF = block_sum(sF, sh);
        sW = block_sum(sW, sh);
        if (threadIdx.x == 0) {
            B.ysc[0] = -(sD * invK) / (1.0 - invK) + (sF / ((double)K * Zm1)) / denF - sW;
            B.mpart[2 * slabs] = -1e300;
            GapState s{};
            s.hprev = 1e300;
            *R.st = s;
            R.out[4] = 0.0;
        }
        return;
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    double best = -1e300;
    for (int row = blockIdx.x * WAVES_PER_BLOCK + wib; row < K; row += slabs * WAVES_PER_BLOCK) {
        const int dp = P.diag_pos[row];
        double s = 0.0;
        for (int e = P.indptr[row] + lane; e < P.indptr[row + 1]; e += WAVE)
            if (e != dp) {
                const int q = P.xslot(e);
                s += ((double)xavg[q] + (xdef ? (double)xdef[q] : 0.0)) / nterm;
            }
        s = wave_sum(s);
        if (lane == 0) {
            B.wrs[row] = s;
            const int q = P.xdiag(row);
            const double eD = (((double)xavg[q] + (xdef ? (double)xdef[q] : 0.0)) / nterm - 1.0) * (1.0 / (1.0 - invK));
            best = eD > best ? eD : best;
        }
    }
    for (int p = blockIdx.x * BLOCK + threadIdx.x; p < EA; p += slabs * BLOCK) {
        const int q = P.xpair(p);
        const double eF = (((double)xavg[q] + (xdef ? (double)xdef[q] : 0.0)) / nterm + 1.0 / Zm1) / denF;
        best = eF > best ? eF : best;
    }
    best = block_max(best, sh);
    if (threadIdx.x == 0) B.mpart[blockIdx.x] = best;
}

// blocks [0, slabs): one wave per row -- eH, the start vector; blocks past them: the entries of L(Ybar), grid-stride
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_gap_build_b(PatternDev<T> P, const int* __restrict__ lrow, const T* __restrict__ yavg, double nterm, GapConsts Cn,
                                                       GapBuildDev B, GapRowDev R, int slabs) {
    __shared__ double sh[WAVES_PER_BLOCK];
    const int K = P.K, Z = P.Z;
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1);
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    if ((int)blockIdx.x >= slabs) {
        const double dconst = B.ysc[0], gscale = Zm1 / (double)(2 * Z);
        const int nb = (int)gridDim.x - slabs;
        for (int e = ((int)blockIdx.x - slabs) * BLOCK + (int)threadIdx.x; e < P.nnzL; e += nb * BLOCK) {
            const int r = lrow[e], c = P.col[e], q = P.pid[e];
            double v;
            if (c == r) v = ((double)yavg[r] / nterm) / (1.0 - invK) + dconst;
            else if (q >= 0) v = (((double)yavg[K + q] / nterm) * 0.5) / denF;
            else v = (Cn.sab[e] * B.wwH[c] + Cn.sba[e] * B.wwH[r]) * gscale;
            R.gl[e] = v;
        }
        return;
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    double best = -1e300, ss = 0.0;
    for (int row = blockIdx.x * WAVES_PER_BLOCK + wib; row < K; row += slabs * WAVES_PER_BLOCK) {
        double s = 0.0;
        for (int e = P.indptr[row] + lane; e < P.indptr[row + 1]; e += WAVE) {
            const double w = Cn.sab[e];
            if (w != 0.0) s += w * B.wrs[P.col[e]];
        }
        s = wave_sum(s);
        if (lane == 0) {
            const double eH = (s * Zm1 / (double)Z - (Cn.h_max[row] - (1.0 / (double)Z) * Cn.S_sum[row])) * Cn.inv_norm_H[row];
            best = eH > best ? eH : best;
            uint32_t w4[4];
            philox4x32_10((uint32_t)row, 0u, 0u, 0x4c5a4750u, (uint32_t)K, (uint32_t)P.nnzL, w4);
            double n0, n1;
            box_muller(w4, n0, n1);
            R.u[row] = n0;
            ss += n0 * n0;
        }
    }
    best = block_max(best, sh);
    ss = block_sum(ss, sh);
    if (threadIdx.x == 0) {
        B.mpart[slabs + blockIdx.x] = best;
        R.bpart[blockIdx.x] = ss;
    }
}

// step j, first launch.  lpr lanes serve a row (8, 16, 32 or 64); gridDim.x = slabs
__global__ __launch_bounds__(BLOCK) void k_gap_mv(const int* __restrict__ indptr, const int* __restrict__ col, int K, int j, int lpr, GapRowDev R, GapBuildDev B) {
    __shared__ double sh[WAVES_PER_BLOCK];
    GapState* st = R.st;
    if (st->done || st->stop_m) return;
    const int slabs = (int)gridDim.x;
    const double be = sqrt(gap_fold(R.bpart, slabs, sh));  // beta_{j-1}; |start| for j = 1
    if (j > 1) {
        const double a1 = fabs(R.ta[j - 2]), sc0 = st->scf[j & 1];  // (scf of step j - 2 lies at parity (j - 2) & 1)
        const double scale = fmax(fmax(sc0, a1), 1e-300);
        const bool stop = be <= 1e-11 * scale;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            R.tb[j - 2] = be;
            if (stop) st->stop_m = j - 1;
            else st->scf[(j - 1) & 1] = fmax(sc0, a1 + be);
        }
        if (stop) return;
    } else if (blockIdx.x == 0) {  // the row's e_max: the build's slabs
        double m = -1e300;
        for (int i = (int)threadIdx.x; i < 2 * slabs + 1; i += BLOCK) m = fmax(m, B.mpart[i]);
        m = block_max(m, sh);
        if (threadIdx.x == 0) st->emax = m;
    }
    const double ib = 1.0 / be;
    double* __restrict__ vc = R.v[j & 1];
    const int g = (int)threadIdx.x / lpr, l = (int)threadIdx.x % lpr, ng = BLOCK / lpr;
    double al = 0.0;
    for (int r = blockIdx.x * ng + g; r < K; r += slabs * ng) {
        double acc = 0.0;
        for (int e = indptr[r] + l; e < indptr[r + 1]; e += lpr) acc += R.gl[e] * R.u[col[e]];
        acc = group_sum(acc, lpr);
        if (l == 0) {
            const double wr = acc * ib, vr = R.u[r] * ib;
            R.w[r] = wr;
            vc[r] = vr;
            al += vr * wr;
        }
    }
    al = block_sum(al, sh);
    if (threadIdx.x == 0) R.apart[blockIdx.x] = al;
}

// step j, second launch; gridDim.x = slabs
__global__ __launch_bounds__(BLOCK) void k_gap_up(int K, int j, GapRowDev R) {
    __shared__ double sh[WAVES_PER_BLOCK];
    const GapState* st = R.st;
    if (st->done || st->stop_m) return;
    const int slabs = (int)gridDim.x;
    const double al = gap_fold(R.apart, slabs, sh);
    const double bp = j > 1 ? R.tb[j - 2] : 0.0;
    const double* __restrict__ vc = R.v[j & 1];
    const double* __restrict__ vp = R.v[(j + 1) & 1];
    double bb = 0.0;
    for (int r = blockIdx.x * BLOCK + (int)threadIdx.x; r < K; r += slabs * BLOCK) {
        double t = R.w[r] - al * vc[r];
        if (j > 1) t -= bp * vp[r];
        R.u[r] = t;
        bb += t * t;
    }
    bb = block_sum(bb, sh);
    if (threadIdx.x == 0) {
        R.bpart[blockIdx.x] = bb;
        if (blockIdx.x == 0) R.ta[j - 1] = al;
    }
}

// the check scheduled at step m (after k_gap_up of step m), one workgroup; mmax = min(K, cap)
__global__ __launch_bounds__(GAPH_CHECK_THREADS) void k_gap_check(int K, int m, int mmax, int slabs, GapRowDev R) {
    __shared__ double t_a[GAP_MAX_M], t_b[GAP_MAX_M], t_c[GAP_MAX_M], t_d[GAP_MAX_M], t_s[GAP_MAX_M];
    __shared__ double t_last;
    __shared__ double sh[GAPH_CHECK_THREADS / WAVE];
    GapState* st = R.st;
    if (st->done) return;
    const int tid = (int)threadIdx.x, NT = GAPH_CHECK_THREADS;
    const int stop_m = st->stop_m;
    const int j = stop_m ? stop_m : m;
    const double be = stop_m ? R.tb[j - 1] : sqrt(gap_fold(R.bpart, slabs, sh));
    double lo = 1e300, hi = -1e300, scale = 0.0, amin = 1e300;
    for (int i = tid; i < j; i += NT) {
        const double a = R.ta[i], bl = i > 0 ? R.tb[i - 1] : 0.0, br = i + 1 < j ? R.tb[i] : 0.0;
        t_a[i] = a;
        t_b[i] = i + 1 < j ? br : be;
        lo = fmin(lo, a - bl - br);
        hi = fmax(hi, a + bl + br);
        scale = fmax(scale, fabs(a) + br);
        amin = fmin(amin, a);
    }
    lo = -block_max(-lo, sh);
    hi = block_max(hi, sh);
    scale = fmax(block_max(scale, sh), 1e-300);
    amin = -block_max(-amin, sh);  // (its barriers publish t_a, t_b)
    // theta_min(T_j) in [lo, min(min_i alpha_i, the last check's upper end)]
    double l = lo, h = fmin(amin, st->hprev);
    for (int rd = 0; rd < 16 && h - l > 4e-16 * fmax(fabs(l), fabs(h)); ++rd) {
        const double w = h - l;
        const double x = l + w * ((double)(tid + 1) / (double)(NT + 1));
        double q = t_a[0] - x;
        bool below = q < 0.0;  // an eigenvalue of T_j below x (Sturm sequence)
        for (int i = 1; i < j && !below; ++i) {
            const double den = fabs(q) < 1e-300 ? (q < 0.0 ? -1e-300 : 1e-300) : q;
            q = t_a[i] - x - t_b[i - 1] * t_b[i - 1] / den;
            below = q < 0.0;
        }
        const int fi = (int)(-block_max(below ? -(double)tid : -(double)NT, sh));  // the first such shift
        const double nl = fi > 0 ? l + w * ((double)fi / (double)(NT + 1)) : l;
        if (fi < NT) h = l + w * ((double)(fi + 1) / (double)(NT + 1));
        l = nl;
    }
    const double theta = 0.5 * (l + h);
    if (tid == 0) {  // inverse iteration on (T_j - (theta - shift) I), positive definite
        const double shf = theta - 1e-10 * fmax(1.0, fabs(hi - lo));
        double piv = t_a[0] - shf;
        if (fabs(piv) < 1e-300) piv = 1e-300;
        double pinv = 1.0 / piv;
        t_d[0] = pinv;
#pragma unroll 4
        for (int i = 1; i < j; ++i) {
            const double bi = t_b[i - 1], c = bi * pinv;
            t_c[i - 1] = c;
            piv = t_a[i] - shf - bi * c;
            if (fabs(piv) < 1e-300) piv = 1e-300;
            pinv = 1.0 / piv;
            t_d[i] = pinv;
        }
        for (int i = 0; i < j; ++i) t_s[i] = 1.0;
        double nn = 0.0, sn = 0.0;
        for (int rep = 0; rep < 3; ++rep) {
            double sp = t_s[0];
#pragma unroll 8
            for (int i = 1; i < j; ++i) {
                sp = t_s[i] - t_c[i - 1] * sp;
                t_s[i] = sp;
            }
            sn = sp * t_d[j - 1];
            t_s[j - 1] = sn;
            nn = sn * sn;
#pragma unroll 8
            for (int i = j - 2; i >= 0; --i) {
                sn = t_s[i] * t_d[i] - t_c[i] * sn;
                t_s[i] = sn;
                nn += sn * sn;
            }
        }
        t_last = t_s[j - 1] / sqrt(nn);
    }
    __syncthreads();
    if (tid != 0) return;
    const bool conv = stop_m != 0 || fabs(be * t_last) <= 1e-11 * scale;
    if (conv || j >= mmax) {
        const int steps = conv || j >= K ? j : -j;
        const double kt = (double)K * theta, emax = st->emax;
        R.out[0] = emax;
        R.out[1] = kt;
        R.out[2] = emax - kt;
        R.out[3] = (double)steps;
        R.out[4] = 1.0;
        st->done = 1;
    } else
        st->hprev = h;
}

}  // namespace mmw
