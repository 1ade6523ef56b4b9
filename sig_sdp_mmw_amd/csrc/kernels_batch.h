// Many small MMW instances in one launch: one workgroup per instance, `n` iterations of the loop body mmw.py:75-200 per call.
//
// The per-handle path (kernels_loop.h, kernels_expm.h) spreads ONE instance over the chip and pays ~20 dependent launches per
// iteration.  The reference's sweeps solve instances of K = 75 ... 675 users, where those launches are almost all latency: here
// every phase of an iteration is a loop of the instance's own workgroup, separated by __syncthreads() only.  No grid barrier, no
// spin-wait, no atomics: an instance's result depends on nothing but its own data, and every reduction runs in a fixed order
// inside the workgroup, so it is bitwise the same whatever its batch neighbours are and however the iterations are split into calls.
//
// Layout.  All instances share two device arenas (int32 and fp64); a BatchDesc per instance holds its sizes and the offsets of its
// arrays.  Pattern arrays are the handle's (csrc/pattern.h, CSR order of L / X).  The iterate, the K x D blocks (sketch R, the
// Taylor terms W1 / W2 and exp(L/2)R) and the per-row scalars stay in the arena: at these sizes (tens to hundreds of KB per
// instance) they are L2-resident for the whole call.  LDS holds the reduction slabs and the per-column stop state only.
//
// exp(L/2)R: shifted truncated Taylor (the scheme of scipy's expm_multiply) with the a-priori plan of the handles (plan_order on the
// row-sum bound of ||L/2 - mu I||_1, substeps doubled until the order fits max_order), planned in the workgroup every iteration,
// with a per-column stop: column c stops adding terms once ||T_{j-1} e_c||_inf + ||T_j e_c||_inf <= tol ||F e_c||_inf.
//
// The duality gap (mmw.py:79-117, LOG_GAP) is a phase of the same workgroup: k_mmw_batch<true> logs one row per iteration (the
// maximum violation at Xbar, K lambda_min(L(Ybar)) by Lanczos with the tridiagonal solved in the workgroup, their difference and the
// Lanczos steps taken) into a work buffer of its own.  The phase reads the iterate and writes nothing of it; k_mmw_batch<false> is
// the kernel without the phase.
//
// Limits (mmw_batch_create refuses larger instances; they stay on handles): K <= BATCH_MAX_K, D = Z * rank_radio <= BATCH_MAX_D
// (the sketch's lane layout: 64 lanes x 4 groups x 2 columns), nnzL <= BATCH_MAX_NNZ, and BATCH_MAX_BYTES of arena per instance.
#pragma once
#include "device_utils.h"
#include "kernels_expm.h"

namespace mmw {

constexpr int BATCH_THREADS = 512;  // 8 waves: one workgroup per instance
constexpr int BATCH_WAVES = BATCH_THREADS / WAVE;
constexpr int BATCH_MAX_K = 4096;
constexpr int BATCH_MAX_D = 512;
constexpr int64_t BATCH_MAX_NNZ = (int64_t)1 << 22;
constexpr int64_t BATCH_MAX_BYTES = (int64_t)96 << 20;

struct BatchDesc {
    int K, Z, D, E_asso, C, nnzL;
    int nrun;        // iterations this call runs for the instance (0: none)
    int iter0;       // iterations the instance had done before this call (the sketch counter)
    int max_order;
    int pad0;
    double eta, tol;
    uint64_t seed;
    int64_t o_randv;  // offset of the instance's uploaded sketches in this call's randv buffer, -1: Philox on the device
    // int32 arena
    int64_t o_indptr, o_col, o_lrow, o_pid, o_diag, o_apos;
    // fp64 arena: pattern data
    int64_t o_sab, o_hmax, o_ssum, o_invn, o_cH;
    // fp64 arena: iterate
    int64_t o_lval, o_xval, o_xavg, o_Y, o_yavg, o_eaccu, o_ethis, o_wH, o_rsum;
    int64_t o_Xh, o_R, o_W1, o_W2, o_info;
};

// The row-normalised Philox sketch of (seed, iteration) with the layout of kernels_loop.h's sketch_rows for fp64 (one wave per row,
// lane l draws column pairs l + 64 i, i < 4; the squared norm in the same order and the same wave reduction): the block is bitwise
// the one a handle's mmw_sketch returns for that (seed, iteration).  R is K x D, row-major, stride D.  Every row is drawn whole (its
// norm needs all D columns); only the columns [c0, c1) are written: 0, D for the whole block, a slice for kernels_batch_split.h.
__device__ __forceinline__ void batch_sketch_rows(int K, int D, uint64_t seed, uint32_t iter, double* __restrict__ R, int c0, int c1) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int ngroups = (D + 1) >> 1;
    for (int row = wib; row < K; row += nw) {
        double n[4][2];
        double ssl = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = lane + WAVE * i;
            n[i][0] = n[i][1] = 0.0;
            if (p < ngroups) {
                uint32_t w[4];
                philox4x32_10((uint32_t)row, (uint32_t)p, iter, 0x4d4d5753u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
                box_muller(w, n[i][0], n[i][1]);
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    if (p * 2 + v >= D) n[i][v] = 0.0;
                    ssl += n[i][v] * n[i][v];
                }
            }
        }
        const double ss = wave_sum(ssl);
        const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = lane + WAVE * i;
#pragma unroll
            for (int v = 0; v < 2; ++v)
                if (p * 2 + v >= c0 && p * 2 + v < c1) R[(size_t)row * D + p * 2 + v] = n[i][v] * inv;
        }
    }
}

// one sketch block per workgroup (mmw_batch_sketch)
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_sketch(int K, int D, uint64_t seed, uint32_t iter, double* __restrict__ R) {
    batch_sketch_rows(K, D, seed, iter, R, 0, D);
}

// ---- the duality gap of one iteration (mmw.py:79-117), a phase of the instance's workgroup ----------------------------------------
constexpr int GAP_MAX_M = 1024;     // Lanczos steps per row at most: the tridiagonal and its solve live in LDS
constexpr int GAP_DEFAULT_M = 600;  // the handles' cap (solver_extras.h lambda_min)

struct GapDesc {
    int m_cap, pad0;
    int64_t o_work;  // gap buffer: L(Ybar) on the pattern [nnzL], row sums [K], H weights [K], three Lanczos vectors [3K]
    int64_t o_log;   // gap buffer: 4 doubles per iteration {e_max, K theta, e_max - K theta, steps}
};

// Row `gi` of the instance's gap log, from n = gi + 1 terms: xbar = (xavg + xval) / n and ybar = (yavg + Y) / n are the averages the
// iteration forms right after (the same sums, bitwise).  e_max by the DUAL formulas, L(Ybar) by the LOSS formulas with coefficient
// +1, lambda_min by plain Lanczos (no reorthogonalisation: the extreme Ritz value converges regardless) on a Philox start vector
// keyed by the instance's sizes.  One row takes 8 lanes in the SpMV (cross-lane sum in a fixed order); alpha and beta are fixed-order
// block sums.  theta_min(T_m) and the last component of its eigenvector are solved in the workgroup at m = 10, 20, ... with the
// interval growing by a quarter: theta by multisection of the Sturm count (every thread one shift per round, the bracket's upper
// end carried over from the last check: theta_min(T_m) does not increase with m), the eigenvector by three inverse iterations of
// one lane on a factorisation kept in LDS (reciprocal pivots and multipliers: one fma per element and pass).  Stop: |beta_m s_m| <= 1e-11 scale (the handles' criterion and scale; beta_m <= 1e-11
// scale, an invariant subspace, meets it at once), or m = min(K, m_cap): steps is negative when the cap cut a Krylov space short.
__device__ __forceinline__ void batch_gap_row(const BatchDesc& d, const GapDesc& g, const int* __restrict__ ia, const double* fa,
                                              double* __restrict__ ga, int gi, double* sh) {
    __shared__ double t_a[GAP_MAX_M], t_b[GAP_MAX_M], t_c[GAP_MAX_M], t_d[GAP_MAX_M], t_s[GAP_MAX_M];
    __shared__ double t_last;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, C = d.C, nnz = d.nnzL, EA = d.E_asso, baseH = K + EA;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const int* __restrict__ pid = ia + d.o_pid;
    const int* __restrict__ diag = ia + d.o_diag;
    const int* __restrict__ apos = ia + d.o_apos;
    const double* sab = fa + d.o_sab;
    const double* sba = sab + nnz;
    const double* hmax = fa + d.o_hmax;
    const double* ssum = fa + d.o_ssum;
    const double* invn = fa + d.o_invn;
    const double* cH = fa + d.o_cH;
    const double* xval = fa + d.o_xval;
    const double* xavg = fa + d.o_xavg;
    const double* Y = fa + d.o_Y;
    const double* yavg = fa + d.o_yavg;
    double* gl = ga + g.o_work;
    double* wrs = gl + nnz;
    double* wwH = wrs + K;
    double* vp = wwH + K;
    double* vc = vp + K;
    double* vw = vc + K;
    const double nterm = (double)(gi + 1);
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1);
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    // ---- e_max = max e(Xbar) (mmw.py:81-96, the DUAL formulas of the loop body)
    double best = -1e300;
    for (int k = tid; k < K; k += NT) {
        const int dp = diag[k];
        double s = 0.0;
        for (int e = indptr[k]; e < indptr[k + 1]; ++e)
            if (e != dp) s += (xavg[e] + xval[e]) / nterm;
        wrs[k] = s;
        const double eD = ((xavg[dp] + xval[dp]) / nterm - 1.0) * (1.0 / (1.0 - invK));
        best = eD > best ? eD : best;
    }
    for (int p = tid; p < EA; p += NT) {
        const double eF = ((xavg[apos[p]] + xval[apos[p]]) / nterm + 1.0 / Zm1) / denF;
        best = eF > best ? eF : best;
    }
    __syncthreads();
    for (int k = tid; k < K; k += NT) {
        double s = 0.0;
        for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
            const double w = sab[e];
            if (w != 0.0) s += w * wrs[col[e]];
        }
        const double eH = (s * Zm1 / (double)Z - (hmax[k] - (1.0 / (double)Z) * ssum[k])) * invn[k];
        best = eH > best ? eH : best;
    }
    const double emax = block_max(best, sh);
    // ---- L(Ybar) on the pattern (mmw.py:98-115, the LOSS formulas with coefficient +1)
    double sD = 0.0, sF = 0.0, sW = 0.0;
    for (int c = tid; c < C; c += NT) {
        const double y = (yavg[c] + Y[c]) / nterm;
        if (c < K) sD += y;
        else if (c < baseH) sF += y;
        else {
            const double w = y * invn[c - baseH];
            wwH[c - baseH] = w;
            sW += cH[c - baseH] * w;
        }
    }
    sD = block_sum(sD, sh);
    sF = block_sum(sF, sh);
    sW = block_sum(sW, sh);  // (its barriers publish wwH)
    const double dconst = -(sD * invK) / (1.0 - invK) + (sF / ((double)K * Zm1)) / denF - sW;
    const double gscale = Zm1 / (double)(2 * Z);
    for (int e = tid; e < nnz; e += NT) {
        const int r = lrow[e], c = col[e], q = pid[e];
        double v;
        if (c == r) v = ((yavg[r] + Y[r]) / nterm) / (1.0 - invK) + dconst;
        else if (q >= 0) v = (((yavg[K + q] + Y[K + q]) / nterm) * 0.5) / denF;
        else v = (sab[e] * wwH[c] + sba[e] * wwH[r]) * gscale;
        gl[e] = v;
    }
    // ---- lambda_min(L(Ybar)): 8 lanes per row, lane 0 of a group owns the row's vector entries
    const int g8 = tid >> 3, l8 = tid & 7, NG8 = NT >> 3;
    double ss = 0.0;
    if (l8 == 0)
        for (int r = g8; r < K; r += NG8) {
            uint32_t w[4];
            philox4x32_10((uint32_t)r, 0u, 0u, 0x4c5a4750u, (uint32_t)K, (uint32_t)nnz, w);
            double n0, n1;
            box_muller(w, n0, n1);
            vc[r] = n0;
            ss += n0 * n0;
        }
    ss = block_sum(ss, sh);
    const double inrm = 1.0 / sqrt(ss);
    if (l8 == 0)
        for (int r = g8; r < K; r += NG8) vc[r] *= inrm;
    __syncthreads();  // gl and the start vector
    const int mmax = K < g.m_cap ? K : g.m_cap;
    double beta_prev = 0.0, theta = 0.0, hprev = 1e300;
    double lo_full = 1e300, hi_full = -1e300, sc_full = 0.0, amin = 1e300;
    int steps = 0, next = mmax < 10 ? mmax : 10;
    for (int j = 1; j <= mmax; ++j) {
        double al = 0.0;
        for (int r = g8; r < K; r += NG8) {
            double acc = 0.0;
            for (int e = indptr[r] + l8; e < indptr[r + 1]; e += 8) acc += gl[e] * vc[col[e]];
            acc = group_sum(acc, 8);
            if (l8 == 0) {
                vw[r] = acc;
                al += vc[r] * acc;
            }
        }
        al = block_sum(al, sh);
        double bb = 0.0;
        if (l8 == 0)
            for (int r = g8; r < K; r += NG8) {
                double t = vw[r] - al * vc[r];
                if (j > 1) t -= beta_prev * vp[r];
                vw[r] = t;
                bb += t * t;
            }
        bb = block_sum(bb, sh);
        const double be = sqrt(bb);
        if (tid == 0) { t_a[j - 1] = al; t_b[j - 1] = be; }
        // Gershgorin bounds and the scale of T_j (its last row has beta_{j-1} only)
        const double lo = fmin(lo_full, al - beta_prev), hi = fmax(hi_full, al + beta_prev);
        const double scale = fmax(fmax(sc_full, fabs(al)), 1e-300);
        amin = fmin(amin, al);
        lo_full = fmin(lo_full, al - beta_prev - be);
        hi_full = fmax(hi_full, al + beta_prev + be);
        sc_full = fmax(sc_full, fabs(al) + be);
        if (be <= 1e-11 * scale || j == next || j == mmax) {
            __syncthreads();  // t_a, t_b
            // theta_min(T_j) in [lo, min(min_i alpha_i, the last check's upper end)]
            double l = lo, h = fmin(amin, hprev);
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
            theta = 0.5 * (l + h);
            hprev = h;
            if (tid == 0) {  // inverse iteration on (T_j - (theta - shift) I), positive definite
                const double shf = theta - 1e-10 * fmax(1.0, fabs(hi - lo));
                // pivots once (the shift is the same for the three solves): t_d = 1 / pivot, t_c = beta / pivot
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
                // three solves from s = 1, unnormalised in between (growth <= 1e10 per solve); each pass is one fma per element
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
            const bool conv = fabs(be * t_last) <= 1e-11 * scale;
            if (conv || j == mmax) {
                steps = conv || j >= K ? j : -j;
                break;
            }
            next = j + (j / 4 > 10 ? j / 4 : 10);
            next = next < mmax ? next : mmax;
        }
        const double ib = 1.0 / be;
        if (l8 == 0)
            for (int r = g8; r < K; r += NG8) vw[r] *= ib;
        double* const t = vp;
        vp = vc;
        vc = vw;
        vw = t;
        beta_prev = be;
        __syncthreads();
    }
    if (tid == 0) {
        double* row = ga + g.o_log + (size_t)4 * gi;
        const double kt = (double)K * theta;
        row[0] = emax;
        row[1] = kt;
        row[2] = emax - kt;
        row[3] = (double)steps;
    }
}

template <bool GAP>
__global__ __launch_bounds__(BATCH_THREADS) void k_mmw_batch(const BatchDesc* __restrict__ descs, const int* __restrict__ ia,
                                                             double* __restrict__ fa, const double* __restrict__ randv,
                                                             const GapDesc* __restrict__ gdescs, double* __restrict__ ga) {
    const BatchDesc d = descs[blockIdx.x];
    if (d.nrun <= 0) return;
    __shared__ double sh[BATCH_WAVES];
    __shared__ double red_a[BATCH_THREADS], red_b[BATCH_THREADS];  // per (row group, column) partial maxima of the Taylor stop
    __shared__ double c_prev[BATCH_MAX_D];                          // ||T_{j-1} e_c||_inf
    __shared__ int c_on[BATCH_MAX_D];                               // column c still adds terms
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, D = d.D, C = d.C, nnz = d.nnzL, EA = d.E_asso, baseH = K + EA;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const int* __restrict__ pid = ia + d.o_pid;
    const int* __restrict__ diag = ia + d.o_diag;
    const int* __restrict__ apos = ia + d.o_apos;
    const double* __restrict__ sab = fa + d.o_sab;
    const double* __restrict__ sba = sab + nnz;  // S_T'[col,row] follows S_T'[row,col]
    const double* __restrict__ hmax = fa + d.o_hmax;
    const double* __restrict__ ssum = fa + d.o_ssum;
    const double* __restrict__ invn = fa + d.o_invn;
    const double* __restrict__ cH = fa + d.o_cH;
    double* __restrict__ lval = fa + d.o_lval;
    double* __restrict__ xval = fa + d.o_xval;
    double* __restrict__ xavg = fa + d.o_xavg;
    double* __restrict__ Y = fa + d.o_Y;
    double* __restrict__ yavg = fa + d.o_yavg;
    double* __restrict__ eacc = fa + d.o_eaccu;
    double* __restrict__ eth = fa + d.o_ethis;
    double* __restrict__ wH = fa + d.o_wH;
    double* __restrict__ rs = fa + d.o_rsum;
    double* __restrict__ Xh = fa + d.o_Xh;
    double* __restrict__ R = fa + d.o_R;
    double* __restrict__ info = fa + d.o_info;
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1), eta = d.eta;
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;  // mmw.py:131 (= cF of the LOSS, mmw.py:150)
    // the Taylor block's thread map: column c = tid % D, row group g = tid / D of NG groups (threads past NG * D idle there)
    const int NG = NT / D, tc = tid % D, tg = tid / D;
    const bool tlive = tg < NG;
    const size_t KD = (size_t)K * D;
    GapDesc g{};
    if constexpr (GAP) g = gdescs[blockIdx.x];

    for (int it = 0; it < d.nrun; ++it) {
        if constexpr (GAP) {
            // ---- LOG_GAP (mmw.py:79-117) on the sums this iteration is about to form; reads the iterate only
            batch_gap_row(d, g, ia, fa, ga, d.iter0 + it, sh);
        }
        // ---- averaging (mmw.py:77-78) and DUAL step 1: off-diagonal row sums of X, eD, eF (mmw.py:124-131)
        for (int e = tid; e < nnz; e += NT) xavg[e] += xval[e];
        for (int c = tid; c < C; c += NT) yavg[c] += Y[c];
        for (int k = tid; k < K; k += NT) {
            const int dp = diag[k];
            double s = 0.0;
            for (int e = indptr[k]; e < indptr[k + 1]; ++e)
                if (e != dp) s += xval[e];
            rs[k] = s;
            eth[k] = (xval[dp] - 1.0) * (1.0 / (1.0 - invK));
        }
        for (int p = tid; p < EA; p += NT) eth[K + p] = (xval[apos[p]] + 1.0 / Zm1) / denF;
        __syncthreads();
        // ---- DUAL step 2: eH = (S_T' (X_offdi 1) (Z-1)/Z - (h - S_sum/Z)) / norm_H (mmw.py:133-134, the SpGEMM as an SpMV), e_accu
        double best = -1e300;
        for (int k = tid; k < K; k += NT) {
            double s = 0.0;
            for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
                const double w = sab[e];
                if (w != 0.0) s += w * rs[col[e]];
            }
            eth[baseH + k] = (s * Zm1 / (double)Z - (hmax[k] - (1.0 / (double)Z) * ssum[k])) * invn[k];
        }
        __syncthreads();
        for (int c = tid; c < C; c += NT) {
            const double a = eacc[c] + eth[c] * eta;  // mmw.py:137
            eacc[c] = a;
            best = a > best ? a : best;
        }
        const double m = block_max(best, sh);
        // ---- softmax (mmw.py:139)
        double tot = 0.0;
        for (int c = tid; c < C; c += NT) {
            const double ex = exp(eacc[c] - m);
            Y[c] = ex;
            tot += ex;
        }
        tot = block_sum(tot, sh);
        double sD = 0.0, sF = 0.0, sW = 0.0;
        for (int c = tid; c < C; c += NT) {
            const double y = Y[c] / tot;
            Y[c] = y;
            if (c < K) sD += y;
            else if (c < baseH) sF += y;
            else {
                const double w = y * invn[c - baseH];  // column scaling of the CSC matrix (mmw.py:162-163, scipy_util.py:20-24)
                wH[c - baseH] = w;
                sW += cH[c - baseH] * w;
            }
        }
        sD = block_sum(sD, sh);
        sF = block_sum(sF, sh);
        sW = block_sum(sW, sh);
        // ---- LOSS: L_accu -= eta (LD + LF + LH) on the pattern (mmw.py:144-167)
        const double dconst = -(sD * invK) / (1.0 - invK) + (sF / ((double)K * Zm1)) / denF - sW;
        const double gscale = Zm1 / (double)(2 * Z);
        for (int e = tid; e < nnz; e += NT) {
            const int r = lrow[e], c = col[e], q = pid[e];
            double add;
            if (c == r) add = Y[r] / (1.0 - invK) + dconst;
            else if (q >= 0) add = (Y[K + q] * 0.5) / denF;
            else add = (sab[e] * wH[c] + sba[e] * wH[r]) * gscale;
            lval[e] = lval[e] - eta * add;
        }
        __syncthreads();
        // ---- the plan of exp(A) R, A = L/2: mu = tr(A)/K, rho >= ||A - mu I||_1 from the row sums (as kernels_expm.h's plan_body)
        double sd = 0.0, pp = -1e300, pm = -1e300;
        for (int k = tid; k < K; k += NT) {
            double dg = 0.0, o = 0.0;
            for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
                const double v = 0.5 * lval[e];
                if (col[e] == k) dg = v;
                else o += fabs(v);
            }
            sd += dg;
            pp = dg + o > pp ? dg + o : pp;
            pm = o - dg > pm ? o - dg : pm;
        }
        sd = block_sum(sd, sh);
        pp = block_max(pp, sh);
        pm = block_max(pm, sh);
        const double mu = sd / (double)K;
        const double rho = pp - mu > pm + mu ? pp - mu : pm + mu;
        int nsub = 1, mo = -1;
        for (; nsub <= 4096; nsub *= 2) {
            mo = plan_order(1, rho / nsub, d.tol / nsub, d.max_order);
            if (mo > 0) break;
        }
        if (mo <= 0) { mo = d.max_order; nsub = 4096; }
        // ---- the sketch of this iteration (mmw.py:226-227): uploaded, or Philox keyed by (seed, iteration, row, column pair)
        const int gi = d.iter0 + it;
        if (d.o_randv >= 0) {
            const double* src = randv + d.o_randv + (size_t)it * KD;
            for (size_t i = tid; i < KD; i += NT) R[i] = src[i];
        } else {
            batch_sketch_rows(K, D, d.seed, (uint32_t)gi, R, 0, D);
        }
        __syncthreads();
        // ---- exp(A) R by nsub substeps of degree <= mo with a per-column stop (mmw.py:180, 228)
        double* F = Xh;
        double* T0 = fa + d.o_W1;
        double* T1 = fa + d.o_W2;
        for (size_t i = tid; i < KD; i += NT) { F[i] = R[i]; T0[i] = R[i]; }
        __syncthreads();  // written row-major by thread, read below by (row group, column)
        const double scale_mu = exp(mu / (double)nsub);
        int msteps = 0;
        for (int s = 0; s < nsub; ++s) {
            // ||F e_c||_inf at the start of the substep
            double fm = 0.0;
            if (tlive)
                for (int r = tg; r < K; r += NG) fm = fmax(fm, fabs(F[(size_t)r * D + tc]));
            red_a[tid] = fm;
            __syncthreads();
            for (int c = tid; c < D; c += NT) {
                double t = 0.0;
                for (int g = 0; g < NG; ++g) t = fmax(t, red_a[g * D + c]);
                c_prev[c] = t;
                c_on[c] = 1;
            }
            __syncthreads();
            for (int j = 1; j <= mo; ++j) {
                const double coef = 1.0 / ((double)nsub * (double)j);
                double tmax = 0.0, fmx = 0.0;
                if (tlive && c_on[tc]) {
                    for (int r = tg; r < K; r += NG) {
                        double acc = 0.0;
                        for (int e = indptr[r]; e < indptr[r + 1]; ++e) acc += (0.5 * lval[e]) * T0[(size_t)col[e] * D + tc];
                        const double t = (acc - mu * T0[(size_t)r * D + tc]) * coef;
                        T1[(size_t)r * D + tc] = t;
                        const double f = F[(size_t)r * D + tc] + t;
                        F[(size_t)r * D + tc] = f;
                        tmax = fmax(tmax, fabs(t));
                        fmx = fmax(fmx, fabs(f));
                    }
                }
                red_a[tid] = tmax;
                red_b[tid] = fmx;
                __syncthreads();
                for (int c = tid; c < D; c += NT) {
                    if (!c_on[c]) continue;
                    double t = 0.0, f = 0.0;
                    for (int g = 0; g < NG; ++g) { t = fmax(t, red_a[g * D + c]); f = fmax(f, red_b[g * D + c]); }
                    if (c_prev[c] + t <= d.tol * f) c_on[c] = 0;
                    c_prev[c] = t;
                }
                if (tid == 0 && j > msteps) msteps = j;
                double* sw = T0; T0 = T1; T1 = sw;
                // all columns stopped: the block is done early (a workgroup-uniform decision read from LDS)
                __syncthreads();
                int any = 0;
                for (int c = 0; c < D && !any; ++c) any = c_on[c];
                __syncthreads();
                if (!any) break;
            }
            if (s + 1 < nsub || scale_mu != 1.0)
                for (size_t i = tid; i < KD; i += NT) {
                    const double f = F[i] * scale_mu;
                    F[i] = f;
                    T0[i] = f;
                }
            __syncthreads();
        }
        if (tid == 0) { info[0] = rho; info[1] = (double)msteps; info[2] = (double)nsub; info[3] = mu; }
        // ---- X = X_half X_half^T / (tr / K) on the pattern (mmw.py:182-194)
        double dsum = 0.0;
        for (int k = tid; k < K; k += NT) {
            const double* y = Xh + (size_t)k * D;
            double s = 0.0;
            for (int c = 0; c < D; ++c) s += y[c] * y[c];
            rs[k] = s;
            dsum += s;
        }
        const double tr = block_sum(dsum, sh) / (double)K;
        const double itr = 1.0 / tr;
        for (int e = tid; e < nnz; e += NT) {
            const int r = lrow[e], c = col[e];
            double v;
            if (r == c) v = rs[r];
            else {
                const double* a = Xh + (size_t)r * D;
                const double* b = Xh + (size_t)c * D;
                v = 0.0;
                for (int q = 0; q < D; ++q) v += a[q] * b[q];
            }
            xval[e] = v * itr;
        }
        __syncthreads();
    }
}

}  // namespace mmw
