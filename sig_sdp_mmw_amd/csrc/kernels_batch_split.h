// A batch iteration spread over several workgroups per instance (mmw_batch_set_split): the loop body of k_mmw_batch (kernels_batch.h)
// as three launches for all instances together, the kernel boundaries being the only synchronisation -- no atomics, no spin-wait,
// no grid barrier.
//
//   k_batch_split_head   one workgroup per instance: the gap row (GAP), averaging, DUAL, e_accu, softmax, LOSS -- O(nnz) work
//   k_batch_split_expm   one workgroup per (instance, column slice): the plan, the sketch and exp(L/2)R for the slice's columns
//   k_batch_split_x      one workgroup per (instance, entry range): X on the pattern for the range's entries
//
// Why the bits do not change.  exp(L/2)R is independent per column of the sketch: thread (row group, column) sums a row's entries
// in CSR order, the stop rule is per column and built from fmax only (exact, so the number of row groups does not matter), and the
// plan (mu, rho, substeps, order) is recomputed by every slice with k_mmw_batch's thread map and block reductions.  X on the pattern
// sums over q < D sequentially per stored entry; the trace is taken by every part with k_mmw_batch's thread map.  Each phase below
// restates the expressions of k_mmw_batch term by term; tests/test_hip_batch_split.py holds the two statements together, bitwise.
//
// The work tables (SplitSlice, SplitRange) and the slab of per-slice Taylor degrees live in buffers of the split's own: the
// arenas and their layout are those of the single-launch kernel.
#pragma once
#include "kernels_batch.h"

namespace mmw {

constexpr int BATCH_MAX_PARTS = MMW_BATCH_MAX_PARTS;
#ifndef MMW_SPLIT_COL_QUANTUM
#define MMW_SPLIT_COL_QUANTUM 8  // slice widths are multiples of it: 8 columns are one 64-byte run per gathered row; not yet timed against 16
#endif
constexpr int SPLIT_COL_QUANTUM = MMW_SPLIT_COL_QUANTUM;

// one workgroup of k_batch_split_expm
struct SplitSlice {
    int inst;   // instance of the batch
    int part;   // column slice of the instance: columns [part * width, min(D, (part + 1) * width))
    int width;  // columns per slice (the last may be narrower)
    int slab;   // where this slice's Taylor degree goes in the slab
};
// one workgroup of k_batch_split_x
struct SplitRange {
    int inst;    // instance of the batch
    int part;    // entry range of the instance: [part * nnzL / nparts, (part + 1) * nnzL / nparts)
    int nparts;  // entry ranges of the instance
    int slab0;   // where the instance's per-slice Taylor degrees start in the slab ...
    int nslab;   // ... and how many there are (its slice count); read by part 0
};

// Column slices of an instance: width W = 8 ceil(ceil(D / parts) / 8), G = ceil(D / W) slices.
__host__ __device__ inline int split_width(int D, int parts) {
    const int per = (D + parts - 1) / parts;
    return SPLIT_COL_QUANTUM * ((per + SPLIT_COL_QUANTUM - 1) / SPLIT_COL_QUANTUM);
}
__host__ __device__ inline int split_slices(int D, int parts) {
    const int W = split_width(D, parts);
    return (D + W - 1) / W;
}

// ---- iteration `it` of the call, top of the loop body down to the barrier after the lval update (k_mmw_batch, same statements)
template <bool GAP>
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_split_head(const BatchDesc* __restrict__ descs, const int* __restrict__ ia,
                                                                    double* __restrict__ fa, const GapDesc* __restrict__ gdescs,
                                                                    double* __restrict__ ga, int it) {
    const BatchDesc d = descs[blockIdx.x];
    if (it >= d.nrun) return;
    __shared__ double sh[BATCH_WAVES];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, C = d.C, nnz = d.nnzL, EA = d.E_asso, baseH = K + EA;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const int* __restrict__ pid = ia + d.o_pid;
    const int* __restrict__ diag = ia + d.o_diag;
    const int* __restrict__ apos = ia + d.o_apos;
    const double* __restrict__ sab = fa + d.o_sab;
    const double* __restrict__ sba = sab + nnz;
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
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1), eta = d.eta;
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    if constexpr (GAP) {
        const GapDesc g = gdescs[blockIdx.x];
        batch_gap_row(d, g, ia, fa, ga, d.iter0 + it, sh);
    }
    // ---- averaging and DUAL step 1
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
    // ---- DUAL step 2, e_accu
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
        const double a = eacc[c] + eth[c] * eta;
        eacc[c] = a;
        best = a > best ? a : best;
    }
    const double m = block_max(best, sh);
    // ---- softmax
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
            const double w = y * invn[c - baseH];
            wH[c - baseH] = w;
            sW += cH[c - baseH] * w;
        }
    }
    sD = block_sum(sD, sh);
    sF = block_sum(sF, sh);
    sW = block_sum(sW, sh);
    // ---- LOSS
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
}

// ---- the plan, the sketch and exp(L/2)R for the columns [c0, c1) of one instance
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_split_expm(const BatchDesc* __restrict__ descs, const SplitSlice* __restrict__ work,
                                                                    const int* __restrict__ ia, double* __restrict__ fa,
                                                                    const double* __restrict__ randv, double* __restrict__ slab, int it) {
    const SplitSlice w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    __shared__ double sh[BATCH_WAVES];
    __shared__ double red_a[BATCH_THREADS], red_b[BATCH_THREADS];
    __shared__ double c_prev[BATCH_MAX_D];
    __shared__ int c_on[BATCH_MAX_D];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, D = d.D;
    const int c0 = w.part * w.width, c1 = c0 + w.width < D ? c0 + w.width : D, Ds = c1 - c0;
    if (Ds <= 0) return;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const double* __restrict__ lval = fa + d.o_lval;
    double* Xh = fa + d.o_Xh;
    double* R = fa + d.o_R;
    double* __restrict__ info = fa + d.o_info;
    // the slice's thread map: column tc = c0 + tid % Ds, row group tg = tid / Ds of NG groups
    const int NG = NT / Ds, tc = c0 + tid % Ds, tg = tid / Ds, lc = tid % Ds;
    const bool tlive = tg < NG;
    const size_t KD = (size_t)K * D, KDs = (size_t)K * Ds;
    // ---- the plan (every slice the same bits: k_mmw_batch's thread map and reductions)
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
    // ---- the sketch: the slice's columns of the uploaded block, or of the rows drawn whole
    const int gi = d.iter0 + it;
    if (d.o_randv >= 0) {
        const double* src = randv + d.o_randv + (size_t)it * KD;
        for (size_t i = tid; i < KDs; i += NT) {
            const size_t at = (i / Ds) * D + c0 + i % Ds;
            R[at] = src[at];
        }
    } else {
        batch_sketch_rows(K, D, d.seed, (uint32_t)gi, R, c0, c1);
    }
    __syncthreads();
    // ---- exp(A) R on the slice
    double* F = Xh;
    double* T0 = fa + d.o_W1;
    double* T1 = fa + d.o_W2;
    for (size_t i = tid; i < KDs; i += NT) {
        const size_t at = (i / Ds) * D + c0 + i % Ds;
        F[at] = R[at];
        T0[at] = R[at];
    }
    __syncthreads();
    const double scale_mu = exp(mu / (double)nsub);
    int msteps = 0;
    for (int s = 0; s < nsub; ++s) {
        double fm = 0.0;
        if (tlive)
            for (int r = tg; r < K; r += NG) fm = fmax(fm, fabs(F[(size_t)r * D + tc]));
        red_a[tid] = fm;
        __syncthreads();
        for (int c = tid; c < Ds; c += NT) {
            double t = 0.0;
            for (int g = 0; g < NG; ++g) t = fmax(t, red_a[g * Ds + c]);
            c_prev[c] = t;
            c_on[c] = 1;
        }
        __syncthreads();
        for (int j = 1; j <= mo; ++j) {
            const double coef = 1.0 / ((double)nsub * (double)j);
            double tmax = 0.0, fmx = 0.0;
            if (tlive && c_on[lc]) {
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
            for (int c = tid; c < Ds; c += NT) {
                if (!c_on[c]) continue;
                double t = 0.0, f = 0.0;
                for (int g = 0; g < NG; ++g) { t = fmax(t, red_a[g * Ds + c]); f = fmax(f, red_b[g * Ds + c]); }
                if (c_prev[c] + t <= d.tol * f) c_on[c] = 0;
                c_prev[c] = t;
            }
            if (j > msteps) msteps = j;
            double* sw = T0; T0 = T1; T1 = sw;
            __syncthreads();
            int any = 0;
            for (int c = 0; c < Ds && !any; ++c) any = c_on[c];
            __syncthreads();
            if (!any) break;
        }
        if (s + 1 < nsub || scale_mu != 1.0)
            for (size_t i = tid; i < KDs; i += NT) {
                const size_t at = (i / Ds) * D + c0 + i % Ds;
                const double f = F[at] * scale_mu;
                F[at] = f;
                T0[at] = f;
            }
        __syncthreads();
    }
    if (tid == 0) {
        if (w.part == 0) { info[0] = rho; info[2] = (double)nsub; info[3] = mu; }
        slab[w.slab] = (double)msteps;
    }
}

// ---- X = X_half X_half^T / (tr / K) for the entries [p nnzL / P, (p + 1) nnzL / P) of one instance
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_split_x(const BatchDesc* __restrict__ descs, const SplitRange* __restrict__ work,
                                                                 const int* __restrict__ ia, double* __restrict__ fa,
                                                                 const double* __restrict__ slab, int it) {
    const SplitRange w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    const int64_t e0 = (int64_t)w.part * d.nnzL / w.nparts, e1 = (int64_t)(w.part + 1) * d.nnzL / w.nparts;
    if (e0 >= e1 && w.part != 0) return;  // an empty range (part 0 still owns rs and the info record)
    __shared__ double sh[BATCH_WAVES];
    __shared__ double rsl[BATCH_MAX_K];  // the K row sums sum_c Xh[k, c]^2: every part forms them all, for the trace
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, D = d.D;
    const int* __restrict__ col = ia + d.o_col;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const double* __restrict__ Xh = fa + d.o_Xh;
    double* __restrict__ xval = fa + d.o_xval;
    double* __restrict__ rs = fa + d.o_rsum;
    double* __restrict__ info = fa + d.o_info;
    double dsum = 0.0;
    for (int k = tid; k < K; k += NT) {
        const double* y = Xh + (size_t)k * D;
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += y[c] * y[c];
        rsl[k] = s;
        dsum += s;
    }
    const double tr = block_sum(dsum, sh) / (double)K;  // (its barriers publish rsl)
    const double itr = 1.0 / tr;
    for (int64_t e = e0 + tid; e < e1; e += NT) {
        const int r = lrow[e], c = col[e];
        double v;
        if (r == c) v = rsl[r];
        else {
            const double* a = Xh + (size_t)r * D;
            const double* b = Xh + (size_t)c * D;
            v = 0.0;
            for (int q = 0; q < D; ++q) v += a[q] * b[q];
        }
        xval[e] = v * itr;
    }
    if (w.part == 0) {
        for (int k = tid; k < K; k += NT) rs[k] = rsl[k];
        if (tid == 0) {
            double ms = 0.0;
            for (int i = 0; i < w.nslab; ++i) ms = fmax(ms, slab[w.slab0 + i]);
            info[1] = ms;
        }
    }
}

}  // namespace mmw
