// The head and the plan of a batch iteration spread over workgroups (mmw_batch_set_head_split): everything k_batch_split_head and
// k_batch_rows_plan do on one workgroup per instance, O(nnzL), as launches with one workgroup per (instance, row part), and the row
// sums of X_half X_half^T that every entry range of k_batch_split_x recomputes, once.  An iteration is
//
//   k_batch_head_gap     only with the gap on: one workgroup per instance, batch_gap_row unchanged -- a launch of its own, because
//                        it reads the running sums before this iteration's terms are added
//   k_batch_head_avg     own rows: xavg += xval on their entries, the off-diagonal row sums rs, eD; own share of the pairs: eF; yavg += Y
//   k_batch_head_dual    own rows: eH, from the rs of all rows (written by the launch before)
//   k_batch_head_fold    one workgroup per instance, O(C): e_accu, its maximum, the softmax, wH, (sD, sF, sW) and the LOSS constant into
//                        a per-instance record
//   k_batch_head_loss    own rows: the LOSS update of their entries, then the plan's per-row (dg, o) into two K-length scratch arrays
//   k_batch_head_plan    row-split path only, one workgroup per instance, O(K): k_batch_rows_plan with its pass over L replaced by
//                        reads of (dg, o); the column-split path keeps k_batch_split_expm, which plans for itself
//   ... exp(L/2)R as the path has it (kernels_batch_split.h, kernels_batch_rows.h) ...
//   k_batch_head_xrows   own rows: rs[k] = sum_c Xh[k, c]^2 in ascending c
//   k_batch_head_x       one workgroup per entry range, as k_batch_split_x: the trace from rs, the diagonal from rs, the rest as there
//
// Kernel boundaries are the only synchronisation: no atomics, no spin-wait, no grid barrier.  One writer per address per launch, and
// no workgroup reads what another writes in the same launch: avg writes rs and e_this on own rows (own pairs) and dual reads rs one
// launch later; fold is the only reader and writer of e_accu, Y and wH in its launch; loss writes lval on the entries of own rows and
// reads lval on those same entries only, after a barrier of its own workgroup; xrows writes rs on own rows and x reads it one launch later.
//
// Why the bits do not change.  Per-entry and per-row statements do not depend on who owns the entry or the row: they are restated
// from k_mmw_batch term by term.  A row's sum (rs, eH, the plan's o, the row sums of X_half) runs over its CSR entries, or its
// columns, in order.  Every cross-thread sum -- tot, sD, sF, sW of the softmax, sd of the plan, the trace -- stays on one workgroup
// with the single launch's thread map (c = tid, k = tid, stride 512) and block_sum; the maxima (the softmax shift, pp, pm) are fmax
// folds, which are exact.  tests/test_hip_batch_head.py holds the two statements together, bitwise.
//
// The work table (HeadWork), the records of the LOSS constant and the (dg, o) scratch live in buffers of the split's own: the arenas
// and their layout are those of the single-launch kernel.
#pragma once
#include "kernels_batch_rows.h"

namespace mmw {

constexpr int BATCH_MAX_HEAD_PARTS = MMW_BATCH_MAX_HEAD_PARTS;

// one workgroup of k_batch_head_avg / dual / loss / xrows
struct HeadWork {
    int inst;    // instance of the batch
    int part;    // row part of the instance, of `parts`: its share of the E_asso pairs is [part * EA / parts, (part + 1) * EA / parts)
    int parts;   // row parts of the instance
    int r0, r1;  // own rows [r0, r1), possibly none
};

// ---- the gap row of iteration `it`, on the sums as the iteration before left them
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_gap(const BatchDesc* __restrict__ descs, const int* __restrict__ ia,
                                                                  double* __restrict__ fa, const GapDesc* __restrict__ gdescs,
                                                                  double* __restrict__ ga, int it) {
    const BatchDesc d = descs[blockIdx.x];
    if (it >= d.nrun) return;
    __shared__ double sh[BATCH_WAVES];
    const GapDesc g = gdescs[blockIdx.x];
    batch_gap_row(d, g, ia, fa, ga, d.iter0 + it, sh);
}

// ---- averaging and DUAL step 1 for the rows [r0, r1) and the part's share of the pairs
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_avg(const BatchDesc* __restrict__ descs, const HeadWork* __restrict__ work,
                                                                  const int* __restrict__ ia, double* __restrict__ fa, int it) {
    const HeadWork w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, EA = d.E_asso, baseH = K + EA;
    const int r0 = w.r0, r1 = w.r1;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ diag = ia + d.o_diag;
    const int* __restrict__ apos = ia + d.o_apos;
    const double* __restrict__ xval = fa + d.o_xval;
    const double* __restrict__ Y = fa + d.o_Y;
    double* __restrict__ xavg = fa + d.o_xavg;
    double* __restrict__ yavg = fa + d.o_yavg;
    double* __restrict__ eth = fa + d.o_ethis;
    double* __restrict__ rs = fa + d.o_rsum;
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1);
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    for (int e = indptr[r0] + tid; e < indptr[r1]; e += NT) xavg[e] += xval[e];
    for (int k = r0 + tid; k < r1; k += NT) {
        const int dp = diag[k];
        double s = 0.0;
        for (int e = indptr[k]; e < indptr[k + 1]; ++e)
            if (e != dp) s += xval[e];
        rs[k] = s;
        eth[k] = (xval[dp] - 1.0) * (1.0 / (1.0 - invK));
        yavg[k] += Y[k];
        yavg[baseH + k] += Y[baseH + k];
    }
    const int p0 = (int)((int64_t)w.part * EA / w.parts), p1 = (int)((int64_t)(w.part + 1) * EA / w.parts);
    for (int p = p0 + tid; p < p1; p += NT) {
        eth[K + p] = (xval[apos[p]] + 1.0 / Zm1) / denF;
        yavg[K + p] += Y[K + p];
    }
}

// ---- DUAL step 2 for the rows [r0, r1)
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_dual(const BatchDesc* __restrict__ descs, const HeadWork* __restrict__ work,
                                                                   const int* __restrict__ ia, double* __restrict__ fa, int it) {
    const HeadWork w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, baseH = K + d.E_asso;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const double* __restrict__ sab = fa + d.o_sab;
    const double* __restrict__ hmax = fa + d.o_hmax;
    const double* __restrict__ ssum = fa + d.o_ssum;
    const double* __restrict__ invn = fa + d.o_invn;
    const double* __restrict__ rs = fa + d.o_rsum;
    double* __restrict__ eth = fa + d.o_ethis;
    const double Zm1 = (double)(Z - 1);
    for (int k = w.r0 + tid; k < w.r1; k += NT) {
        double s = 0.0;
        for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
            const double wt = sab[e];
            if (wt != 0.0) s += wt * rs[col[e]];
        }
        eth[baseH + k] = (s * Zm1 / (double)Z - (hmax[k] - (1.0 / (double)Z) * ssum[k])) * invn[k];
    }
}

// ---- e_accu, the softmax and the LOSS constant of one instance (k_batch_split_head's loops and reductions), dconst into dcon[instance]
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_fold(const BatchDesc* __restrict__ descs, double* __restrict__ fa,
                                                                   double* __restrict__ dcon, int it) {
    const BatchDesc d = descs[blockIdx.x];
    if (it >= d.nrun) return;
    __shared__ double sh[BATCH_WAVES];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, C = d.C, baseH = K + d.E_asso;
    const double* __restrict__ invn = fa + d.o_invn;
    const double* __restrict__ cH = fa + d.o_cH;
    const double* __restrict__ eth = fa + d.o_ethis;
    double* __restrict__ Y = fa + d.o_Y;
    double* __restrict__ eacc = fa + d.o_eaccu;
    double* __restrict__ wH = fa + d.o_wH;
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1), eta = d.eta;
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    double best = -1e300;
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
            const double wt = y * invn[c - baseH];
            wH[c - baseH] = wt;
            sW += cH[c - baseH] * wt;
        }
    }
    sD = block_sum(sD, sh);
    sF = block_sum(sF, sh);
    sW = block_sum(sW, sh);
    const double dconst = -(sD * invK) / (1.0 - invK) + (sF / ((double)K * Zm1)) / denF - sW;
    if (tid == 0) dcon[blockIdx.x] = dconst;
}

// ---- LOSS on the entries of the rows [r0, r1), then the plan's per-row diagonal and off-diagonal sum of L/2 for those rows
// scr: the instance's scratch at soff[instance], dg[K] then o[K]
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_loss(const BatchDesc* __restrict__ descs, const HeadWork* __restrict__ work,
                                                                   const int* __restrict__ ia, double* __restrict__ fa,
                                                                   const double* __restrict__ dcon, const int64_t* __restrict__ soff,
                                                                   double* __restrict__ scr, int it) {
    const HeadWork w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, Z = d.Z, nnz = d.nnzL;
    const int r0 = w.r0, r1 = w.r1;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const int* __restrict__ pid = ia + d.o_pid;
    const double* __restrict__ sab = fa + d.o_sab;
    const double* __restrict__ sba = sab + nnz;
    const double* __restrict__ Y = fa + d.o_Y;
    const double* __restrict__ wH = fa + d.o_wH;
    double* lval = fa + d.o_lval;
    double* __restrict__ sdg = scr + soff[w.inst];
    double* __restrict__ so = sdg + K;
    const double invK = 1.0 / (double)K, Zm1 = (double)(Z - 1), eta = d.eta;
    const double denF = 1.0 / ((double)K * Zm1) + 0.5;
    const double dconst = dcon[w.inst];
    const double gscale = Zm1 / (double)(2 * Z);
    for (int e = indptr[r0] + tid; e < indptr[r1]; e += NT) {
        const int r = lrow[e], c = col[e], q = pid[e];
        double add;
        if (c == r) add = Y[r] / (1.0 - invK) + dconst;
        else if (q >= 0) add = (Y[K + q] * 0.5) / denF;
        else add = (sab[e] * wH[c] + sba[e] * wH[r]) * gscale;
        lval[e] = lval[e] - eta * add;
    }
    __syncthreads();  // the rows below read the entries other threads of this workgroup updated
    for (int k = r0 + tid; k < r1; k += NT) {
        double dg = 0.0, o = 0.0;
        for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
            const double v = 0.5 * lval[e];
            if (col[e] == k) dg = v;
            else o += fabs(v);
        }
        sdg[k] = dg;
        so[k] = o;
    }
}

// ---- k_batch_rows_plan with the pass over L replaced by the (dg, o) k_batch_head_loss left: the same thread map, reductions,
// plan_order, record, info writes and tally
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_plan(const BatchDesc* __restrict__ descs, double* __restrict__ fa,
                                                                   const int64_t* __restrict__ soff, const double* __restrict__ scr,
                                                                   double* __restrict__ rec, const int* __restrict__ prev_flags, int nsid,
                                                                   int* __restrict__ cnt, int it) {
    __shared__ double sh[BATCH_WAVES];
    if (blockIdx.x == 0 && prev_flags) rows_tally(prev_flags, nsid, cnt, sh);  // the last step launch of the iteration before
    const BatchDesc d = descs[blockIdx.x];
    if (it >= d.nrun) return;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K;
    const double* __restrict__ sdg = scr + soff[blockIdx.x];
    const double* __restrict__ so = sdg + K;
    double* __restrict__ info = fa + d.o_info;
    double sd = 0.0, pp = -1e300, pm = -1e300;
    for (int k = tid; k < K; k += NT) {
        const double dg = sdg[k], o = so[k];
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
    if (tid == 0) {
        double* r = rec + (size_t)ROWS_REC * blockIdx.x;
        r[0] = rho; r[1] = mu; r[2] = (double)nsub; r[3] = (double)mo;
        info[0] = rho; info[2] = (double)nsub; info[3] = mu;
    }
}

// ---- rs[k] = sum_c Xh[k, c]^2 for the rows [r0, r1)
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_xrows(const BatchDesc* __restrict__ descs, const HeadWork* __restrict__ work,
                                                                    double* __restrict__ fa, int it) {
    const HeadWork w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int D = d.D;
    const double* __restrict__ Xh = fa + d.o_Xh;
    double* __restrict__ rs = fa + d.o_rsum;
    for (int k = w.r0 + tid; k < w.r1; k += NT) {
        const double* y = Xh + (size_t)k * D;
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += y[c] * y[c];
        rs[k] = s;
    }
}

// ---- k_batch_split_x with the row sums read from rs: the trace by k_mmw_batch's thread map and block_sum, the diagonal from rs[r]
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_head_x(const BatchDesc* __restrict__ descs, const SplitRange* __restrict__ work,
                                                                const int* __restrict__ ia, double* __restrict__ fa,
                                                                const double* __restrict__ slab, int it) {
    const SplitRange w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    if (it >= d.nrun) return;
    const int64_t e0 = (int64_t)w.part * d.nnzL / w.nparts, e1 = (int64_t)(w.part + 1) * d.nnzL / w.nparts;
    if (e0 >= e1 && w.part != 0) return;  // an empty range (part 0 still owns the info record)
    __shared__ double sh[BATCH_WAVES];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, D = d.D;
    const int* __restrict__ col = ia + d.o_col;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const double* __restrict__ Xh = fa + d.o_Xh;
    const double* __restrict__ rs = fa + d.o_rsum;
    double* __restrict__ xval = fa + d.o_xval;
    double* __restrict__ info = fa + d.o_info;
    double dsum = 0.0;
    for (int k = tid; k < K; k += NT) dsum += rs[k];
    const double tr = block_sum(dsum, sh) / (double)K;
    const double itr = 1.0 / tr;
    for (int64_t e = e0 + tid; e < e1; e += NT) {
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
    if (w.part == 0 && tid == 0) {
        double ms = 0.0;
        for (int i = 0; i < w.nslab; ++i) ms = fmax(ms, slab[w.slab0 + i]);
        info[1] = ms;
    }
}

}  // namespace mmw
