// The rows of a Taylor term spread over workgroups (mmw_batch_set_row_split): exp(L/2)R of kernels_batch_split.h's k_batch_split_expm
// as one launch per term, each with one workgroup per (instance, column slice, row part).  An iteration is
//
//   k_batch_split_head   unchanged, one workgroup per instance
//   k_batch_rows_plan    one workgroup per instance: (mu, rho, substeps, order) into a record the host reads -- the one
//                        synchronisation of the iteration; the host then knows how many launches follow
//   k_batch_rows_step    launch l = s (1 + mo) + j of the instance's schedule: j = 0 starts substep s (s = 0: the sketch, F = T0 = R;
//                        s > 0: F *= e^{mu / nsub}, T0 = F), j >= 1 is term j.  One launch serves all instances, each at its own (s, j);
//                        a workgroup past its instance's nsub (1 + mo) launches, or whose slice has no live column, returns at once
//   k_batch_split_x      unchanged, with slices x row parts entry ranges per instance
//
// Kernel boundaries are the only synchronisation: no atomics, no spin-wait, no grid barrier.  One writer per address per launch, and no
// workgroup reads what another writes in the same launch: a term reads the T buffer the launch before wrote (all rows) and writes the
// other one (own rows); F is read and written on own rows only; the per-part column maxima go to a slab of the launch's parity and are
// folded by every workgroup of the slice in the next launch; the per-column stop state (c_prev, c_on) is a copy of the workgroup's own.
//
// Why the bits do not change.  A row's sum runs over its CSR entries in order, whichever workgroup owns the row; the stop rule is
// built from fmax only (exact, so neither the row parts nor the thread map matter); the plan uses k_mmw_batch's thread map and block
// reductions; the sketch's row norm comes from the whole row; the final e^{mu / nsub} scaling of a column multiplies the same F by the
// same factor, in the launch that finds the column stopped (or in the last term of the schedule).  Each phase restates the expressions
// of k_mmw_batch term by term; tests/test_hip_batch_rows.py holds the two statements together, bitwise.
#pragma once
#include "kernels_batch_split.h"

namespace mmw {

constexpr int BATCH_MAX_ROW_PARTS = MMW_BATCH_MAX_ROW_PARTS;

// one workgroup of k_batch_rows_step
struct RowsWork {
    int inst;    // instance of the batch
    int slice;   // column slice: columns [slice * width, min(D, (slice + 1) * width))
    int width;   // columns per slice (the last may be narrower)
    int rpart;   // row part of the slice, of `rows`
    int rows;    // row parts of the instance
    int r0, r1;  // own rows [r0, r1), possibly none
    int sbase;   // the slice's block in a slab: part p, local column c at sbase + p * width + c
    int sid;     // the slice's index among all slices of the launch: its Taylor degree and its live flag
};

// plan record of an instance: 4 doubles
constexpr int ROWS_REC = 4;  // {rho, mu, nsub, mo}

// The tally of a launch's live flags (one per slice, written by its row part 0): a launch in which no slice had work counts as idle.
__device__ __forceinline__ void rows_tally(const int* __restrict__ flags, int nsid, int* __restrict__ cnt, double* sh) {
    double any = 0.0;
    for (int i = (int)threadIdx.x; i < nsid; i += (int)blockDim.x) any = fmax(any, (double)flags[i]);
    any = block_max(any, sh);
    if (threadIdx.x == 0 && any == 0.0) cnt[0] += 1;
}

// ---- the plan of exp(A) R, A = L/2 (k_mmw_batch's statements, thread map and reductions) into the instance's record and EXPM_INFO[0,2,3]
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_rows_plan(const BatchDesc* __restrict__ descs, const int* __restrict__ ia,
                                                                   double* __restrict__ fa, double* __restrict__ rec,
                                                                   const int* __restrict__ prev_flags, int nsid, int* __restrict__ cnt, int it) {
    __shared__ double sh[BATCH_WAVES];
    if (blockIdx.x == 0 && prev_flags) rows_tally(prev_flags, nsid, cnt, sh);  // the last step launch of the iteration before
    const BatchDesc d = descs[blockIdx.x];
    if (it >= d.nrun) return;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const double* __restrict__ lval = fa + d.o_lval;
    double* __restrict__ info = fa + d.o_info;
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
    if (tid == 0) {
        double* r = rec + (size_t)ROWS_REC * blockIdx.x;
        r[0] = rho; r[1] = mu; r[2] = (double)nsub; r[3] = (double)mo;
        info[0] = rho; info[2] = (double)nsub; info[3] = mu;
    }
}

// batch_sketch_rows (kernels_batch.h) for the rows [r0, r1): every row drawn whole, the columns [c0, c1) written
__device__ __forceinline__ void rows_sketch(int r0, int r1, int D, uint64_t seed, uint32_t iter, double* __restrict__ R, int c0, int c1) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int ngroups = (D + 1) >> 1;
    for (int row = r0 + wib; row < r1; row += nw) {
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

// ---- launch l of the schedules: the start of a substep or one Taylor term, for the rows [r0, r1) and the columns of one slice
// slab_t / slab_f: 2 x nslab doubles (by launch parity) of per-part column maxima of |t| and |F|; st_prev / st_on: nslab entries, the
// workgroup's own copy of the slice's stop state; deg: the slices' Taylor degrees (k_batch_split_x's slab); flags: 2 x nsid live flags.
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_rows_step(const BatchDesc* __restrict__ descs, const RowsWork* __restrict__ work,
                                                                   const double* __restrict__ rec, const int* __restrict__ ia,
                                                                   double* __restrict__ fa, const double* __restrict__ randv,
                                                                   double* __restrict__ slab_t, double* __restrict__ slab_f,
                                                                   double* __restrict__ st_prev, int* __restrict__ st_on,
                                                                   double* __restrict__ deg, int* __restrict__ flags, int* __restrict__ cnt,
                                                                   int nslab, int nsid, int it, int l) {
    __shared__ double sh[BATCH_WAVES];
    __shared__ double red_a[BATCH_THREADS], red_b[BATCH_THREADS];
    __shared__ int c_on[BATCH_MAX_D], c_off[BATCH_MAX_D];  // column still adds terms; column found stopped in this launch
    const int par = l & 1;
    if (blockIdx.x == 0 && l > 0) rows_tally(flags + (size_t)(par ^ 1) * nsid, nsid, cnt, sh);
    const RowsWork w = work[blockIdx.x];
    const BatchDesc d = descs[w.inst];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const bool head = w.rpart == 0 && tid == 0;  // the slice's one writer of its degree and its live flag
    int* const flag = flags + (size_t)par * nsid + w.sid;
    if (it >= d.nrun) {
        if (head) *flag = 0;
        return;
    }
    const double* rc = rec + (size_t)ROWS_REC * w.inst;
    const double mu = rc[1];
    const int nsub = (int)rc[2], mo = (int)rc[3];
    if (l >= nsub * (1 + mo)) {  // past this instance's schedule
        if (head) *flag = 0;
        return;
    }
    const int s = l / (1 + mo), j = l % (1 + mo);
    const int K = d.K, D = d.D;
    const int c0 = w.slice * w.width, c1 = c0 + w.width < D ? c0 + w.width : D, Ds = c1 - c0;
    const int r0 = w.r0, r1 = w.r1;
    const int* __restrict__ indptr = ia + d.o_indptr;
    const int* __restrict__ col = ia + d.o_col;
    const double* __restrict__ lval = fa + d.o_lval;
    double* F = fa + d.o_Xh;
    double* R = fa + d.o_R;
    // T0 / T1 alternate by the instance's term count g = s mo + (j - 1): term g reads buffer g & 1 and writes the other; the start of
    // substep s writes the buffer its first term reads
    const int g = s * mo + (j > 0 ? j - 1 : 0);
    double* T0 = fa + ((g & 1) ? d.o_W2 : d.o_W1);
    double* T1 = fa + ((g & 1) ? d.o_W1 : d.o_W2);
    // the slice's thread map: column tc = c0 + tid % Ds, row group tg = tid / Ds of NG groups over the own rows
    const int NG = NT / Ds, lc = tid % Ds, tc = c0 + lc, tg = tid / Ds;
    const bool tlive = tg < NG;
    const size_t mine = (size_t)w.sbase + (size_t)w.rpart * w.width;
    double* const my_t = slab_t + (size_t)par * nslab + mine;
    double* const my_f = slab_f + (size_t)par * nslab + mine;
    const double* const prev_t = slab_t + (size_t)(par ^ 1) * nslab + w.sbase;
    const double* const prev_f = slab_f + (size_t)(par ^ 1) * nslab + w.sbase;
    const double scale_mu = exp(mu / (double)nsub);
    if (j == 0) {
        // ---- the start of substep s
        if (s == 0) {
            const int gi = d.iter0 + it;
            if (d.o_randv >= 0) {
                const double* src = randv + d.o_randv + (size_t)it * K * D;
                for (size_t i = tid; i < (size_t)(r1 - r0) * Ds; i += NT) {
                    const size_t at = (r0 + i / Ds) * D + c0 + i % Ds;
                    R[at] = src[at];
                }
            } else {
                rows_sketch(r0, r1, D, d.seed, (uint32_t)gi, R, c0, c1);
            }
            __syncthreads();
        }
        double fm = 0.0;
        if (tlive)
            for (int r = r0 + tg; r < r1; r += NG) {
                const size_t at = (size_t)r * D + tc;
                const double f = s == 0 ? R[at] : F[at] * scale_mu;
                F[at] = f;
                T0[at] = f;
                fm = fmax(fm, fabs(f));
            }
        red_a[tid] = fm;
        __syncthreads();
        for (int c = tid; c < Ds; c += NT) {
            double t = 0.0;
            for (int q = 0; q < NG; ++q) t = fmax(t, red_a[q * Ds + c]);
            my_f[c] = t;
        }
        if (head) {
            if (s == 0) deg[w.sid] = 0.0;
            *flag = 1;
        }
        return;
    }
    // ---- term j of substep s: the stop state of the slice's columns after term j - 1, from the slabs of the launch before
    for (int c = tid; c < Ds; c += NT) {
        double cp;
        int on, off = 0;
        if (j == 1) {
            cp = 0.0;
            for (int p = 0; p < w.rows; ++p) cp = fmax(cp, prev_f[(size_t)p * w.width + c]);
            on = 1;
        } else {
            cp = st_prev[mine + c];
            on = st_on[mine + c];
            if (on) {
                double t = 0.0, f = 0.0;
                for (int p = 0; p < w.rows; ++p) { t = fmax(t, prev_t[(size_t)p * w.width + c]); f = fmax(f, prev_f[(size_t)p * w.width + c]); }
                if (cp + t <= d.tol * f) { on = 0; off = 1; }
                cp = t;
            }
        }
        st_prev[mine + c] = cp;
        st_on[mine + c] = on;
        c_on[c] = on;
        c_off[c] = off;
    }
    __syncthreads();
    int any = 0, anyoff = 0;
    for (int c = 0; c < Ds; ++c) { any |= c_on[c]; anyoff |= c_off[c]; }
    if (head) *flag = any | anyoff;
    if (!any && !anyoff) return;  // every column of the slice had stopped before
    // the scaling that ends the last substep (k_mmw_batch: F *= e^{mu / nsub} after the term loop) is applied per column: here for
    // the columns found stopped, below for those that run the schedule's last term
    const bool fin = s + 1 == nsub && scale_mu != 1.0;
    if (fin && tlive && c_off[lc])
        for (int r = r0 + tg; r < r1; r += NG) F[(size_t)r * D + tc] = F[(size_t)r * D + tc] * scale_mu;
    if (!any) return;
    if (head && (double)j > deg[w.sid]) deg[w.sid] = (double)j;
    const double coef = 1.0 / ((double)nsub * (double)j);
    const bool last = fin && j == mo;
    double tmax = 0.0, fmx = 0.0;
    if (tlive && c_on[lc]) {
        for (int r = r0 + tg; r < r1; r += NG) {
            double acc = 0.0;
            for (int e = indptr[r]; e < indptr[r + 1]; ++e) acc += (0.5 * lval[e]) * T0[(size_t)col[e] * D + tc];
            const double t = (acc - mu * T0[(size_t)r * D + tc]) * coef;
            T1[(size_t)r * D + tc] = t;
            const double f = F[(size_t)r * D + tc] + t;
            F[(size_t)r * D + tc] = last ? f * scale_mu : f;
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
        for (int q = 0; q < NG; ++q) { t = fmax(t, red_a[q * Ds + c]); f = fmax(f, red_b[q * Ds + c]); }
        my_t[c] = t;
        my_f[c] = f;
    }
}

}  // namespace mmw
