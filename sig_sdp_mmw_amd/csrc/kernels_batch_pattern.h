// State processing on the device for MANY small instances, one workgroup per instance (mmw_batch_create_from_env): pattern_device.h
// restated for the layout a BatchEnv holds (BatchEnvDesc, kernels_batch_env.h: rx is K x A, the association, the sorted members of
// every AP) and for the two arenas the batched solver reads (BatchDesc, kernels_batch.h).
//
// The rules are pattern_device.h's.  With S_T'[a][j] = thr0(rx[j][asso[a]]) for asso[j] != asso[a] and Q[a][j] = 1 for j != a in the
// same AP, row a of L / X is {a} + {j : S_T'[a][j] != 0 or S_T'[j][a] != 0} + Q row a.  One wave per row scans the users in ascending
// order, 64 at a time, and compacts with ballots: rows come out sorted, there is no sort, no sparse transpose and no atomic.  Pair ids
// (triu-CSR order of Q) come from a user's position in its AP's member list.  S_sum and the squared row sums are computed by one
// thread per row in ascending column order with separately rounded products and sums, the roundings of the host build (pattern.h).
// rx is read by rows (rx[a][asso[j]], a gather inside one row) and by columns (rx[j][asso[a]], strided: at K, A <= 1024 the matrix
// stays in L2, and a dense transpose gives the same bits).
//
// k_batch_pattern_count: per row the length of L's pattern and the pairs above the user, with their prefix sums inside the workgroup in a
// fixed order (benv_scan); the totals of S_T' and of the upper gain edges (integer sums per wave, added in wave order); S_sum, the squared row sums and h_max beside them, so ONE readback
// brings the host everything it needs to lay out the arenas and to compute norm_H and cH (update_slots).
// k_batch_pattern_fill: the instance's slice of the int32 arena (indptr, col, lrow, pid, diag, apos), the pattern part of the fp64
// arena (sab, sba, h_max, S_sum; 1 / norm_H and cH from the call's upload, as k_batch_relayout places them), and the batch's own copy of
// the state's lists (S_gain, S_gain without its diagonal, Q_asso, h_max), which the environment rewrites at its next move.
// k_batch_pattern_init: the initial point, field by field what BatchCore::reset_one writes.
//
// Nothing waits across workgroups, no atomic, one writer per address: an instance is bitwise the same alone and among neighbours.
#pragma once
#include "kernels_batch.h"
#include "kernels_batch_env.h"
#include "pattern_device.h"

namespace mmw {

constexpr int BPAT_TOTALS = 4;  // ints per instance behind its l_indptr in the readback: nnzL, nnz(S_T'), E_gain, E_asso

// The count pass's buffers are laid out by the users before an instance (BatchEnvDesc::o_k) and its index b alone, so the pass needs
// no table of its own.  rb (read back): S_sum, the squared row sums and h_max of all users side by side (3 Ktot doubles), then, as
// int32, per instance l_indptr[K + 1] and the totals.  wi (stays on the device): per instance the users' positions in their APs'
// member lists [K] and the prefix sums of the pairs above a user [K + 1].
__host__ __device__ inline int64_t bpat_rb_doubles(int64_t Ktot, int64_t B) { return 3 * Ktot + (Ktot + (BPAT_TOTALS + 1) * B + 1) / 2; }
__host__ __device__ inline int64_t bpat_rb_int(int64_t o_k, int64_t b) { return o_k + (BPAT_TOTALS + 1) * b; }
__host__ __device__ inline int64_t bpat_wi_ints(int64_t Ktot, int64_t B) { return 2 * Ktot + B; }
__host__ __device__ inline int64_t bpat_wi(int64_t o_k, int64_t b) { return 2 * o_k + b; }

// where the batch keeps its own copy of an instance's state (int32 buffer: c_*, fp64 buffer: v_*) and its values in the call's
// scalar arrays
struct BatchPatItem {
    int64_t o_scal;                                         // the instance's K values in 1 / norm_H and in cH of the upload
    int64_t c_sptr, c_soptr, c_qptr, c_sidx, c_soidx, c_qidx;
    int64_t v_hmax, v_sval, v_soval, v_sohmax, v_qval;
};

// what a lane sees of (row a, user j)
struct BpatCell {
    double vab, vba;  // S_T'[a][j], S_T'[j][a]
    bool same;        // same AP (j == a included)
    bool inL;
};
__device__ __forceinline__ BpatCell bpat_cell(int a, int aa, int j, int K, int A, double thr, const double* __restrict__ rx, const int* __restrict__ asso) {
    BpatCell c{0.0, 0.0, false, false};
    if (j >= K) return c;
    const int aj = asso[j];
    c.same = aj == aa;
    if (!c.same) {
        c.vab = pat_thr0(rx[(size_t)j * A + aa], thr);
        c.vba = pat_thr0(rx[(size_t)a * A + aj], thr);
    }
    c.inL = c.same || c.vab != 0.0 || c.vba != 0.0;
    return c;
}
// S_sum and the squared row sum of row k of S_T' (mmw.py:34,37-39 as pattern.h evaluates them): the stored entries in ascending
// column order, products and sums rounded separately
__device__ __forceinline__ void bpat_rowstats(int k, int K, int A, double thr, const double* __restrict__ rx, const int* __restrict__ asso, double& s_out,
                                              double& q_out) {
#pragma clang fp contract(off)  // (a fused multiply-add would differ from the host's last bit)
    const int ak = asso[k];
    double s = 0.0, q = 0.0;
    for (int j = 0; j < K; ++j) {
        if (asso[j] == ak) continue;
        const double v = pat_thr0(rx[(size_t)j * A + ak], thr);
        if (v != 0.0) {
            const double vv = v * v;
            s = s + v;
            q = q + vv;
        }
    }
    s_out = s;
    q_out = q;
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_pattern_count(const BatchEnvDesc* __restrict__ edescs, double thr, const double* __restrict__ efa,
                                                                       const int* __restrict__ eia, int64_t Ktot, double* __restrict__ rb,
                                                                       int* __restrict__ wi) {
    const BatchEnvDesc d = edescs[blockIdx.x];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, A = d.A;
    const double* rx = efa + d.f_rx;
    const int* asso = eia + d.i_asso;
    const int* ap_cnt = eia + d.i_apcnt;
    const int* ap_ptr = eia + d.i_apptr;
    const int* ap_mem = eia + d.i_apmem;
    int* l_ptr = reinterpret_cast<int*>(rb + 3 * Ktot) + bpat_rb_int(d.o_k, blockIdx.x);
    int* appos = wi + bpat_wi(d.o_k, blockIdx.x);
    int* qu_ptr = appos + K;
    __shared__ int s_tot[2][BATCH_WAVES];  // per wave: entries of S_T', upper gain edges
    // position of every user in its AP's ascending member list
    for (int a = wv; a < A; a += BATCH_WAVES)
        for (int i = ap_ptr[a] + lane; i < ap_ptr[a + 1]; i += WAVE) appos[ap_mem[i]] = i - ap_ptr[a];
    __syncthreads();
    int cS = 0, cG = 0;
    for (int a = wv; a < K; a += BATCH_WAVES) {
        const int aa = asso[a];
        int cL = 0;
        for (int j0 = 0; j0 < K; j0 += WAVE) {
            const int j = j0 + lane;
            const BpatCell c = bpat_cell(a, aa, j, K, A, thr, rx, asso);
            cL += __popcll(__ballot(c.inL));
            cS += __popcll(__ballot(c.vab != 0.0));
            cG += __popcll(__ballot(j > a && (c.vab != 0.0 || c.vba != 0.0)));
        }
        if (lane == 0) {
            l_ptr[a] = cL;
            qu_ptr[a] = ap_cnt[aa] - appos[a] - 1;  // same-AP users above a: row a of triu(Q, 1)
        }
    }
    if (lane == 0) { s_tot[0][wv] = cS; s_tot[1][wv] = cG; }
    for (int k = tid; k < K; k += BATCH_THREADS) {
        double s, q;
        bpat_rowstats(k, K, A, thr, rx, asso, s, q);
        rb[d.o_k + k] = s;
        rb[Ktot + d.o_k + k] = q;
        rb[2 * Ktot + d.o_k + k] = efa[d.f_hmax + k];
    }
    __syncthreads();
    if (wv == 0) benv_scan(l_ptr, K);
    if (wv == 1) benv_scan(qu_ptr, K);
    __syncthreads();
    if (tid == 0) {
        int* t = l_ptr + K + 1;
        t[0] = l_ptr[K];
        t[1] = t[2] = 0;
        for (int w = 0; w < BATCH_WAVES; ++w) { t[1] += s_tot[0][w]; t[2] += s_tot[1][w]; }
        t[3] = qu_ptr[K];
    }
}

__device__ __forceinline__ void bpat_copy(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
    for (int64_t i = threadIdx.x; i < n; i += BATCH_THREADS) dst[i] = src[i];
}
__device__ __forceinline__ void bpat_copy(int* __restrict__ dst, const int* __restrict__ src, int64_t n) {
    for (int64_t i = threadIdx.x; i < n; i += BATCH_THREADS) dst[i] = src[i];
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_pattern_fill(const BatchEnvDesc* __restrict__ edescs, const BatchDesc* __restrict__ descs,
                                                                      const BatchPatItem* __restrict__ items, double thr, const double* __restrict__ efa,
                                                                      const int* __restrict__ eia, int64_t Ktot, const double* __restrict__ rb,
                                                                      const int* __restrict__ wi, const double* __restrict__ invn,
                                                                      const double* __restrict__ cH, int* __restrict__ ia, double* __restrict__ fa,
                                                                      int* __restrict__ si, double* __restrict__ sf) {
    const BatchEnvDesc e = edescs[blockIdx.x];
    const BatchDesc& d = descs[blockIdx.x];
    const BatchPatItem t = items[blockIdx.x];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = e.K, A = e.A;
    const int64_t nnz = d.nnzL;
    const double* rx = efa + e.f_rx;
    const int* asso = eia + e.i_asso;
    const int* l_ptr = reinterpret_cast<const int*>(rb + 3 * Ktot) + bpat_rb_int(e.o_k, blockIdx.x);
    const int* appos = wi + bpat_wi(e.o_k, blockIdx.x);
    const int* qu_ptr = appos + K;
    int* col = ia + d.o_col;
    int* lrow = ia + d.o_lrow;
    int* pid = ia + d.o_pid;
    int* diag = ia + d.o_diag;
    int* apos = ia + d.o_apos;
    double* sab = fa + d.o_sab;
    double* sba = sab + nnz;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int a = wv; a < K; a += BATCH_WAVES) {
        const int aa = asso[a], pa = appos[a];
        int oL = l_ptr[a];
        for (int j0 = 0; j0 < K; j0 += WAVE) {
            const int j = j0 + lane;
            const BpatCell c = bpat_cell(a, aa, j, K, A, thr, rx, asso);
            const unsigned long long mL = __ballot(c.inL);
            if (c.inL) {
                const int en = oL + __popcll(mL & below);
                col[en] = j;
                lrow[en] = a;
                sab[en] = c.vab;
                sba[en] = c.vba;
                int id = -1;
                if (c.same && j != a) {  // pair (lo, hi) in the triu-CSR order of Q: row lo, its same-AP users above it in ascending order
                    const int pj = appos[j];
                    const int lo = j > a ? a : j, plo = j > a ? pa : pj, phi = j > a ? pj : pa;
                    id = qu_ptr[lo] + (phi - plo - 1);
                    if (j > a) apos[id] = en;
                }
                pid[en] = id;
                if (j == a) diag[a] = en;
            }
            oL += __popcll(mL);
        }
    }
    bpat_copy(ia + d.o_indptr, l_ptr, (int64_t)K + 1);
    bpat_copy(fa + d.o_hmax, rb + 2 * Ktot + e.o_k, K);
    bpat_copy(fa + d.o_ssum, rb + e.o_k, K);
    bpat_copy(fa + d.o_invn, invn + t.o_scal, K);
    bpat_copy(fa + d.o_cH, cH + t.o_scal, K);
    // the batch's own copy of the state: the environment's lists are rewritten by its next move
    const int64_t ns = eia[e.i_sptr + K], no = eia[e.i_soptr + K], nq = eia[e.i_qptr + K];
    bpat_copy(si + t.c_sptr, eia + e.i_sptr, (int64_t)K + 1);
    bpat_copy(si + t.c_soptr, eia + e.i_soptr, (int64_t)K + 1);
    bpat_copy(si + t.c_qptr, eia + e.i_qptr, (int64_t)K + 1);
    bpat_copy(si + t.c_sidx, eia + e.i_sidx, ns);
    bpat_copy(si + t.c_soidx, eia + e.i_soidx, no);
    bpat_copy(si + t.c_qidx, eia + e.i_qidx, nq);
    bpat_copy(sf + t.v_hmax, efa + e.f_hmax, K);
    bpat_copy(sf + t.v_sval, efa + e.f_sval, ns);
    bpat_copy(sf + t.v_soval, efa + e.f_soval, no);
    bpat_copy(sf + t.v_sohmax, efa + e.f_sohmax, no);
    bpat_copy(sf + t.v_qval, efa + e.f_qval, nq);
}

// The reference's initial point (mmw.py:62-73) as BatchCore::reset_one writes it: the iterate (lval ... W2) zero, X = I on the
// pattern, Y = y0[b] (1.0 / (double)C, divided on the host).  Like reset_one it leaves the plan's record (info) alone: creation has
// cleared the whole arena (clear == 0: nothing to zero again), and a reset (clear == 1) keeps the last plan readable.
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_pattern_init(const BatchDesc* __restrict__ descs, const double* __restrict__ y0,
                                                                      const int* __restrict__ ia, double* __restrict__ fa, int clear) {
    const BatchDesc& d = descs[blockIdx.x];
    if (clear) {
        for (int64_t i = threadIdx.x; i < d.o_info - d.o_lval; i += BATCH_THREADS) fa[d.o_lval + i] = 0.0;
        __syncthreads();
    }  // the values below land in the span just cleared
    const int* __restrict__ diag = ia + d.o_diag;
    for (int k = threadIdx.x; k < d.K; k += BATCH_THREADS) fa[d.o_xval + diag[k]] = 1.0;
    const double y = y0[blockIdx.x];
    for (int c = threadIdx.x; c < d.C; c += BATCH_THREADS) fa[d.o_Y + c] = y;
}

}  // namespace mmw
