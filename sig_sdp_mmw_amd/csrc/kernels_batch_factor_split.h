// The factor of a batched probe spread over several workgroups per instance (mmw_batch_set_factor_split): k_batch_factor
// (kernels_batch_epilogue.h) as a chain of launches for all taking instances together, the kernel boundaries being the only
// synchronisation -- no atomics, no spin-wait, no grid barrier, one stream.
//
//   k_batch_factor_head    one workgroup per instance: Xbar scattered into the dense work matrix; the instance's slots and record cleared
//   k_batch_factor_round   one launch per tournament round r, one workgroup per item {instance, first pair, pair count}
//   k_batch_factor_sweep   one workgroup per instance after the last round of a sweep: the items' {rotations, |cos|} into the record
//   k_batch_factor_tail    one workgroup per instance: row norms, the rank cut by counting, X_half, MMW_F_FACTOR_INFO's record
// (FactorDesc::kind == 1, mmw_batch_factor_spectral: the head builds the state's Laplacian and the tail the row-normalised eigenvector
// block instead, kernels_batch_spectral.h; the rounds and the sweep records do not know the difference)
//
// Why the bits do not change.  A round of the tournament is ceil(K / 2) disjoint row pairs; a pair is reduced and rotated by one
// wave -- per-lane sums in ascending column order, the fixed-order wave reduction -- so what it computes does not depend on the wave
// or the workgroup that takes it.  Across pairs a sweep shares its rotation count (an integer sum) and its largest |cos| (an fmax):
// both exact in any order.  The workgroup barrier that ends a round in k_batch_factor is a kernel boundary here.  Every statement
// below restates k_batch_factor's term by term; tests/test_hip_batch_factor_split.py holds the two together, bitwise.
//
// The item table, the spans, the slab of per-item sums and the sweep records live in buffers of their own: ew / ei keep the layout
// mmw_batch_factor gives them, and the factor, the norms, the order and the record lie where k_batch_round and the reads expect them.
#pragma once
#include "kernels_batch_epilogue.h"

namespace mmw {

// one workgroup of k_batch_factor_round
struct FactorItem {
    int inst;    // taking instance of the call (index into the call's FactorDesc table)
    int p0, np;  // its pairs of every round: [p0, p0 + np)
    int rounds;  // rounds of the instance's tournament; the table is sorted by it, descending: the grid shrinks as r grows
    int slot;    // the item's own pair of doubles in the slab
};
// the items of one taking instance: slots [slot0, slot0 + nitems), in item order
struct FactorSpan {
    int slot0, nitems;
};
constexpr int FSPLIT_SLOT = 2;  // doubles per slab slot: {rotations, largest |cos|} of the item in the sweep under way
constexpr int FSPLIT_REC = 4;   // doubles per sweep record: {rotations, largest |cos|} of the last sweep, sweeps so far, ended (0 / 1)

// The tournament: n = K + (K & 1) players (index K is the bye of an odd K), n - 1 rounds of P = n / 2 disjoint pairs.
inline int factor_rounds(int K) { return K + (K & 1) - 1; }
inline int factor_pairs(int K) { return (K + (K & 1)) / 2; }
// Items of an instance: contiguous ranges of ceil(P / parts) pairs, G = ceil(P / that) <= parts of them, none empty.
inline int factor_item_pairs(int K, int parts) { return (factor_pairs(K) + parts - 1) / parts; }
inline int factor_item_count(int K, int parts) {
    const int per = factor_item_pairs(K, parts);
    return (factor_pairs(K) + per - 1) / per;
}

// ---- Xbar, dense (k_batch_factor, same statements); the instance's slab slots and its sweep record start at zero
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_factor_head(const FactorDesc* __restrict__ descs, const FactorSpan* __restrict__ spans,
                                                                     const int* __restrict__ ia, const double* __restrict__ fa, double* ew,
                                                                     double* __restrict__ slab, double* __restrict__ rec,
                                                                     const int* __restrict__ si, const double* __restrict__ sf) {
    const FactorDesc d = descs[blockIdx.x];
    const FactorSpan sp = spans[blockIdx.x];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const int* __restrict__ col = ia + d.o_col;
    const double* src = (d.src_work ? ew : fa) + d.o_src;
    double* A = ew + d.o_A;
    if (d.kind == 1) {  // (workgroup-uniform) the Laplacian of the state instead of Xbar
        spectral_head(K, si + d.s_soptr, si + d.s_soidx, sf + d.s_sodata, A);
    } else {
        const size_t KK = (size_t)K * K;
        for (size_t i = tid; i < KK; i += NT) A[i] = 0.0;
        __syncthreads();
        for (int e = tid; e < d.nnzL; e += NT) A[(size_t)lrow[e] * K + col[e]] = src[e] / d.div;
    }
    for (int i = tid; i < sp.nitems * FSPLIT_SLOT; i += NT) slab[(size_t)sp.slot0 * FSPLIT_SLOT + i] = 0.0;
    if (tid < FSPLIT_REC) rec[(size_t)blockIdx.x * FSPLIT_REC + tid] = 0.0;
}

// The pair step of epi_jacobi (same statements): the two row pairs (pr[u], qr[u]) (pr[u] < 0: none, or the bye) of A, NE = elements of
// a row per lane; `rot` counts the rotations made, `cmax` keeps the largest |cos| met.
template <int NE>
__device__ __forceinline__ void factor_pair_step(double* A, int K, const int (&pr)[2], const int (&qr)[2], int lane, int& rot, double& cmax) {
    double x[2][2][NE];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const double* P = A + (size_t)(pr[u] < 0 ? 0 : pr[u]) * K;
        const double* Q = A + (size_t)(qr[u] < 0 ? 0 : qr[u]) * K;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int c = lane + WAVE * i;
            const bool in = pr[u] >= 0 && c < K;
            x[u][0][i] = in ? P[c] : 0.0;
            x[u][1][i] = in ? Q[c] : 0.0;
        }
    }
    double al[2], be[2], ga[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            a += x[u][0][i] * x[u][0][i];
            b += x[u][1][i] * x[u][1][i];
            g += x[u][0][i] * x[u][1][i];
        }
        al[u] = wave_sum(a);
        be[u] = wave_sum(b);
        ga[u] = wave_sum(g);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (pr[u] < 0) continue;
        const double nn = sqrt(al[u] * be[u]);
        if (nn > 0.0) cmax = fmax(cmax, fabs(ga[u]) / nn);  // as met, before the rotation: skipped pairs count too
        if (!(fabs(ga[u]) > EPI_ROT_TOL * nn)) continue;  // (wave-uniform: every lane holds the same sums)
        const double zeta = (be[u] - al[u]) / (2.0 * ga[u]);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        double* P = A + (size_t)pr[u] * K;
        double* Q = A + (size_t)qr[u] * K;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int col = lane + WAVE * i;
            if (col < K) {
                P[col] = c * x[u][0][i] - s * x[u][1][i];
                Q[col] = s * x[u][0][i] + c * x[u][1][i];
            }
        }
        ++rot;
    }
}

// The pairs [p0, p1) of round r, 16 at a time as epi_jacobi walks a whole round: wave w takes the pairs pi and pi + 8.
template <int NE>
__device__ __forceinline__ void factor_round_pairs(double* A, int K, int r, int p0, int p1, int& rot, double& cmax) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int n = K + (K & 1), m = n - 1;  // players (index K is the bye of an odd K), rounds
    for (int pi = p0 + wv; pi < p1; pi += 2 * BATCH_WAVES) {
        int pr[2], qr[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pj = pi + u * BATCH_WAVES;
            int a = -1, b = -1;
            if (pj < p1) {
                if (pj == 0) { a = m; b = r; }
                else { a = r + pj; a = a >= m ? a - m : a; b = r - pj; b = b < 0 ? b + m : b; }
                if (a >= K || b >= K) a = b = -1;
            }
            pr[u] = a < b ? a : b;
            qr[u] = a < b ? b : a;
        }
        factor_pair_step<NE>(A, K, pr, qr, lane, rot, cmax);
    }
}

// ---- round r of the sweep under way, for the item's pairs
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_factor_round(const FactorDesc* __restrict__ descs, const FactorItem* __restrict__ items,
                                                                      double* ew, double* __restrict__ slab, const double* __restrict__ rec, int r) {
    const FactorItem w = items[blockIdx.x];
    if (r >= w.rounds) return;
    if (rec[(size_t)w.inst * FSPLIT_REC + 3] != 0.0) return;  // the instance has ended
    __shared__ int s_rot[BATCH_WAVES];
    __shared__ double s_cos[BATCH_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = descs[w.inst].K;
    double* A = ew + descs[w.inst].o_A;
    const int p0 = w.p0, p1 = w.p0 + w.np;
    int rot = 0;
    double cmax = 0.0;
    if (K <= 4 * WAVE) factor_round_pairs<4>(A, K, r, p0, p1, rot, cmax);
    else if (K <= 8 * WAVE) factor_round_pairs<8>(A, K, r, p0, p1, rot, cmax);
    else if (K <= 12 * WAVE) factor_round_pairs<12>(A, K, r, p0, p1, rot, cmax);
    else factor_round_pairs<16>(A, K, r, p0, p1, rot, cmax);
    if (lane == 0) { s_rot[wv] = rot; s_cos[wv] = cmax; }
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        double cm = 0.0;
        for (int v = 0; v < BATCH_WAVES; ++v) { tot += s_rot[v]; cm = fmax(cm, s_cos[v]); }
        double* s = slab + (size_t)w.slot * FSPLIT_SLOT;  // the item's own slot: one writer per launch
        s[0] += (double)tot;                               // (a count below 2^53: exact)
        s[1] = fmax(s[1], cm);
    }
}

// ---- the end of a sweep: the instance's slots, in item order, into its record; the slots are cleared for the next sweep.  The
// instance ends on a sweep without a rotation or at the sweep cap (epi_jacobi's rule); the host reads the records and does the same.
__global__ __launch_bounds__(WAVE) void k_batch_factor_sweep(const FactorDesc* __restrict__ descs, const FactorSpan* __restrict__ spans,
                                                             double* __restrict__ slab, double* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    double* rc = rec + (size_t)blockIdx.x * FSPLIT_REC;
    if (rc[3] != 0.0) return;
    const FactorSpan sp = spans[blockIdx.x];
    double rot = 0.0, cm = 0.0;
    for (int i = 0; i < sp.nitems; ++i) {
        double* s = slab + (size_t)(sp.slot0 + i) * FSPLIT_SLOT;
        rot += s[0];
        cm = fmax(cm, s[1]);
        s[0] = 0.0;
        s[1] = 0.0;
    }
    const double sweeps = rc[2] + 1.0;
    rc[0] = rot;
    rc[1] = cm;
    rc[2] = sweeps;
    rc[3] = (rot == 0.0 || sweeps >= (double)descs[blockIdx.x].cap) ? 1.0 : 0.0;
}

// ---- singular values = row norms, ranked by counting; X_half; the record (k_batch_factor, same statements)
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_factor_tail(const FactorDesc* __restrict__ descs, const double* __restrict__ rec, double* ew,
                                                                     int* __restrict__ ei) {
    const FactorDesc d = descs[blockIdx.x];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, rank = d.rank;
    double* A = ew + d.o_A;
    double* fac = ew + d.o_fac;
    double* nrm = ew + d.o_nrm;
    int* ord = ei + d.o_ord;
    const int sweeps = (int)rec[(size_t)blockIdx.x * FSPLIT_REC + 2];
    const double lastcos = rec[(size_t)blockIdx.x * FSPLIT_REC + 1];
    for (int row = wv; row < K; row += BATCH_WAVES) {
        double s = 0.0;
        for (int c = lane; c < K; c += WAVE) {
            const double v = A[(size_t)row * K + c];
            s += v * v;
        }
        s = wave_sum(s);
        if (lane == 0) nrm[row] = sqrt(s);
    }
    __syncthreads();
    for (int k = tid; k < K; k += NT) {
        const double mine = nrm[k];
        int r = 0;
        for (int j = 0; j < K; ++j) {
            const double o = nrm[j];
            r += (o > mine) || (o == mine && j < k);
        }
        ord[r] = k;
    }
    __syncthreads();
    if (d.kind == 1) {  // the eigenvector block, rows normalised, instead of U sqrt(S)
        spectral_tail(K, rank, A, nrm, ord, fac, ew + d.o_rown);
    } else {
        const size_t KR = (size_t)K * rank;
        for (size_t idx = tid; idx < KR; idx += NT) {
            const int i = (int)(idx / rank), j = (int)(idx % rank);
            const int row = ord[rank - 1 - j];
            const double nv = nrm[row];
            fac[idx] = nv > 0.0 ? A[(size_t)row * K + i] / sqrt(nv) : 0.0;
        }
    }
    if (tid == 0) {
        double* info = ew + d.o_info;
        info[0] = (double)sweeps;
        info[1] = lastcos;
        info[2] = (double)rank;
        info[3] = nrm[ord[rank - 1]];
        info[4] = rank < K ? nrm[ord[rank]] : 0.0;
    }
}

}  // namespace mmw
