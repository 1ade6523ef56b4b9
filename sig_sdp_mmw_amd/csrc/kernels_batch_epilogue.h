// The epilogue of a batched probe on the device: X_half of the averaged X (mmw.py:213-216) and the randomized rounding
// (sdp_solver.py:18-107) of every instance, one launch each, one workgroup per instance like the loop kernel (kernels_batch.h).
//
// The handle path factors with a Chebyshev-filtered subspace iteration of many launches and ~40 host synchronisations per call: built
// for K = 10 003, where a dense decomposition is out of reach.  A sweep instance has K = 75 ... 675 users, a flat spectrum (relative
// gap at the cut 1e-2 ... 7e-4) and keeps a sizeable share of it (rank 50 - 98, up to K - 1): a DENSE decomposition inside the
// instance's workgroup has no convergence question and no launch chain.
//
// k_batch_factor: Xbar = (sum of X) / nit scattered from the pattern into a dense K x K row-major work matrix, then a one-sided Jacobi
// (Hestenes) on its ROWS.  Xbar is symmetric, so once the rows g_j are mutually orthogonal they are lambda_j v_j^T: the row norms are
// |lambda_j| -- the singular values svds ranks by, negative eigenvalues included -- and the column of X_half = U sqrt(S) is
// g_j / sqrt(||g_j||).  No eigenvector matrix is accumulated.  Pairs are taken in a round-robin tournament order (K - 1 rounds of K / 2
// disjoint pairs, K odd: K rounds with a bye); the eight waves share the pairs of a round, each wave takes two pairs at a time (both
// pairs' rows are loaded into registers before either is reduced, to have two dependent chains in flight), the three dot products are
// per-lane sums in ascending column order followed by the fixed-order wave reduction, and one workgroup barrier ends a round.  A rotation
// is skipped when |<p,q>| <= 1e-15 ||p|| ||q||; a sweep without a rotation, or the sweep cap, ends the iteration.  Nothing waits across
// workgroups and there are no atomics: an instance's factor is bitwise independent of its batch neighbours.
//
// k_batch_round: sdp_solver.rounding for the resident factor.  Row norms and the visiting order once; per attempt the Philox normals
// randv[Z, rank] keyed by (seed, attempt), row-normalised (:48-49), inprod (:56), the preference order (:57, descending, ties to the
// lower slot) and the greedy pass (:70-101) with k_greedy_b's three checks and its accumulation order, one user per step on the first
// wave.  Attempts run one after another; with stop_at_first the workgroup ends after the first attempt that leaves nobody over (:23-24).
//
// Limits: K <= EPI_MAX_K (the row registers of a pair: 2 x 2 x K / 64 doubles per lane) and the batch's own D <= 512.
#pragma once
#include "../../include/mmw_hip.h"
#include "kernels_batch.h"
#include "kernels_batch_spectral.h"
#include "kernels_round_draw.h"

namespace mmw {

constexpr int EPI_MAX_K = MMW_BATCH_EPILOGUE_MAX_K;
constexpr int EPI_SWEEP_CAP = 30;  // the CPU restatement of the method needed <= 13 sweeps on sweep instances
constexpr double EPI_ROT_TOL = 1e-15;
constexpr int EPI_INFO = 5;  // {sweeps, largest |cos| of a row pair met in the last sweep, rank, sigma_rank, sigma_rank+1}
constexpr int EPI_INFO_STRIDE = 8;  // doubles between the records of a call's instances
static_assert(EPI_MAX_K % WAVE == 0 && EPI_MAX_K / WAVE <= 16, "the Jacobi keeps K / 64 <= 16 elements of a row per lane");

struct FactorDesc {
    int K, rank, nnzL, cap;
    double div;             // Xbar = values / div (the run's sum: nit; parity mode: 1)
    int src_work;           // the values lie in the work buffer (parity mode) instead of the arena
    int unit_rows;          // the rows are unit by construction (k_batch_factor_random): the rounding visits them in index order
    int64_t o_lrow, o_col;  // int32 arena
    int64_t o_src;          // [nnzL] values on the pattern
    int64_t o_A, o_fac, o_nrm, o_info;  // fp64 work: K x K, K x rank, K, EPI_INFO
    int64_t o_ord;                      // int32 work: rows by descending norm
    int kind;                           // 0: X_half of Xbar; 1: the spectral block of the state's Laplacian (kernels_batch_spectral.h)
    int64_t s_soptr, s_soidx, s_sodata;  // kind 1: the state's rounding lists (S_gain without its diagonal), int32 / fp64
    int64_t o_rown;                      // kind 1, fp64 work: K, the users' row norms of the block before the division
};

// All sweeps of the one-sided Jacobi on the rows of A (K x K, row-major), NE = elements of a row per lane.
template <int NE>
__device__ __forceinline__ void epi_jacobi(double* A, int K, int cap, int* s_rot, double* s_cos, int& sweeps_out, double& cos_out) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int n = K + (K & 1), m = n - 1, npairs = n >> 1;  // players (index K is the bye of an odd K), rounds, pairs per round
    int sweeps = 0;
    double lastcos = 0.0;
    for (int sw = 0; sw < cap; ++sw) {
        int rot = 0;
        double cmax = 0.0;
        for (int r = 0; r < m; ++r) {
            for (int pi = wv; pi < npairs; pi += 2 * BATCH_WAVES) {
                int pr[2], qr[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int pj = pi + u * BATCH_WAVES;
                    int a = -1, b = -1;
                    if (pj < npairs) {
                        if (pj == 0) { a = m; b = r; }
                        else { a = r + pj; a = a >= m ? a - m : a; b = r - pj; b = b < 0 ? b + m : b; }
                        if (a >= K || b >= K) a = b = -1;
                    }
                    pr[u] = a < b ? a : b;
                    qr[u] = a < b ? b : a;
                }
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
            __syncthreads();  // the rows of this round are final before the next round pairs them anew
        }
        if (lane == 0) { s_rot[wv] = rot; s_cos[wv] = cmax; }
        __syncthreads();
        int tot = 0;
        double cm = 0.0;
        for (int w = 0; w < BATCH_WAVES; ++w) { tot += s_rot[w]; cm = fmax(cm, s_cos[w]); }
        __syncthreads();
        ++sweeps;
        lastcos = cm;
        if (tot == 0) break;
    }
    sweeps_out = sweeps;
    cos_out = lastcos;
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_factor(const FactorDesc* __restrict__ descs, const int* __restrict__ ia,
                                                                const double* __restrict__ fa, double* ew, int* __restrict__ ei,
                                                                const int* __restrict__ si, const double* __restrict__ sf) {
    const FactorDesc d = descs[blockIdx.x];
    __shared__ int s_rot[BATCH_WAVES];
    __shared__ double s_cos[BATCH_WAVES];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, rank = d.rank;
    const int* __restrict__ lrow = ia + d.o_lrow;
    const int* __restrict__ col = ia + d.o_col;
    const double* src = (d.src_work ? ew : fa) + d.o_src;
    double* A = ew + d.o_A;
    double* fac = ew + d.o_fac;
    double* nrm = ew + d.o_nrm;
    int* ord = ei + d.o_ord;
    if (d.kind == 1) {  // (workgroup-uniform) the Laplacian of the state instead of Xbar
        spectral_head(K, si + d.s_soptr, si + d.s_soidx, sf + d.s_sodata, A);
    } else {
        // ---- Xbar, dense (mmw.py:201, 213)
        const size_t KK = (size_t)K * K;
        for (size_t i = tid; i < KK; i += NT) A[i] = 0.0;
        __syncthreads();
        for (int e = tid; e < d.nnzL; e += NT) A[(size_t)lrow[e] * K + col[e]] = src[e] / d.div;
        __syncthreads();
    }
    // ---- rows made orthogonal
    int sweeps = 0;
    double lastcos = 0.0;
    if (K <= 4 * WAVE) epi_jacobi<4>(A, K, d.cap, s_rot, s_cos, sweeps, lastcos);
    else if (K <= 8 * WAVE) epi_jacobi<8>(A, K, d.cap, s_rot, s_cos, sweeps, lastcos);
    else if (K <= 12 * WAVE) epi_jacobi<12>(A, K, d.cap, s_rot, s_cos, sweeps, lastcos);
    else epi_jacobi<16>(A, K, d.cap, s_rot, s_cos, sweeps, lastcos);
    // ---- singular values = row norms, ranked by counting: descending, ties to the lower index (k_rank_count's rule)
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
    // ---- X_half[K, rank] = U sqrt(S) (mmw.py:215-216), columns in ascending sigma as svds returns them; a row of norm 0 gives a zero column
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

// ---- the random embedding (rand_sdp_solver.run_with_state, sdp_solver.py:109-114): K x D row-normalised normals as the resident factor.
// The block is the batch's own sketch of (seed, iteration 0), bitwise (batch_sketch_rows, kernels_batch.h); its record says rank = D.
// Every row has norm 1, so the rounding's visiting order (descending norm, sdp_solver.py:51) is one tie over all users: the reference
// sorts the last-bit noise of its norms there, an arbitrary permutation of exchangeable rows.  The batch takes the tie rule literally
// instead, the lower index first (RoundDesc::index_order), so the result depends on no summation order.
struct FactorRandomDesc {
    int K, D;
    uint64_t seed;
    int64_t o_fac, o_info;  // fp64 work: K x D, EPI_INFO
};
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_factor_random(const FactorRandomDesc* __restrict__ descs, double* ew) {
    const FactorRandomDesc d = descs[blockIdx.x];
    batch_sketch_rows(d.K, d.D, d.seed, 0u, ew + d.o_fac, 0, d.D);
    if ((int)threadIdx.x < EPI_INFO) ew[d.o_info + threadIdx.x] = threadIdx.x == 2 ? (double)d.D : 0.0;
}

// ---- the rounding ------------------------------------------------------------------------------------------------------------------
struct RoundDesc {
    int K, Z, Dp, nattempt, stop_first;
    int index_order;                                     // unit rows (FactorDesc::unit_rows): all norms tie, visit by index
    uint64_t seed;
    int64_t o_fac;                                       // fp64 factor work: gX = X_half [K, Dp]
    int64_t s_soptr, s_soidx, s_qptr, s_qidx;            // int32 lists of the state: S_gain without its diagonal, Q_asso
    int64_t s_sodata, s_sohmax, s_hmax;                  // fp64 lists: the gains, h_max of the receiving user, h_max
    int64_t r_randv, r_inprod, r_gain, r_nrm;            // fp64 round work: Z x Dp, K x Z, K x Z, K
    int64_t r_order, r_pref, r_z, r_rem;                 // int32 round work: K, K x Z, nattempt x K, nattempt + 1 (the last: attempts run)
};

// randv of (seed, attempt): Philox normals, one wave per row after the other; the row itself is randv_row's (kernels_round_draw.h), the
// one statement of the draw, which the handle's k_round_randv calls too (sdp_solver.py:48-49)
__device__ __forceinline__ void epi_randv_rows(int Z, int Dp, uint64_t seed, uint32_t attempt, double* R) {
    const int lane = (int)threadIdx.x & 63, wib = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    for (int row = wib; row < Z; row += nw) randv_row(row, Dp, seed, attempt, lane, R + (size_t)row * Dp);
}
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_randv(int Z, int Dp, uint64_t seed, uint32_t attempt, double* __restrict__ R) {
    epi_randv_rows(Z, Dp, seed, attempt, R);
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_round(const RoundDesc* __restrict__ descs, const double* __restrict__ ew,
                                                               const int* __restrict__ si, const double* __restrict__ sf, double* rw,
                                                               int* ri) {
    const RoundDesc d = descs[blockIdx.x];
    __shared__ int slot_l[EPI_MAX_K];
    __shared__ int bad[BATCH_MAX_D];
    __shared__ int s_rem;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, Z = d.Z, Dp = d.Dp;
    const double* __restrict__ gX = ew + d.o_fac;
    const int* __restrict__ soptr = si + d.s_soptr;
    const int* __restrict__ soidx = si + d.s_soidx;
    const int* __restrict__ qptr = si + d.s_qptr;
    const int* __restrict__ qidx = si + d.s_qidx;
    const double* __restrict__ sodata = sf + d.s_sodata;
    const double* __restrict__ sohmax = sf + d.s_sohmax;
    const double* __restrict__ hmax = sf + d.s_hmax;
    double* R = rw + d.r_randv;
    double* ip = rw + d.r_inprod;
    double* gain = rw + d.r_gain;
    double* nrm = rw + d.r_nrm;
    int* order = ri + d.r_order;
    int* pref = ri + d.r_pref;
    int* zout = ri + d.r_z;
    int* rem = ri + d.r_rem;
    const size_t KZ = (size_t)K * Z;
    for (size_t i = tid; i < (size_t)d.nattempt * K; i += NT) zout[i] = -2;  // attempts not run
    for (int a = tid; a < d.nattempt; a += NT) rem[a] = -1;
    // ---- the visiting order, once: descending ||gX_k|| (sdp_solver.py:51), ties to the lower index
    if (d.index_order) {  // (workgroup-uniform) unit rows: one tie over all users
        for (int k = tid; k < K; k += NT) order[k] = k;
    } else {
        for (int row = wv; row < K; row += BATCH_WAVES) {
            double s = 0.0;
            for (int c = lane; c < Dp; c += WAVE) {
                const double x = gX[(size_t)row * Dp + c];
                s += x * x;
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
            order[r] = k;
        }
    }
    int used = 0;
    for (int a = 0; a < d.nattempt; ++a) {
        epi_randv_rows(Z, Dp, d.seed, (uint32_t)a, R);
        __syncthreads();  // (also: the order, and the last attempt's slots copied out)
        // ---- inprod = randv gX^T (:56), user-major; the sums start empty
        for (size_t idx = tid; idx < KZ; idx += NT) {
            const int k = (int)(idx / Z), z = (int)(idx % Z);
            const double* x = gX + (size_t)k * Dp;
            const double* r = R + (size_t)z * Dp;
            double s = 0.0;
            for (int c = 0; c < Dp; ++c) s += r[c] * x[c];
            ip[idx] = s;
            gain[idx] = 0.0;
        }
        for (int k = tid; k < K; k += NT) slot_l[k] = -1;
        __syncthreads();
        // ---- preference order per user (:57): descending inprod, ties to the lower slot
        for (size_t idx = tid; idx < KZ; idx += NT) {
            const int k = (int)(idx / Z), z = (int)(idx % Z);
            const double* row = ip + (size_t)k * Z;
            const double mine = row[z];
            int r = 0;
            for (int j = 0; j < Z; ++j) r += (row[j] > mine) || (row[j] == mine && j < z);
            pref[(size_t)k * Z + r] = z;
        }
        __syncthreads();
        // ---- the greedy pass (:70-101), one user per step on the first wave: (a) the interference accumulated at k stays within
        // h_max[k], (b) k's emission keeps every member of the slot that k reaches within its h_max, (c) no member shares an access
        // point with k; the sums take one add per address and user, in assignment order (:94)
        if (wv == 0) {
            int un = 0;
            for (int kk = 0; kk < K; ++kk) {
                const int k = order[kk];
                const int sb = soptr[k], deg = soptr[k + 1] - sb, qb = qptr[k], qdeg = qptr[k + 1] - qb;
                const double hk = hmax[k];
                for (int z = lane; z < Z; z += WAVE) bad[z] = gain[(size_t)k * Z + z] > hk ? 1 : 0;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int e = lane; e < deg; e += WAVE) {
                    const int nb = soidx[sb + e];
                    const int zn = slot_l[nb];
                    if (zn >= 0 && gain[(size_t)nb * Z + zn] + sodata[sb + e] > sohmax[sb + e]) bad[zn] = 1;
                }
                for (int e = lane; e < qdeg; e += WAVE) {
                    const int zn = slot_l[qidx[qb + e]];
                    if (zn >= 0) bad[zn] = 1;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                int z_take = -1;
                for (int z0 = 0; z0 < Z && z_take < 0; z0 += WAVE) {
                    const int zz = z0 + lane;
                    const int pz = zz < Z ? pref[(size_t)k * Z + zz] : 0;
                    const bool ok = zz < Z && !bad[pz];
                    const unsigned long long mk = __ballot(ok);
                    if (mk) z_take = __shfl(pz, (int)__builtin_ctzll(mk));
                }
                if (z_take >= 0) {
                    for (int e = lane; e < deg; e += WAVE) gain[(size_t)soidx[sb + e] * Z + z_take] += sodata[sb + e];
                    if (lane == 0) slot_l[k] = z_take;
                } else {
                    ++un;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the sums and the slot are written before the next user reads them
                __builtin_amdgcn_wave_barrier();
            }
            if (lane == 0) { s_rem = un; rem[a] = un; }
        }
        __syncthreads();
        for (int k = tid; k < K; k += NT) zout[(size_t)a * K + k] = slot_l[k];
        used = a + 1;
        if (d.stop_first && s_rem == 0) break;  // (workgroup-uniform: read from LDS after the barrier)
    }
    if (tid == 0) rem[d.nattempt] = used;
}

}  // namespace mmw
