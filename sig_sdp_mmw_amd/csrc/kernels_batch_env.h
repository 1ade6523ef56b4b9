// The problem generator and the scorer for MANY small instances, one workgroup per instance: what env_device.h does for one
// instance with a chain of launches and three host prefix sums, restated for the online sweeps of the reference
// (sim_script/journal_version/sim_mmw_online.py:34-78: 100 seeds x 3 variants x 11 time points at K = 300), where the stations move
// between the points and every point needs generate_S_Q_hmax (sim_src/env/env.py:136-196) of the moved positions for the rounding
// and evaluate_sinr / evaluate_bler (env.py:198-233) of the colouring it returns.
//
// k_batch_env_rx: receive powers, association, the members of every AP, the row lengths of S_gain / S_gain without its diagonal /
// Q_asso with their prefix sums, h_max, and the three totals the host needs to size the lists.  k_batch_env_fill: the lists, in
// the layout k_batch_round reads through RoundDesc::s_* (kernels_batch_epilogue.h) and the full CSR mmw_batch_env_state hands out.
// k_batch_env_evaluate: SINR, the one-survivor rule and the block error rate.  The arithmetic is env_device.h's, function for
// function (env_dist, env_loss, the power control, the first-maximum association, ordered compaction by ballot, interference
// summed member by member in ascending user order), so an instance's state is bitwise the one mmw_env_create builds.
//
// No atomics, nothing waits across workgroups, every reduction and every prefix sum runs in a fixed order inside the instance's
// workgroup: an instance's results are bitwise independent of its batch neighbours.  Work arrays live in global memory (one
// workgroup = one CU, so they stay in its caches); LDS holds only the evaluator's slot numbers (4 KiB, under k_batch_round's 6 KiB).
//
// Limits: K <= EPI_MAX_K (the evaluator's slot numbers in LDS, and what k_batch_round takes), A <= BENV_MAX_A.
#pragma once
#include "env_device.h"
#include "kernels_batch_epilogue.h"

namespace mmw {

constexpr int BENV_MAX_A = 1024;
constexpr int BENV_TOTALS = 4;  // ints per instance read back after the count pass: nnz(S), nnz(S without diagonal), nnz(Q), spare

struct BatchEnvDesc {
    int K, A;
    int64_t o_k;                                                          // users of the instances before this one (call buffers)
    int64_t f_sta, f_ap, f_rx, f_hmax, f_sinr0;                           // fp64 arena, fixed part: 2K, 2A, K x A, K, K
    int64_t i_asso, i_apcnt, i_apptr, i_apmem, i_sptr, i_soptr, i_qptr;   // int32 arena, fixed part: K, A, A+1, K, K+1, K+1, K+1
    int64_t i_sidx, i_soidx, i_qidx;                                      // int32 arena, the lists of the last move
    int64_t f_sval, f_soval, f_sohmax, f_qval;                            // fp64 arena, the lists of the last move
};

// exclusive prefix sums of v[0 .. n) in place and the total in v[n], by ONE wave: 64 entries per trip, carried in order
__device__ __forceinline__ void benv_scan(int* v, int n) {
    const int lane = (int)threadIdx.x & 63;
    int carry = 0;
    for (int b = 0; b < n; b += WAVE) {
        const int i = b + lane;
        const int x = i < n ? v[i] : 0;
        int s = x;
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(s, o);
            if (lane >= o) s += t;
        }
        if (i < n) v[i] = carry + s - x;
        carry += __shfl(s, WAVE - 1);
    }
    if (lane == 0) v[n] = carry;
}

// The count pass of a move.  One wave per user / per AP, eight waves per instance.
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_env_rx(const BatchEnvDesc* __restrict__ descs, EnvParams P, double min_sinr,
                                                                double* fa, int* ia, int* __restrict__ totals) {
    const BatchEnvDesc d = descs[blockIdx.x];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, A = d.A;
    const double* sta = fa + d.f_sta;
    const double* ap = fa + d.f_ap;
    double* rx = fa + d.f_rx;
    double* hmax = fa + d.f_hmax;
    int* asso = ia + d.i_asso;
    int* ap_cnt = ia + d.i_apcnt;
    int* ap_ptr = ia + d.i_apptr;
    int* ap_mem = ia + d.i_apmem;
    int* s_ptr = ia + d.i_sptr;
    int* so_ptr = ia + d.i_soptr;
    int* q_ptr = ia + d.i_qptr;
    // ---- rx[k][a] (unthresholded) and the association (k_env_rx, env.py:136-155, 177)
    for (int k = wv; k < K; k += BATCH_WAVES) {
        const double x = sta[2 * k], y = sta[2 * k + 1];
        double gmax = -1e300;
        for (int a = lane; a < A; a += WAVE) {
            const double g = -env_loss(P, env_dist(x, y, ap[2 * a], ap[2 * a + 1]));
            gmax = g > gmax ? g : gmax;
        }
        gmax = wave_max(gmax);
        const double t = __dsub_rn(P.min_sinr_db, __dsub_rn(gmax, P.noise_dbm));  // env.py:140
        const double txp = __dadd_rn(t, P.txp_off_db);                            // env.py:141
        double best = -1.0;
        int besta = 0x7fffffff;
        for (int a = lane; a < A; a += WAVE) {
            const double loss = env_loss(P, env_dist(x, y, ap[2 * a], ap[2 * a + 1]));
            const double db = __dsub_rn(__dsub_rn(txp, loss), P.noise_dbm);  // env.py:148
            const double v = pow(10.0, db / 10.0);
            rx[(size_t)k * A + a] = v;
            const double vt = v < P.thr ? 0.0 : v;
            if (vt > best) { best = vt; besta = a; }  // ascending a within a lane: keeps the first maximum
        }
        for (int o = 32; o >= 1; o >>= 1) {  // larger value wins, ties to the smaller AP index (np.argmax)
            const double ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(besta, o);
            if (ob > best || (ob == best && oa < besta)) { best = ob; besta = oa; }
        }
        if (lane == 0) asso[k] = besta;
    }
    __syncthreads();
    // ---- the users of every AP in ascending order (k_env_ap_members): count, prefix, ordered compaction
    for (int a = wv; a < A; a += BATCH_WAVES) {
        int n = 0;
        for (int k0 = 0; k0 < K; k0 += WAVE) {
            const int k = k0 + lane;
            n += __popcll(__ballot(k < K && asso[k] == a));
        }
        if (lane == 0) { ap_cnt[a] = n; ap_ptr[a] = n; }
    }
    __syncthreads();
    if (wv == 0) benv_scan(ap_ptr, A);
    __syncthreads();
    for (int a = wv; a < A; a += BATCH_WAVES) {
        int n = ap_ptr[a];
        for (int k0 = 0; k0 < K; k0 += WAVE) {
            const int k = k0 + lane;
            const bool hit = k < K && asso[k] == a;
            const unsigned long long m = __ballot(hit);
            if (hit) ap_mem[n + __popcll(m & ((1ull << lane) - 1ull))] = k;
            n += __popcll(m);
        }
    }
    // ---- row lengths (k_env_rowlen): S row k holds every user whose AP hears k above the threshold; h_max (env.py:194)
    for (int k = wv; k < K; k += BATCH_WAVES) {
        int n = 0;
        for (int a = lane; a < A; a += WAVE) {
            const double v = rx[(size_t)k * A + a];
            if ((v < P.thr ? 0.0 : v) != 0.0) n += ap_cnt[a];
        }
        n = wave_sum(n);
        if (lane == 0) {
            const int ak = asso[k];
            const double v = rx[(size_t)k * A + ak];
            const bool own = (v < P.thr ? 0.0 : v) != 0.0;  // the diagonal entry is stored
            s_ptr[k] = n;
            so_ptr[k] = n - (own ? 1 : 0);
            q_ptr[k] = ap_cnt[ak] - 1;
            hmax[k] = own ? __dsub_rn(v / min_sinr, 1.0) : -1.0;  // a user whose own link is below the threshold: 0 / min_sinr - 1
        }
    }
    __syncthreads();
    if (wv == 0) benv_scan(s_ptr, K);
    if (wv == 1) benv_scan(so_ptr, K);
    if (wv == 2) benv_scan(q_ptr, K);
    __syncthreads();
    if (tid == 0) {
        int* t = totals + (size_t)blockIdx.x * BENV_TOTALS;
        t[0] = s_ptr[K];
        t[1] = so_ptr[K];
        t[2] = q_ptr[K];
        t[3] = 0;
    }
}

// The fill pass (k_env_fill): CSR rows of S = rx[:, asso] without explicit zeros (env.py:190-192), the same rows without the diagonal
// with h_max of the receiving user beside every gain (what the greedy pass compares against), and Q (same AP, no diagonal, :181-189).
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_env_fill(const BatchEnvDesc* __restrict__ descs, double thr, double* fa, int* ia) {
    const BatchEnvDesc d = descs[blockIdx.x];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = d.K, A = d.A;
    const double* rx = fa + d.f_rx;
    const double* hmax = fa + d.f_hmax;
    const int* asso = ia + d.i_asso;
    const int* s_ptr = ia + d.i_sptr;
    const int* so_ptr = ia + d.i_soptr;
    const int* q_ptr = ia + d.i_qptr;
    int* s_idx = ia + d.i_sidx;
    int* so_idx = ia + d.i_soidx;
    int* q_idx = ia + d.i_qidx;
    double* s_val = fa + d.f_sval;
    double* so_val = fa + d.f_soval;
    double* so_hmax = fa + d.f_sohmax;
    double* q_val = fa + d.f_qval;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = wv; k < K; k += BATCH_WAVES) {
        int ns = s_ptr[k], no = so_ptr[k], nq = q_ptr[k];
        const int ak = asso[k];
        for (int j0 = 0; j0 < K; j0 += WAVE) {
            const int j = j0 + lane;
            double v = 0.0;
            int aj = -1;
            if (j < K) {
                aj = asso[j];
                v = rx[(size_t)k * A + aj];
                if (v < thr) v = 0.0;
            }
            const bool hs = v != 0.0, ho = hs && j != k, hq = j < K && aj == ak && j != k;
            const unsigned long long ms = __ballot(hs), mo = __ballot(ho), mq = __ballot(hq);
            if (hs) {
                const int o = ns + __popcll(ms & below);
                s_idx[o] = j;
                s_val[o] = v;
            }
            if (ho) {
                const int o = no + __popcll(mo & below);
                so_idx[o] = j;
                so_val[o] = v;
                so_hmax[o] = hmax[j];
            }
            if (hq) {
                const int o = nq + __popcll(mq & below);
                q_idx[o] = j;
                q_val[o] = 1.0;
            }
            ns += __popcll(ms);
            no += __popcll(mo);
            nq += __popcll(mq);
        }
    }
}

// evaluate_sinr / evaluate_bler (env.py:198-233) of one colouring per instance.  zin: the colourings of all instances one after
// another (Ktot doubles), then one slot count per instance (as doubles).  out: sinr[Ktot], then bler[Ktot] when want_bler.
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_env_evaluate(const BatchEnvDesc* __restrict__ descs, double* fa, const int* __restrict__ ia,
                                                                      const double* __restrict__ zin, int64_t Ktot, double Lbits, double Bw,
                                                                      double Tslot, int want_bler, double* __restrict__ out) {
    const BatchEnvDesc d = descs[blockIdx.x];
    __shared__ int s_z[EPI_MAX_K];  // the slot of every user, -1: outside [0, Z) (belongs to no slot, env.py:205)
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int K = d.K, A = d.A;
    const int Z = (int)zin[Ktot + blockIdx.x];
    const double* z = zin + d.o_k;
    const double* rx = fa + d.f_rx;
    double* sinr0 = fa + d.f_sinr0;
    const int* asso = ia + d.i_asso;
    const int* ap_ptr = ia + d.i_apptr;
    const int* ap_mem = ia + d.i_apmem;
    for (int k = tid; k < K; k += NT) {
        const double zi = z[k];
        const bool in = zi >= 0.0 && zi < (double)Z;
        const int s = in ? (int)zi : -1;
        s_z[k] = in && (double)s == zi ? s : -1;
    }
    __syncthreads();
    // SINR before the collision rule (k_env_sinr): the other members of the slot, one by one in ascending user order
    for (int i = tid; i < K; i += NT) {
        const int s = s_z[i];
        double v = 1e-3;
        if (s >= 0) {
            const int a = asso[i];
            double acc = 0.0;
            for (int j = 0; j < K; ++j)
                if (s_z[j] == s && j != i) acc = __dadd_rn(acc, rx[(size_t)j * A + a]);
            v = rx[(size_t)i * A + a] / __dadd_rn(acc, 1.0);
        }
        sinr0[i] = v;
    }
    __syncthreads();
    // users of one AP colliding in a slot: the strongest survives, first maximum (k_env_collide_bler, env.py:214-224); then the model
    for (int i = tid; i < K; i += NT) {
        double s = sinr0[i];
        const int zi = s_z[i];
        if (zi >= 0) {
            const int a = asso[i];
            bool lose = false;
            for (int m = ap_ptr[a]; m < ap_ptr[a + 1]; ++m) {
                const int j = ap_mem[m];
                if (j != i && s_z[j] == zi) {
                    const double sj = sinr0[j];
                    if (sj > s || (sj == s && j < i)) lose = true;
                }
            }
            if (lose) s = 1e-3;
        }
        out[d.o_k + i] = s;
        if (want_bler) out[Ktot + d.o_k + i] = env_bler(s, Lbits, Bw, Tslot);
    }
}

}  // namespace mmw
