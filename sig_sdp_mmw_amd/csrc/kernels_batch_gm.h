// The greedy baselines of the reference's sweeps inside the batch: MAX_GAIN.run / MAX_ASSO.run (sim_src/alg/gm.py:9-127) in the
// "stable" visiting order for MANY instances in one launch, one workgroup per taking instance (sim_script/journal_version/
// sim_all_bler.py:30-72 runs both on every (cell size, seed); ton_major_rv/sim_mmw_online_cmp_methods.py:79-88 runs MAX_GAIN once per
// drop).  The per-state path (kernels_gm.h, gm_handle.h) is one handle, one host-made key and one single-wave launch per instance:
// the greedy chain is one dependent sequence per instance, so the parallelism there is to have is across instances.
//
// k_batch_gm, per instance:
//   key    kind 0 (gm.py:11-18): the column sums of S with the diagonal zeroed, key[i] = sum_j S[j, i], accumulated in ASCENDING ROW j
//          -- the order scipy's CSC matvec gives S.transpose().sum(axis=1): the rows are walked in order, the lanes of the group add
//          one row's entries to distinct addresses (a canonical CSR row has no column twice), a barrier ends the row.
//          kind 1 (gm.py:81): the row sums of Q in stored order, one thread per row.
//          Both are bitwise the host's expressions (gm._gain_key / gm._asso_key).
//   order  argsort(-key, kind="stable"): rank by counting in LDS with the whole group, ties to the lower user index (mmw_gm_run's rule;
//          the asso key is almost all ties, so the rule is the contract).
//   slots  gm.py:24-58 / 85-115 exactly as k_gm_slots<*, true> with full = 1: the sums are zeroed once per slot and not per attempt,
//          attempt stamps, the first longest list wins, a slot that accepts nobody ends the loop with ZZ = Z, and so does the slot
//          after which everybody is assigned.  The decisions are a dependent chain: the FIRST WAVE decides (64 positions at a time,
//          the static data of the next 64 requested while the current ones are decided), the whole group forms the key and the
//          order, zeroes the sums and the owners of every slot and writes the winners' slot numbers.
// The slot's sums take one add per address and acceptance, in acceptance order: they are the handle's sums bit for bit.  No atomics,
// nothing waits across workgroups: an instance's result is bitwise independent of its batch neighbours.
//
// LDS (static, K = G = 1024): gsum 8 KiB, key 8 KiB, order 4 KiB, member stamps 4 KiB, group owners 4 KiB, slot 4 KiB, the two list
// buffers 8 KiB = 40 KiB, plus two words.
//
// Scope: Q a union of cliques with weights >= 1 (every state env.generate_S_Q_hmax makes, env.py:182-189) -- the owner path of
// k_gm_slots: one owner per group and slot, a user without a Q row has no group -- and K <= MMW_BATCH_EPILOGUE_MAX_K, at most that
// many groups.  Other states stay on a GreedyHandle.
#pragma once
#include "kernels_batch_epilogue.h"
#include "kernels_gm.h"

namespace mmw {

constexpr int BGM_MAX_G = 1024;  // group owners in LDS (a batch instance has at most K groups, an environment's at most BENV_MAX_A)

struct GmDesc {
    int K, G, kind, Zb, nattempt, pad0;       // Zb: the slot bound (K for not_Z_bound)
    int64_t s_soptr, s_soidx, s_qptr;         // int32 lists of the state: S_gain without its diagonal (rows), Q_asso's row pointers
    int64_t s_sodata, s_sohmax, s_hmax;       // fp64 lists: the gains, h_max of the receiving user, h_max
    int64_t g_grp, g_qdata;                   // int32 group id per user (-1: none); fp64 Q values in stored order
    int64_t o_z, o_key;                       // results: int32 view {slot[K], ZZ, remainder}; fp64 key[K]
};

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_gm(const GmDesc* __restrict__ descs, const int* __restrict__ si,
                                                            const double* __restrict__ sf, const int* __restrict__ gi,
                                                            const double* __restrict__ gf, double* out) {
    const GmDesc d = descs[blockIdx.x];
    __shared__ double gsum[EPI_MAX_K], key[EPI_MAX_K];
    __shared__ int order[EPI_MAX_K], mark[EPI_MAX_K], owner[BGM_MAX_G], slot[EPI_MAX_K], lists[2 * EPI_MAX_K];
    __shared__ int s_blen, s_buf;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, G = d.G;
    const int* __restrict__ soptr = si + d.s_soptr;
    const int* __restrict__ soidx = si + d.s_soidx;
    const int* __restrict__ qptr = si + d.s_qptr;
    const double* __restrict__ sodata = sf + d.s_sodata;
    const double* __restrict__ sohmax = sf + d.s_sohmax;
    const double* __restrict__ hmax = sf + d.s_hmax;
    const int* __restrict__ grp = gi + d.g_grp;
    const double* __restrict__ qdata = gf + d.g_qdata;
    int* zout = reinterpret_cast<int*>(out) + d.o_z;
    double* kout = out + d.o_key;
    for (int i = tid; i < K; i += NT) {
        key[i] = 0.0;
        mark[i] = 0;
        slot[i] = -1;
    }
    __syncthreads();
    // ---- the key
    if (d.kind == 0) {
        // row j's first entries are requested while row j - 1 is added
        int e = soptr[0] + tid;
        bool has = e < soptr[1];
        int idx = has ? soidx[e] : 0;
        double val = has ? sodata[e] : 0.0;
        for (int j = 0; j < K; ++j) {
            const int end = soptr[j + 1];
            int ne = end + tid;
            const bool nhas = j + 1 < K && ne < soptr[j + 2];
            const int nidx = nhas ? soidx[ne] : 0;
            const double nval = nhas ? sodata[ne] : 0.0;
            if (has) key[idx] += val;
            for (int e2 = e + NT; e2 < end; e2 += NT) key[soidx[e2]] += sodata[e2];
            __syncthreads();  // row j is added everywhere before row j + 1 adds to the same addresses
            e = ne; has = nhas; idx = nidx; val = nval;
        }
    } else {
        for (int k = tid; k < K; k += NT) {
            double s = 0.0;
            for (int q = qptr[k]; q < qptr[k + 1]; ++q) s += qdata[q];
            key[k] = s;
        }
        __syncthreads();
    }
    // ---- the visiting order: descending key, ties to the lower index
    for (int k = tid; k < K; k += NT) {
        const double mine = key[k];
        kout[k] = mine;
        int r = 0;
        for (int j = 0; j < K; ++j) {
            const double o = key[j];
            r += (o > mine) || (o == mine && j < k);
        }
        order[r] = k;
    }
    // ---- the slots
    int total = 0, entered = 0;
    bool all = false;
    for (int z = 0; z < d.Zb; ++z) {
        for (int i = tid; i < K; i += NT) gsum[i] = 0.0;
        for (int i = tid; i < G; i += NT) owner[i] = -1;
        __syncthreads();  // (also: the order, and the last slot's numbers)
        if (wv == 0) {
            int best = -1, blen = 0;
            for (int a = 0; a < d.nattempt; ++a) {
                const int stamp = z * d.nattempt + a + 1;
                const int cb = best == 0 ? 1 : 0;  // the buffer that does not hold the list kept so far
                int* cur = lists + cb * K;
                int len = 0;
                // static data of the 64 positions of the next chunk, requested while the current one is decided
                int nk = lane < K ? order[lane] : -1, ng = -1, nsb = 0, ndeg = 0;
                double nhk = 0.0;
                if (nk >= 0) { nhk = hmax[nk]; nsb = soptr[nk]; ndeg = soptr[nk + 1] - nsb; ng = grp[nk]; }
                for (int base = 0; base < K; base += WAVE) {
                    const int k = nk, g = ng, sb = nsb, deg = ndeg;
                    const double hk = nhk;
                    nk = base + WAVE + lane < K ? order[base + WAVE + lane] : -1;
                    ng = -1; nsb = 0; ndeg = 0; nhk = 0.0;
                    if (nk >= 0) { nhk = hmax[nk]; nsb = soptr[nk]; ndeg = soptr[nk + 1] - nsb; ng = grp[nk]; }
                    bool cand = k >= 0 && slot[k] < 0;
                    if (cand && g >= 0) {
                        const int o = owner[g];
                        cand = o < 0 || o == k;
                    }
                    unsigned long long m = __ballot(cand);
                    while (m) {
                        const int c = __builtin_ctzll(m);
                        m &= m - 1;
                        const int kc = __shfl(k, c), gc = __shfl(g, c), sbc = __shfl(sb, c), degc = __shfl(deg, c);
                        const double hkc = __shfl(hk, c);
                        bool bad = false;
                        if (gc >= 0) {
                            const int o = owner[gc];
                            bad = o >= 0 && o != kc;
                        }
                        bad = bad || gsum[kc] > hkc;  // gain_sum[k] + S[k,k] (zeroed) > h_max[k]
                        if (bad) continue;
                        // the first 64 entries of k's row stay in registers for the additions
                        bool v = false;
                        int j0 = -1;
                        double v0 = 0.0;
                        if (lane < degc) {
                            j0 = soidx[sbc + lane];
                            v0 = sodata[sbc + lane];
                            v = mark[j0] == stamp && gsum[j0] + v0 > sohmax[sbc + lane];
                        }
                        for (int e = lane + WAVE; e < degc; e += WAVE) {
                            const int j = soidx[sbc + e];
                            if (mark[j] == stamp && gsum[j] + sodata[sbc + e] > sohmax[sbc + e]) v = true;
                        }
                        if (__any(v)) continue;
                        if (j0 >= 0) gsum[j0] += v0;
                        for (int e = lane + WAVE; e < degc; e += WAVE) gsum[soidx[sbc + e]] += sodata[sbc + e];
                        if (lane == 0) {
                            mark[kc] = stamp;
                            cur[len] = kc;
                            if (gc >= 0) owner[gc] = kc;
                        }
                        ++len;
                        // the additions and the owner / stamp are seen by every lane before the next decision
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                if (len > blen) {
                    blen = len;
                    best = cb;
                }
            }
            if (lane == 0) {
                s_blen = blen;
                s_buf = best < 0 ? 0 : best;
            }
        }
        __syncthreads();
        const int blen = s_blen;
        const int* win = lists + s_buf * K;
        for (int i = tid; i < blen; i += NT) slot[win[i]] = z;
        ++entered;
        total += blen;
        __syncthreads();  // (also: s_blen is read by everybody before the next slot writes it)
        if (blen == 0) break;  // every later slot sees the same inputs and accepts nobody either
        if (total == K) { all = true; break; }
    }
    __syncthreads();
    for (int i = tid; i < K; i += NT) zout[i] = slot[i];
    if (tid == 0) {
        zout[K] = all ? entered : d.Zb;  // an empty slot: the reference enters every remaining one
        zout[K + 1] = K - total;
    }
}

// ---- the host side both handles share: one copy of the descriptors in, one launch, one copy of the results back
inline int batch_gm_args(const std::string& who, int kind, int32_t nattempt) {
    if (kind != 0 && kind != 1) return fail(MMW_ERR_ARG, who + ": kind must be 0 (MAX_GAIN) or 1 (MAX_ASSO), got " + std::to_string(kind));
    if (nattempt < 1) return fail(MMW_ERR_ARG, who + ": nattempt must be >= 1");
    if (nattempt > (1 << 20)) return fail(MMW_ERR_ARG, who + ": nattempt must be at most 2^20 (the attempt stamps are int32)");
    return MMW_OK;
}
struct GmWork {
    DevBuf<GmDesc> d_desc;
    DevBuf<double> out;
    // gd: one descriptor per taking instance tk[t] with its sizes and list offsets set; the result offsets are laid out here
    int run(hipStream_t st, int B, const std::vector<int>& tk, std::vector<GmDesc>& gd, const int* si, const double* sf, const int* gi,
            const double* gf, int32_t* z_out, int32_t* zz_out, int32_t* rem_out, double* key_out) {
        int64_t ni = 0, nk = 0;
        for (GmDesc& g : gd) { g.o_z = ni; ni += g.K + 2; }
        const int64_t nid = (ni + 1) / 2;  // the int32 results lie in front, the keys behind them
        for (GmDesc& g : gd) { g.o_key = nid + nk; nk += g.K; }
        MMW_TRY(out.alloc((size_t)(nid + nk)));
        MMW_TRY(d_desc.alloc(gd.size()));
        MMW_TRY(copy_h2d(d_desc.p, gd.data(), gd.size() * sizeof(GmDesc), st));
        hipLaunchKernelGGL(k_batch_gm, dim3((unsigned)gd.size()), dim3(BATCH_THREADS), 0, st, d_desc.p, si, sf, gi, gf, out.p);
        MMW_HIP(hipGetLastError());
        std::vector<double> host((size_t)(nid + (key_out ? nk : 0)));
        MMW_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(double), st));
        const int32_t* hi = reinterpret_cast<const int32_t*>(host.data());
        for (int b = 0; b < B; ++b) zz_out[b] = rem_out[b] = -1;
        int32_t* z = z_out;
        double* kq = key_out;
        for (size_t t = 0; t < tk.size(); ++t) {
            const GmDesc& g = gd[t];
            std::copy(hi + g.o_z, hi + g.o_z + g.K, z);
            z += g.K;
            zz_out[tk[t]] = hi[g.o_z + g.K];
            rem_out[tk[t]] = hi[g.o_z + g.K + 1];
            if (key_out) {
                std::copy(host.begin() + g.o_key, host.begin() + g.o_key + g.K, kq);
                kq += g.K;
            }
        }
        return MMW_OK;
    }
};

}  // namespace mmw
