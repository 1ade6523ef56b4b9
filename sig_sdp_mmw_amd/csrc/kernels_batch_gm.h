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
#include "kernels_gm_rand.h"

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

// ---- MAX_RAND.run (gm.py:131-200) with its draws on the device, for many instances in one launch (mmw_batch_gm_rand) -----------------
// One workgroup per taking instance; per attempt a: the users' order keys of (seed, a) into LDS and their ascending rank (ties to the
// lower user), the K x Z preference values into the work arena (kernels_gm_rand.h: the draw mmw_gm_rand makes, value by value), the
// preference rows by k_slot_pref's rule, then the rounding's greedy pass -- a COPY of k_batch_round's (kernels_batch_epilogue.h), which
// stays as it is: the first wave, one user per step, the same three checks (a) the sum accumulated at k within h_max[k], (b) k's row
// keeps every member of the slot that k reaches within its h_max, (c) no member of the slot in k's Q row, and one add per address and
// user in assignment order.  (c) reads the columns of Q themselves: nothing assumes that Q is a union of cliques, so mmw_batch_gm's
// clique condition does not apply here.  Limits: K <= MMW_BATCH_EPILOGUE_MAX_K, Z <= BGMR_MAX_Z (one flag per slot in LDS).
constexpr int BGMR_MAX_Z = EPI_MAX_K;

struct GmRandDesc {
    int K, Z, nattempt, stop_first;
    uint64_t seed;
    int64_t s_soptr, s_soidx, s_qptr, s_qidx;  // int32 lists of the state: S_gain without its diagonal, Q_asso
    int64_t s_sodata, s_sohmax, s_hmax;        // fp64 lists: the gains, h_max of the receiving user, h_max
    int64_t r_pval, r_gain;                    // fp64 work: K x Z each
    int64_t r_pref, r_z, r_rem;                // int32 work: K x Z; results: nattempt x K, nattempt + 1 (the last: attempts run)
};

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_gm_rand(const GmRandDesc* __restrict__ descs, const int* __restrict__ si,
                                                                 const double* __restrict__ sf, double* rw, int* ri) {
    const GmRandDesc d = descs[blockIdx.x];
    __shared__ double key[EPI_MAX_K];
    __shared__ int order[EPI_MAX_K], slot_l[EPI_MAX_K], bad[BGMR_MAX_Z];
    __shared__ int s_rem;
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int K = d.K, Z = d.Z, npair = (Z + 1) >> 1;
    const int* __restrict__ soptr = si + d.s_soptr;
    const int* __restrict__ soidx = si + d.s_soidx;
    const int* __restrict__ qptr = si + d.s_qptr;
    const int* __restrict__ qidx = si + d.s_qidx;
    const double* __restrict__ sodata = sf + d.s_sodata;
    const double* __restrict__ sohmax = sf + d.s_sohmax;
    const double* __restrict__ hmax = sf + d.s_hmax;
    double* pv = rw + d.r_pval;
    double* gain = rw + d.r_gain;
    int* pref = ri + d.r_pref;
    int* zout = ri + d.r_z;
    int* rem = ri + d.r_rem;
    const size_t KZ = (size_t)K * Z;
    for (size_t i = tid; i < (size_t)d.nattempt * K; i += NT) zout[i] = -2;  // attempts not run
    for (int a = tid; a < d.nattempt; a += NT) rem[a] = -1;
    int used = 0;
    for (int a = 0; a < d.nattempt; ++a) {
        // ---- the draw of (seed, a); the sums start empty
        for (int k = tid; k < K; k += NT) {
            key[k] = gmr_order_key(k, d.seed, (uint32_t)a);
            slot_l[k] = -1;
        }
        for (size_t i = tid; i < (size_t)K * npair; i += NT) {
            const int k = (int)(i / npair), p = (int)(i % npair);
            double v0, v1;
            gmr_pref_pair(k, p, d.seed, (uint32_t)a, v0, v1);
            pv[(size_t)k * Z + 2 * p] = v0;
            if (2 * p + 1 < Z) pv[(size_t)k * Z + 2 * p + 1] = v1;
        }
        for (size_t idx = tid; idx < KZ; idx += NT) gain[idx] = 0.0;
        __syncthreads();  // (also: the last attempt's slots are copied out)
        // ---- the visiting order: ascending order key (argsort(randn(K)), gm.py:150), ties to the lower user
        for (int k = tid; k < K; k += NT) {
            const double mine = key[k];
            int r = 0;
            for (int j = 0; j < K; ++j) {
                const double o = key[j];
                r += (o < mine) || (o == mine && j < k);
            }
            order[r] = k;
        }
        // ---- preference order per user (gm.py:149): descending value, ties to the lower slot
        for (size_t idx = tid; idx < KZ; idx += NT) {
            const int k = (int)(idx / Z), z = (int)(idx % Z);
            const double* row = pv + (size_t)k * Z;
            const double mine = row[z];
            int r = 0;
            for (int j = 0; j < Z; ++j) r += (row[j] > mine) || (row[j] == mine && j < z);
            pref[(size_t)k * Z + r] = z;
        }
        __syncthreads();
        // ---- the greedy pass (gm.py:158-193 = sdp_solver.py:70-101), as k_batch_round runs it
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
        const bool done = d.stop_first && s_rem == 0;  // (workgroup-uniform: read from LDS after the barrier)
        __syncthreads();                               // everybody has read s_rem and slot_l before the next attempt writes them
        if (done) break;
    }
    if (tid == 0) rem[d.nattempt] = used;
}

// ---- the host side both handles share, in mmw_batch_round's output shapes: z_out nattempt * K slots per taking instance, attempt-major
// (-1 left over, -2 attempt not run), rem_out[B * nattempt] (-1: not run), used_out[B]
inline int batch_gm_rand_args(const std::string& who, int32_t nattempt, const void* Z, const void* seeds, const void* z_out, const void* rem_out, const void* used_out) {
    if (!Z || !seeds || !z_out || !rem_out || !used_out) return fail(MMW_ERR_ARG, who + ": null pointer");
    if (nattempt < 1 || nattempt > 4096) return fail(MMW_ERR_ARG, who + ": nattempt = " + std::to_string(nattempt) + " must be in [1, 4096]");
    return MMW_OK;
}
// the instances of `tk` that run: Z[b] > 0 (Z[b] <= 0 leaves an instance out, as a zero in `take` does); K and Z are refused by name
inline int batch_gm_rand_takers(const std::string& who, const std::vector<int>& tk, const int* K, const int32_t* Z, std::vector<int>& run) {
    run.clear();
    for (int b : tk) {
        if (Z[b] <= 0) continue;
        const std::string inst = who + ": instance " + std::to_string(b);
        if (K[b] > EPI_MAX_K) return fail(MMW_ERR_ARG, inst + ": K = " + std::to_string(K[b]) + " exceeds the limit " + std::to_string(EPI_MAX_K) + " (it stays on a GreedyHandle)");
        if (Z[b] > BGMR_MAX_Z) return fail(MMW_ERR_ARG, inst + ": Z = " + std::to_string(Z[b]) + " exceeds the limit " + std::to_string(BGMR_MAX_Z) + " (it stays on a GreedyHandle)");
        run.push_back(b);
    }
    if (run.empty()) return fail(MMW_ERR_ARG, who + ": no instance takes part");
    return MMW_OK;
}
inline void batch_gm_rand_blank(int B, int32_t nattempt, int32_t* rem_out, int32_t* used_out) {
    for (int b = 0; b < B; ++b) {
        used_out[b] = 0;
        for (int a = 0; a < nattempt; ++a) rem_out[(size_t)b * nattempt + a] = -1;
    }
}
struct GmRandWork {
    DevBuf<GmRandDesc> d_desc;
    DevBuf<double> rw;
    DevBuf<int> ri;
    // gd: one descriptor per running instance run[t] with its sizes, seed and list offsets set; the work offsets are laid out here
    int run(hipStream_t st, int B, const std::vector<int>& run, std::vector<GmRandDesc>& gd, int32_t nattempt, const int* si, const double* sf,
            int32_t* z_out, int32_t* rem_out, int32_t* used_out) {
        int64_t of = 0, oz = 0;
        for (GmRandDesc& g : gd) { g.r_z = oz; oz += (int64_t)nattempt * g.K; g.r_rem = oz; oz += nattempt + 1; }  // what goes back, in front
        const int64_t nback = oz;
        int64_t oi = a32(oz);
        for (GmRandDesc& g : gd) {
            const int64_t KZ = (int64_t)g.K * g.Z;
            g.r_pval = of; of = a32(of + KZ);
            g.r_gain = of; of = a32(of + KZ);
            g.r_pref = oi; oi = a32(oi + KZ);
        }
        MMW_TRY(rw.alloc((size_t)of));
        MMW_TRY(ri.alloc((size_t)oi));
        MMW_TRY(d_desc.alloc(gd.size()));
        MMW_TRY(copy_h2d(d_desc.p, gd.data(), gd.size() * sizeof(GmRandDesc), st));
        hipLaunchKernelGGL(k_batch_gm_rand, dim3((unsigned)gd.size()), dim3(BATCH_THREADS), 0, st, d_desc.p, si, sf, rw.p, ri.p);
        MMW_HIP(hipGetLastError());
        std::vector<int> host((size_t)nback);
        MMW_TRY(copy_d2h(host.data(), ri.p, host.size() * sizeof(int), st));
        batch_gm_rand_blank(B, nattempt, rem_out, used_out);
        int32_t* z = z_out;
        for (size_t t = 0; t < run.size(); ++t) {
            const GmRandDesc& g = gd[t];
            const size_t nz = (size_t)nattempt * g.K;
            std::copy(host.begin() + g.r_z, host.begin() + g.r_z + nz, z);
            z += nz;
            std::copy(host.begin() + g.r_rem, host.begin() + g.r_rem + nattempt, rem_out + (size_t)run[t] * nattempt);
            used_out[run[t]] = host[g.r_rem + nattempt];
        }
        return MMW_OK;
    }
};
// the plain C++ form of one instance (a host-only batch): z[nattempt * K], rem[nattempt], returns the attempts run
inline int batch_gm_rand_host(const GmState& g, int32_t Z, int32_t nattempt, int stop_first, uint64_t seed, int32_t* z, int32_t* rem) {
    const int K = g.K;
    std::vector<double> pv((size_t)K * Z), key(K);
    std::vector<int32_t> order(K), prf((size_t)K * Z);
    std::fill(z, z + (size_t)nattempt * K, -2);
    int used = 0;
    for (int a = 0; a < nattempt; ++a) {
        gm_rand_draw_host(K, Z, seed, (uint32_t)a, pv.data(), key.data());
        gm_rand_order_host(K, Z, pv.data(), key.data(), order.data(), prf.data());
        g.assign_host(Z, order.data(), prf.data(), z + (size_t)a * K, rem + a);
        used = a + 1;
        if (stop_first && rem[a] == 0) break;
    }
    return used;
}

}  // namespace mmw
