// The greedy baselines of sim_src/alg/gm.py: MAX_GAIN / MAX_ASSO (:9-127), slot-major, and MAX_RAND (:134-200), user-major.
//
// MAX_GAIN and MAX_ASSO fill slot z = 0, 1, ... one after another.  In a slot every still unassigned user is visited in a given
// order (descending key, :31-32 / :88-89); it joins the slot when
//   (1) the gain already accumulated at it stays within its h_max (its own row adds 0 there, the diagonal is zeroed, :15),
//   (2) adding its row keeps every member j of the slot within h_max[j] (:36-39),
//   (3) no member shares its access point (:42-45),
// and the slot's sums then grow by its rows in acceptance order (:49-50).  `nattempt` passes run per slot on sums that are set to
// zero once per slot, not per attempt (:26-27: each attempt starts from what the earlier ones left), and the first longest list wins
// (:53-54).  The dense K-vectors of the reference reduce to the nonzeros: a member j that k does not reach sees gain_sum[j] + 0, and
// gain_sum[j] <= h_max[j] holds for every member from the moment it was accepted (each later acceptance checked it), so only k's
// out-neighbours that are members can fail (2); the same holds for the association sums and k's Q row in (3).  Adding 0.0 changes
// no sum, so the sums formed on the nonzeros in acceptance order are the reference's bit for bit.
//
// (3) on a Q that is a union of cliques with weights >= 1 (env.generate_S_Q_hmax, env.py:182-189): asso_sum[k] >= 1 exactly when a
// user of k's group other than k was accepted in this slot (in any attempt), and a member of k's group makes (3) fail for k.  So one
// owner per group and slot decides it: k passes iff the owner is nobody or k itself (an attempt after the first may accept the same
// user again).  The handle checks the structure once at creation; otherwise the sums of Q rows are kept like the gains.
//
// One wavefront runs the whole sequence (the decisions are a dependent chain).  Positions are taken 64 at a time: every lane loads
// one user's static data and the checks that only become stricter as the slot fills (user already assigned, group owned by another
// user) drop most candidates in one step; the survivors are decided one after another by the whole wave, the out-list and the Q row
// 64 entries at a time.  The slot's sums, the member stamps and the group owners sit in LDS when they fit (K = 10 003: 123 KB).
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "kernels_round.h"
#include "runtime.h"

namespace mmw {

constexpr size_t GM_LDS_MAX = 150 * 1024;
enum { GM_INFO_ENTERED = 0, GM_INFO_STOP = 1, GM_INFO_LAST_LEN = 2, GM_INFO_LAST_BUF = 3, GM_INFO_TOTAL = 4, GM_INFO_N = 8 };
enum { GM_STOP_SLOTS = 0, GM_STOP_ALL_ASSIGNED = 1, GM_STOP_EMPTY = 2 };

// Slots z0 .. z0 + nslot - 1 over the visiting order ord[0..n).  full = 1: users with slot[k] >= 0 are skipped and the winner of each
// slot is written to slot[]; full = 0 (one pass for a host-given order of unassigned users): slot[] is neither read nor written.
// The winner of the last slot entered is lists[info[LAST_BUF] * K .. + info[LAST_LEN]).
template <bool LDS, bool CLIQUE>
__global__ __launch_bounds__(WAVE) void k_gm_slots(int K, int n, const int* __restrict__ ord, int z0, int nslot, int nattempt, int full,
                                                   const int* __restrict__ grp, int G, const double* __restrict__ h_max,
                                                   const int* __restrict__ so_indptr, const int* __restrict__ so_indices,
                                                   const double* __restrict__ so_data, const double* __restrict__ so_hmax,
                                                   const int* __restrict__ q_indptr, const int* __restrict__ q_indices,
                                                   const double* __restrict__ q_data, double* gsum_g, double* asum_g, int* mark_g, int* owner_g,
                                                   int* __restrict__ slot, int* lists /* [2][K] */, int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    // LDS layout: gsum[K] f64, asum[K] f64 (not CLIQUE), mark[K] int, owner[G] int (CLIQUE)
    char* sp = smem_raw;
    double* gsum = gsum_g;
    double* asum = asum_g;
    int* mark = mark_g;
    int* owner = owner_g;
    if (LDS) {
        gsum = reinterpret_cast<double*>(sp); sp += (size_t)K * 8;
        if (!CLIQUE) { asum = reinterpret_cast<double*>(sp); sp += (size_t)K * 8; }
        mark = reinterpret_cast<int*>(sp); sp += (size_t)K * 4;
        if (CLIQUE) owner = reinterpret_cast<int*>(sp);
    }
    const int lane = threadIdx.x;
    for (int i = lane; i < K; i += WAVE) mark[i] = 0;
    int stamp = 0, total = 0, entered = 0, stop = GM_STOP_SLOTS, last_len = 0, last_buf = 0;
    for (int zi = 0; zi < nslot; ++zi) {
        for (int i = lane; i < K; i += WAVE) {
            gsum[i] = 0.0;
            if (!CLIQUE) asum[i] = 0.0;
        }
        if (CLIQUE)
            for (int i = lane; i < G; i += WAVE) owner[i] = -1;
        __syncthreads();
        int best = -1, blen = 0;
        for (int a = 0; a < nattempt; ++a) {
            ++stamp;
            const int cb = best == 0 ? 1 : 0;  // the buffer that does not hold the list kept so far
            int* cur = lists + (size_t)cb * K;
            int len = 0;
            // static data of the 64 positions of the next chunk, requested while the current one is decided
            int nk = -1;
            if (lane < n) nk = ord[lane];
            for (int base = 0; base < n; base += WAVE) {
                const int k = nk;
                nk = base + WAVE + lane < n ? ord[base + WAVE + lane] : -1;
                bool cand = k >= 0;
                if (cand && full) cand = slot[k] < 0;
                int g = -1, sb = 0, deg = 0, qb = 0, qdeg = 0;
                double hk = 0.0;
                if (cand) {
                    hk = h_max[k];
                    sb = so_indptr[k];
                    deg = so_indptr[k + 1] - sb;
                    if (CLIQUE) {
                        g = grp[k];
                        if (g >= 0) {
                            const int o = owner[g];
                            cand = o < 0 || o == k;
                        }
                    } else {
                        qb = q_indptr[k];
                        qdeg = q_indptr[k + 1] - qb;
                    }
                }
                unsigned long long m = __ballot(cand);
                while (m) {
                    const int c = __builtin_ctzll(m);
                    m &= m - 1;
                    const int kc = __shfl(k, c), gc = __shfl(g, c), sbc = __shfl(sb, c), degc = __shfl(deg, c);
                    const int qbc = __shfl(qb, c), qdegc = __shfl(qdeg, c);
                    const double hkc = __shfl(hk, c);
                    bool bad;
                    if (CLIQUE) {
                        bad = false;
                        if (gc >= 0) {
                            const int o = owner[gc];
                            bad = o >= 0 && o != kc;
                        }
                    } else {
                        bad = asum[kc] >= 1.0;  // asso_sum[k] + Q[k,k] (= 0) >= 1
                    }
                    bad = bad || gsum[kc] > hkc;  // gain_sum[k] + S[k,k] (zeroed) > h_max[k]
                    if (!bad) {
                        bool v = false;
                        for (int e = lane; e < degc; e += WAVE) {
                            const int j = so_indices[sbc + e];
                            if (mark[j] == stamp && gsum[j] + so_data[sbc + e] > so_hmax[sbc + e]) v = true;
                        }
                        if (!CLIQUE)
                            for (int e = lane; e < qdegc; e += WAVE) {
                                const int j = q_indices[qbc + e];
                                if (mark[j] == stamp && asum[j] + q_data[qbc + e] >= 1.0) v = true;
                            }
                        bad = __any(v);
                    }
                    if (!bad) {
                        for (int e = lane; e < degc; e += WAVE) {
                            const int j = so_indices[sbc + e];
                            gsum[j] += so_data[sbc + e];
                        }
                        if (!CLIQUE)
                            for (int e = lane; e < qdegc; e += WAVE) {
                                const int j = q_indices[qbc + e];
                                asum[j] += q_data[qbc + e];
                            }
                        if (lane == 0) {
                            mark[kc] = stamp;
                            cur[len] = kc;
                            if (CLIQUE && gc >= 0) owner[gc] = kc;
                        }
                        ++len;
                        __syncthreads();  // the additions and the owner / stamp are seen by every lane before the next decision
                    }
                }
            }
            if (len > blen) {
                blen = len;
                best = cb;
            }
        }
        last_len = blen;
        last_buf = best < 0 ? 0 : best;
        ++entered;
        total += blen;
        if (full) {
            const int* win = lists + (size_t)last_buf * K;
            for (int i = lane; i < blen; i += WAVE) slot[win[i]] = z0 + zi;
        }
        __syncthreads();
        if (blen == 0) { stop = GM_STOP_EMPTY; break; }  // every later slot sees the same inputs and accepts nobody either
        if (full && total == n) { stop = GM_STOP_ALL_ASSIGNED; break; }
    }
    if (lane == 0) {
        info[GM_INFO_ENTERED] = entered;
        info[GM_INFO_STOP] = stop;
        info[GM_INFO_LAST_LEN] = last_len;
        info[GM_INFO_LAST_BUF] = last_buf;
        info[GM_INFO_TOTAL] = total;
    }
}

// The clique structure of Q for a state the generator holds (mmw_gm_create_from_env): its Q is the same-AP relation (env.py:181-189), so a
// user's group is its access point and nothing has to be searched.  Numbered as GmState::find_cliques numbers them on the host: access
// points with two users or more, in the order of their first (lowest) user; a user alone behind its access point has no Q row and no
// group.  One thread per user counts the access points whose first user comes earlier (A is a few hundred); thread 0 counts the groups.
__global__ __launch_bounds__(BLOCK) void k_gm_groups_from_asso(int K, int A, const int* __restrict__ asso, const int* __restrict__ ap_ptr,
                                                               const int* __restrict__ ap_mem, int* __restrict__ grp, int* __restrict__ G_out) {
    for (int k = blockIdx.x * BLOCK + threadIdx.x; k < K; k += gridDim.x * BLOCK) {
        const int a = asso[k];
        int g = -1;
        if (ap_ptr[a + 1] - ap_ptr[a] >= 2) {
            const int first = ap_mem[ap_ptr[a]];
            g = 0;
            for (int b = 0; b < A; ++b)
                if (ap_ptr[b + 1] - ap_ptr[b] >= 2 && ap_mem[ap_ptr[b]] < first) ++g;
        }
        grp[k] = g;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int n = 0;
        for (int b = 0; b < A; ++b) n += ap_ptr[b + 1] - ap_ptr[b] >= 2 ? 1 : 0;
        *G_out = n;
    }
}

// The keys of gm.py:11-18 / :81 from a handle's own device lists, in scipy's summation orders (GmState::key_host says which): the gain key
// is the column sum of S without its diagonal accumulated in ASCENDING ROW, so ONE workgroup walks the rows one after another and adds a
// row's entries side by side (a row's columns are distinct: one writer per address, the barrier orders the rows); the association key
// is a row's Q weights added in stored order, one thread per row.
__global__ __launch_bounds__(BLOCK) void k_gm_keys(int K, const int* __restrict__ so_indptr, const int* __restrict__ so_indices,
                                                   const double* __restrict__ so_data, const int* __restrict__ q_indptr,
                                                   const double* __restrict__ q_data, double* key_gain, double* __restrict__ key_asso) {
    for (int k = threadIdx.x; k < K; k += BLOCK) {
        key_gain[k] = 0.0;
        double s = 0.0;
        for (int e = q_indptr[k]; e < q_indptr[k + 1]; ++e) s += q_data[e];
        key_asso[k] = s;
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        const int b = so_indptr[j], n = so_indptr[j + 1];
        if (b == n) continue;  // (uniform over the workgroup: no barrier is skipped by some threads only)
        for (int e = b + threadIdx.x; e < n; e += BLOCK) key_gain[so_indices[e]] += so_data[e];
        __syncthreads();
    }
}

// ---- the state the greedy baselines read, built on the host once per handle ------------------------------------------------------
struct GmState {
    int K = 0, G = 0;
    bool clique = false;
    std::vector<int32_t> so_indptr, so_indices, q_indptr, q_indices, grp;
    std::vector<double> so_data, so_hmax, q_data, h_max;

    // "" on success.  S: canonical CSR (gm.py reads rows of S with the diagonal zeroed, :15); Q: canonical CSR without diagonal.
    std::string build(int32_t K_, const int32_t* Sp, const int32_t* Si, const double* Sx, const int32_t* Qp, const int32_t* Qi,
                      const double* Qx, const double* h) {
        if (K_ < 1) return "K must be >= 1";
        K = K_;
        if (Sp[0] != 0 || Qp[0] != 0) return "indptr[0] must be 0";
        for (int32_t k = 0; k < K; ++k) {
            if (Sp[k + 1] < Sp[k] || Qp[k + 1] < Qp[k]) return "indptr must be non-decreasing";
            for (int32_t i = Sp[k]; i < Sp[k + 1]; ++i) {
                if (Si[i] < 0 || Si[i] >= K) return "S_gain column index out of range";
                if (i > Sp[k] && Si[i] <= Si[i - 1]) return "S_gain must be canonical CSR (sorted, no duplicates)";
            }
            for (int32_t i = Qp[k]; i < Qp[k + 1]; ++i) {
                if (Qi[i] < 0 || Qi[i] >= K) return "Q_asso column index out of range";
                if (i > Qp[k] && Qi[i] <= Qi[i - 1]) return "Q_asso must be canonical CSR (sorted, no duplicates)";
                if (Qi[i] == k && Qx[i] != 0.0) return "Q_asso must have an empty diagonal";
            }
        }
        h_max.assign(h, h + K);
        so_indptr.assign(K + 1, 0);
        q_indptr.assign(K + 1, 0);
        for (int32_t k = 0; k < K; ++k) {
            for (int32_t i = Sp[k]; i < Sp[k + 1]; ++i) {
                if (Si[i] == k || Sx[i] == 0.0) continue;  // the zeroed diagonal and explicit zeros add nothing and fail nothing
                so_indices.push_back(Si[i]);
                so_data.push_back(Sx[i]);
                so_hmax.push_back(h[Si[i]]);
            }
            so_indptr[k + 1] = (int32_t)so_indices.size();
            for (int32_t i = Qp[k]; i < Qp[k + 1]; ++i) {
                if (Qi[i] == k || Qx[i] == 0.0) continue;
                q_indices.push_back(Qi[i]);
                q_data.push_back(Qx[i]);
            }
            q_indptr[k + 1] = (int32_t)q_indices.size();
        }
        clique = find_cliques();
        return "";
    }
    // Q = union of cliques with every weight >= 1: grp[k] = clique id (-1 for a user without Q row)
    bool find_cliques() {
        grp.assign(K, -1);
        G = 0;
        for (size_t e = 0; e < q_data.size(); ++e)
            if (!(q_data[e] >= 1.0) || !std::isfinite(q_data[e])) { grp.assign(K, -1); G = 0; return false; }
        std::vector<int32_t> mem;
        for (int32_t k = 0; k < K; ++k) {
            if (grp[k] >= 0 || q_indptr[k + 1] == q_indptr[k]) continue;
            mem.assign(q_indices.begin() + q_indptr[k], q_indices.begin() + q_indptr[k + 1]);
            mem.insert(std::lower_bound(mem.begin(), mem.end(), k), k);
            for (int32_t m : mem) {
                if (grp[m] >= 0) { grp.assign(K, -1); G = 0; return false; }
                // row m must be mem without m
                if (q_indptr[m + 1] - q_indptr[m] != (int32_t)mem.size() - 1) { grp.assign(K, -1); G = 0; return false; }
                int32_t p = q_indptr[m];
                for (int32_t x : mem) {
                    if (x == m) continue;
                    if (q_indices[p++] != x) { grp.assign(K, -1); G = 0; return false; }
                }
                grp[m] = G;
            }
            ++G;
        }
        return true;
    }

    // ---- the same procedures as plain host C++ (device = -1) -------------------------------------------------------------------
    // one slot, `nattempt` attempts over ord[0..n) (users not assigned yet); returns the winning list
    void pass_host(const int32_t* ord, int32_t n, int32_t nattempt, std::vector<double>& gs, std::vector<double>& as, std::vector<int>& mark,
                   std::vector<int>& owner, int& stamp, std::vector<int32_t>& best) const {
        std::fill(gs.begin(), gs.end(), 0.0);
        if (clique) std::fill(owner.begin(), owner.end(), -1);
        else std::fill(as.begin(), as.end(), 0.0);
        best.clear();
        std::vector<int32_t> cur;
        for (int a = 0; a < nattempt; ++a) {
            ++stamp;
            cur.clear();
            for (int32_t i = 0; i < n; ++i) {
                const int32_t k = ord[i];
                bool bad;
                if (clique) bad = grp[k] >= 0 && owner[grp[k]] >= 0 && owner[grp[k]] != k;
                else bad = as[k] >= 1.0;
                if (bad || gs[k] > h_max[k]) continue;
                for (int32_t e = so_indptr[k]; e < so_indptr[k + 1] && !bad; ++e) {
                    const int32_t j = so_indices[e];
                    bad = mark[j] == stamp && gs[j] + so_data[e] > so_hmax[e];
                }
                if (!clique)
                    for (int32_t e = q_indptr[k]; e < q_indptr[k + 1] && !bad; ++e) {
                        const int32_t j = q_indices[e];
                        bad = mark[j] == stamp && as[j] + q_data[e] >= 1.0;
                    }
                if (bad) continue;
                for (int32_t e = so_indptr[k]; e < so_indptr[k + 1]; ++e) gs[so_indices[e]] += so_data[e];
                if (!clique)
                    for (int32_t e = q_indptr[k]; e < q_indptr[k + 1]; ++e) as[q_indices[e]] += q_data[e];
                else if (grp[k] >= 0)
                    owner[grp[k]] = k;
                mark[k] = stamp;
                cur.push_back(k);
            }
            if (cur.size() > best.size()) best = cur;
        }
    }
    // The keys of gm.py:11-18 / :81 in scipy's summation orders: kind 0, the column sums of S without its diagonal, accumulated in
    // ascending row (the CSC matvec behind S.transpose().sum(axis=1)); kind 1, the row sums of Q in stored order.
    void key_host(int kind, std::vector<double>& key) const {
        key.assign(K, 0.0);
        if (kind == 0) {
            for (int32_t j = 0; j < K; ++j)
                for (int32_t e = so_indptr[j]; e < so_indptr[j + 1]; ++e) key[so_indices[e]] += so_data[e];
        } else {
            for (int32_t k = 0; k < K; ++k) {
                double s = 0.0;
                for (int32_t e = q_indptr[k]; e < q_indptr[k + 1]; ++e) s += q_data[e];
                key[k] = s;
            }
        }
    }
    // MAX_GAIN / MAX_ASSO in the stable order of -key: pass_host slot by slot; z_out[k] = slot or -1, returns {slots entered, stop, total}
    void run_host(const double* key, int32_t Z, int32_t nattempt, int32_t* z_out, int& entered, int& stop, int& total) const {
        std::vector<double> gs(K, 0.0), as(K, 0.0);
        std::vector<int> mark(K, 0), owner(std::max(G, 1), -1);
        int stamp = 0;
        std::vector<int32_t> order(K), cur(K), best;
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] > key[b]; });
        std::fill(z_out, z_out + K, -1);
        entered = 0; stop = GM_STOP_SLOTS; total = 0;
        for (int32_t z = 0; z < Z; ++z) {
            int32_t n = 0;
            for (int32_t k : order) if (z_out[k] < 0) cur[n++] = k;
            pass_host(cur.data(), n, nattempt, gs, as, mark, owner, stamp, best);
            ++entered;
            for (int32_t k : best) z_out[k] = z;
            total += (int)best.size();
            if (best.empty()) { stop = GM_STOP_EMPTY; break; }
            if (total == K) { stop = GM_STOP_ALL_ASSIGNED; break; }
        }
    }
    // MAX_RAND's user-major assignment: the rounding's greedy (sdp_solver.py:70-101 = gm.py:158-193) for a given user order and
    // per-user slot preference pref[k * Z + r]
    void assign_host(int32_t Z, const int32_t* order, const int32_t* pref, int32_t* z_out, int32_t* rem) const {
        std::vector<double> gs((size_t)K * Z, 0.0);
        std::vector<int32_t> slot(K, -1);
        int32_t un = 0;
        for (int32_t kk = 0; kk < K; ++kk) {
            const int32_t k = order[kk];
            for (int32_t r = 0; r < Z; ++r) {
                const int32_t z = pref[(size_t)k * Z + r];
                if (gs[(size_t)k * Z + z] > h_max[k]) continue;
                bool bad = false;
                for (int32_t e = so_indptr[k]; e < so_indptr[k + 1] && !bad; ++e) {
                    const int32_t j = so_indices[e];
                    bad = slot[j] == z && gs[(size_t)j * Z + z] + so_data[e] > so_hmax[e];
                }
                for (int32_t e = q_indptr[k]; e < q_indptr[k + 1] && !bad; ++e) bad = slot[q_indices[e]] == z;
                if (bad) continue;
                for (int32_t e = so_indptr[k]; e < so_indptr[k + 1]; ++e) gs[(size_t)so_indices[e] * Z + z] += so_data[e];
                slot[k] = z;
                break;
            }
            if (slot[k] < 0) ++un;
        }
        std::copy(slot.begin(), slot.end(), z_out);
        *rem = un;
    }
};

}  // namespace mmw
