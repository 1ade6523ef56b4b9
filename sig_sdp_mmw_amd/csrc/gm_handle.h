#pragma once
#include "kernels_gm.h"
#include "kernels_gm_rand.h"
#include "kernels_round_draw.h"
#include "pattern_device.h"
#include "runtime.h"

using namespace mmw;

// ---- the greedy baselines of sim_src/alg/gm.py (csrc/kernels_gm.h) -----------------------------------------------------------------
// A light handle: the out-lists of S without diagonal, the Q rows, h_max and the clique structure of Q; none of the MMW pattern.
struct mmw_gm {
    GmState S;
    int device = -1;  // -1: host C++ only
    hipStream_t st = nullptr;
    DevBuf<int> so_indptr, so_indices, q_indptr, q_indices, grp, ord, slot, lists, info, rank_part;
    DevBuf<double> so_data, so_hmax, q_data, h_max, key, gsum, asum;
    DevBuf<int> mark, owner;
    // MAX_RAND (the rounding's scheduled greedy, kernels_round.h)
    DevBuf<int> pref, gsched, gnsteps;
    // MAX_RAND with its draws on the device (kernels_gm_rand.h): pref_val, {order_key, -order_key}, every attempt's slots and counts,
    // the winner's slots, {pick, rem[pick]}
    DevBuf<double> rpval, rkey;
    DevBuf<int> rslot, rrem, rwin, rpick;
    DevBuf<unsigned> gmask;
    DevBuf<GreedyHdr> ghdr, ghdr_s;
    DevBuf<double> ggain;
    // host side of the device path
    std::vector<int> h_info;
    // host path work
    std::vector<double> w_gs, w_as;
    std::vector<int> w_mark, w_owner;
    int w_stamp = 0;
    ~mmw_gm() {
        if (st) (void)hipStreamDestroy(st);
    }
    bool lds_fits() const {
        const size_t b = (size_t)S.K * (S.clique ? 12 : 20) + (S.clique ? (size_t)S.G * 4 : 0);
        return b <= GM_LDS_MAX;
    }
    int init(int dev) {
        device = dev;
        if (device < 0) {
            w_gs.assign(S.K, 0.0); w_as.assign(S.K, 0.0); w_mark.assign(S.K, 0); w_owner.assign(std::max(S.G, 1), -1);
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        MMW_TRY(so_indptr.upload(S.so_indptr, st)); MMW_TRY(so_indices.upload(S.so_indices, st));
        MMW_TRY(so_data.upload(S.so_data, st)); MMW_TRY(so_hmax.upload(S.so_hmax, st));
        MMW_TRY(q_indptr.upload(S.q_indptr, st)); MMW_TRY(q_indices.upload(S.q_indices, st)); MMW_TRY(q_data.upload(S.q_data, st));
        MMW_TRY(h_max.upload(S.h_max, st)); MMW_TRY(grp.upload(S.grp, st));
        const size_t K = (size_t)S.K;
        MMW_TRY(ord.alloc(K)); MMW_TRY(slot.alloc(K)); MMW_TRY(lists.alloc(2 * K)); MMW_TRY(info.alloc(GM_INFO_N));
        if (!lds_fits()) {
            MMW_TRY(gsum.alloc(K)); MMW_TRY(mark.alloc(K));
            if (S.clique) MMW_TRY(owner.alloc(std::max(S.G, 1))); else MMW_TRY(asum.alloc(K));
        }
        h_info.assign(GM_INFO_N, 0);
        return MMW_OK;
    }
    // mmw_gm_create_from_env: the handle for the state a generator holds now, its lists built on the device (pattern_device.h: RoundListSet)
    // and its groups taken from the association (k_gm_groups_from_asso).  S keeps K, the clique flag and the group count only: the host
    // vectors stay empty, the sizes are counted here.  A snapshot: nothing of the generator is referenced afterwards.
    int64_t n_so = -1, n_q = -1;  // >= 0: a handle built from an environment
    int64_t nnz_so() const { return n_so >= 0 ? n_so : (int64_t)S.so_indices.size(); }
    int64_t nnz_q() const { return n_q >= 0 ? n_q : (int64_t)S.q_indices.size(); }
    int init_from_env(const EnvListSource& E) {
        device = E.device;
        S.K = E.K;
        S.clique = true;  // the generator's Q is a union of AP cliques with weight 1 (env.py:182-189)
        MMW_HIP(hipSetDevice(device));
        MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        RoundListSet L;
        MMW_TRY(L.build(st, E));
        so_indptr.swap(L.so_indptr); so_indices.swap(L.so_indices); so_data.swap(L.so_data); so_hmax.swap(L.so_hmax);
        q_indptr.swap(L.q_indptr); q_indices.swap(L.q_indices); h_max.swap(L.h_max);
        n_so = L.nso; n_q = E.nnzQ;
        const size_t K = (size_t)S.K;
        MMW_TRY(q_data.alloc((size_t)E.nnzQ)); MMW_TRY(grp.alloc(K)); MMW_TRY(info.alloc(GM_INFO_N));
        if (E.nnzQ) MMW_HIP(hipMemcpyAsync(q_data.p, E.q_val, (size_t)E.nnzQ * sizeof(double), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_gm_groups_from_asso, dim3(grid_elems(K)), dim3(BLOCK), 0, st, S.K, E.A, E.asso, E.ap_ptr, E.ap_mem, grp.p, info.p);
        MMW_HIP(hipGetLastError());
        int G = 0;
        MMW_TRY(copy_d2h(&G, info.p, sizeof(int), st));
        S.G = G;
        MMW_TRY(ord.alloc(K)); MMW_TRY(slot.alloc(K)); MMW_TRY(lists.alloc(2 * K));
        if (!lds_fits()) {
            MMW_TRY(gsum.alloc(K)); MMW_TRY(mark.alloc(K)); MMW_TRY(owner.alloc(std::max(S.G, 1)));
        }
        h_info.assign(GM_INFO_N, 0);
        return MMW_OK;
    }
    // mmw_gm_key: kind 0, MAX_GAIN's key (gm.py:11-18); kind 1, MAX_ASSO's (:81).  A handle made from host arrays forms them there
    // (GmState::key_host); a handle built from an environment has no host lists and forms both on the device from its own, once.
    DevBuf<double> keys;  // [2][K]
    bool keys_ready = false;
    int get_key(int kind, double* out) {
        if (kind != 0 && kind != 1) return fail(MMW_ERR_ARG, "mmw_gm_key: kind must be 0 (MAX_GAIN) or 1 (MAX_ASSO)");
        if (n_so < 0) {
            std::vector<double> k;
            S.key_host(kind, k);
            std::copy(k.begin(), k.end(), out);
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        const size_t K = (size_t)S.K;
        if (!keys_ready) {
            MMW_TRY(keys.alloc(2 * K));
            hipLaunchKernelGGL(k_gm_keys, dim3(1), dim3(BLOCK), 0, st, S.K, (const int*)so_indptr.p, (const int*)so_indices.p, (const double*)so_data.p,
                               (const int*)q_indptr.p, (const double*)q_data.p, keys.p, keys.p + K);
            MMW_HIP(hipGetLastError());
            keys_ready = true;
        }
        return copy_d2h(out, keys.p + (size_t)kind * K, K * sizeof(double), st);
    }
    // one launch of k_gm_slots over ord (already on the device)
    int launch(int n, int z0, int nslot, int nattempt, int full) {
        const bool lds = lds_fits();
        const size_t sh = lds ? (size_t)S.K * (S.clique ? 12 : 20) + (S.clique ? (size_t)S.G * 4 : 0) : 0;
#define MMW_GM_LAUNCH(L, CQ)                                                                                                              \
    do {                                                                                                                                  \
        if (L) MMW_TRY(set_max_lds(reinterpret_cast<const void*>(&k_gm_slots<L, CQ>), (int)sh));                                       \
        hipLaunchKernelGGL((k_gm_slots<L, CQ>), dim3(1), dim3(WAVE), sh, st, S.K, n, (const int*)ord.p, z0, nslot, nattempt, full,       \
                           (const int*)grp.p, S.G, (const double*)h_max.p, (const int*)so_indptr.p, (const int*)so_indices.p,           \
                           (const double*)so_data.p, (const double*)so_hmax.p, (const int*)q_indptr.p, (const int*)q_indices.p,       \
                           (const double*)q_data.p, gsum.p, asum.p, mark.p, owner.p, slot.p, lists.p, info.p);                         \
    } while (0)
        if (lds && S.clique) MMW_GM_LAUNCH(true, true);
        else if (lds) MMW_GM_LAUNCH(true, false);
        else if (S.clique) MMW_GM_LAUNCH(false, true);
        else MMW_GM_LAUNCH(false, false);
#undef MMW_GM_LAUNCH
        MMW_HIP(hipGetLastError());
        MMW_TRY(copy_d2h(h_info.data(), info.p, GM_INFO_N * sizeof(int), st));
        return MMW_OK;
    }
    int check_order(const int32_t* order, int32_t n, bool perm) {
        if (n < 0 || n > S.K || (perm && n != S.K)) return fail(MMW_ERR_ARG, "gm: the visiting order has the wrong length");
        std::vector<char> seen(S.K, 0);
        for (int32_t i = 0; i < n; ++i) {
            if (order[i] < 0 || order[i] >= S.K) return fail(MMW_ERR_ARG, "gm: visiting order entry out of range");
            if (seen[order[i]]) return fail(MMW_ERR_ARG, "gm: a user appears twice in the visiting order");
            seen[order[i]] = 1;
        }
        return MMW_OK;
    }
    int pass(const int32_t* order, int32_t n, int32_t nattempt, int32_t* list_out, int32_t* nlist) {
        MMW_TRY(check_order(order, n, false));
        if (nattempt < 1) return fail(MMW_ERR_ARG, "gm: nattempt must be >= 1");
        if (device < 0) {
            std::vector<int32_t> best;
            S.pass_host(order, n, nattempt, w_gs, w_as, w_mark, w_owner, w_stamp, best);
            std::copy(best.begin(), best.end(), list_out);
            *nlist = (int32_t)best.size();
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        if (n == 0) { *nlist = 0; return MMW_OK; }
        MMW_TRY(copy_h2d(ord.p, order, (size_t)n * sizeof(int), st));
        MMW_TRY(launch(n, 0, 1, nattempt, 0));
        const int len = h_info[GM_INFO_LAST_LEN];
        if (len < 0 || len > n) return fail(MMW_ERR_STATE, "gm: the pass returned an impossible list length");
        MMW_TRY(copy_d2h(list_out, lists.p + (size_t)h_info[GM_INFO_LAST_BUF] * S.K, (size_t)len * sizeof(int), st));
        *nlist = len;
        return MMW_OK;
    }
    int run(const double* key_h, int32_t Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out, int32_t* rem_out) {
        if (Z < 0) return fail(MMW_ERR_ARG, "gm: Z must be >= 0");
        if (nattempt < 1) return fail(MMW_ERR_ARG, "gm: nattempt must be >= 1");
        const int K = S.K;
        int entered = 0, stop = GM_STOP_SLOTS, total = 0;
        if (device < 0) {
            S.run_host(key_h, Z, nattempt, z_out, entered, stop, total);
        } else {
            MMW_HIP(hipSetDevice(device));
            MMW_TRY(key.alloc(K)); MMW_TRY(rank_part.alloc((size_t)RANK_SPLIT * K));
            MMW_TRY(copy_h2d(key.p, key_h, (size_t)K * sizeof(double), st));
            // argsort(-key, kind="stable") on the device: rank by counting, ties by lower index (kernels_round.h)
            hipLaunchKernelGGL(k_rank_count, dim3((K + BLOCK - 1) / BLOCK, RANK_SPLIT), dim3(BLOCK), 0, st, K, (const double*)key.p, rank_part.p);
            hipLaunchKernelGGL(k_rank_scatter, dim3((K + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, K, (const int*)rank_part.p, ord.p);
            MMW_HIP(hipMemsetAsync(slot.p, 0xFF, (size_t)K * sizeof(int), st));
            if (Z > 0) {
                MMW_TRY(launch(K, 0, Z, nattempt, 1));
                entered = h_info[GM_INFO_ENTERED]; stop = h_info[GM_INFO_STOP]; total = h_info[GM_INFO_TOTAL];
            }
            MMW_TRY(copy_d2h(z_out, slot.p, (size_t)K * sizeof(int), st));
        }
        *zz_out = stop == GM_STOP_ALL_ASSIGNED ? entered : Z;  // an empty slot: the reference enters every remaining one (fact a)
        *rem_out = K - total;
        return MMW_OK;
    }
    // the launches of mmw_gm_assign from "ord[K] and pref[K][Z] are on the device" on: the rounding's scheduled greedy (solver_extras.h,
    // Extras::round_chain) with this order and preference, one workgroup; slots to slot_d[K] (-1 = left over), the count to rem_d[0]
    int greedy_buffers(int32_t Z) {
        const size_t K = (size_t)S.K;
        MMW_TRY(pref.alloc(K * Z)); MMW_TRY(ggain.alloc(K * Z)); MMW_TRY(ghdr.alloc(K));
        MMW_TRY(gmask.alloc(K)); MMW_TRY(gsched.alloc(K * GB_WAVES)); MMW_TRY(gnsteps.alloc(1)); MMW_TRY(ghdr_s.alloc(K * GB_WAVES));
        return MMW_OK;
    }
    int greedy_chain(int32_t Z, int* slot_d, int* rem_d) {
        const int K = S.K;
        const size_t baseb = (size_t)GB_WAVES * Z * 4;
        MMW_HIP(hipMemsetAsync(ggain.p, 0, (size_t)K * Z * sizeof(double), st));
        MMW_HIP(hipMemsetAsync(slot_d, 0xFF, (size_t)K * sizeof(int), st));
        MMW_HIP(hipMemsetAsync(gmask.p, 0, (size_t)K * sizeof(unsigned), st));
        hipLaunchKernelGGL(k_greedy_headers, dim3(grid_elems((size_t)K)), dim3(BLOCK), 0, st, K, (const int*)ord.p, (const int*)so_indptr.p,
                           (const int*)q_indptr.p, (const double*)h_max.p, ghdr.p);
        const size_t pairs = (size_t)K * GS_W;
        hipLaunchKernelGGL(k_greedy_cmask, dim3((unsigned)((pairs + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, K, (const GreedyHdr*)ghdr.p,
                           (const int*)so_indices.p, (const int*)q_indices.p, gmask.p);
        hipLaunchKernelGGL(k_greedy_schedule, dim3(1), dim3(WAVE), 0, st, K, (const unsigned*)gmask.p, gsched.p, gnsteps.p);
        hipLaunchKernelGGL(k_greedy_sched_headers, dim3(grid_elems((size_t)K * 2)), dim3(BLOCK), 0, st, K, (const int*)gnsteps.p,
                           (const int*)gsched.p, (const GreedyHdr*)ghdr.p, ghdr_s.p);
        const bool slot_lds = baseb + (size_t)K * 4 <= 150 * 1024;
        const size_t sh = baseb + (slot_lds ? (size_t)K * 4 : 0);
        if (slot_lds) {
            MMW_TRY(set_max_lds(reinterpret_cast<const void*>(&k_greedy_b<true, true>), (int)sh));
            hipLaunchKernelGGL((k_greedy_b<true, true>), dim3(1), dim3(GB_WAVES * 64), sh, st, K, Z, (const GreedyHdr*)ghdr_s.p, (const int*)nullptr,
                               (const int*)pref.p, (const int*)so_indices.p, (const double*)so_data.p, (const double*)so_hmax.p, (const int*)q_indices.p,
                               ggain.p, slot_d, rem_d, (const int*)gnsteps.p);
        } else {
            MMW_TRY(set_max_lds(reinterpret_cast<const void*>(&k_greedy_b<false, true>), (int)sh));
            hipLaunchKernelGGL((k_greedy_b<false, true>), dim3(1), dim3(GB_WAVES * 64), sh, st, K, Z, (const GreedyHdr*)ghdr_s.p, (const int*)nullptr,
                               (const int*)pref.p, (const int*)so_indices.p, (const double*)so_data.p, (const double*)so_hmax.p, (const int*)q_indices.p,
                               ggain.p, slot_d, rem_d, (const int*)gnsteps.p);
        }
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    int assign(int32_t Z, const int32_t* order, const int32_t* pref_h, int32_t* z_out, int32_t* rem_out) {
        const int K = S.K;
        if (Z < 1) return fail(MMW_ERR_ARG, "gm: Z must be >= 1");
        MMW_TRY(check_order(order, K, true));
        for (size_t i = 0; i < (size_t)K * Z; ++i)
            if (pref_h[i] < 0 || pref_h[i] >= Z) return fail(MMW_ERR_ARG, "gm: slot preference entry out of range");
        if (device < 0) {
            S.assign_host(Z, order, pref_h, z_out, rem_out);
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        if ((size_t)GB_WAVES * Z * 4 > 150 * 1024) return fail(MMW_ERR_ARG, "gm: 32 Z bytes exceed the greedy kernel's LDS");
        MMW_TRY(greedy_buffers(Z));
        MMW_TRY(copy_h2d(ord.p, order, (size_t)K * sizeof(int), st));
        MMW_TRY(copy_h2d(pref.p, pref_h, (size_t)K * Z * sizeof(int), st));
        MMW_TRY(greedy_chain(Z, slot.p, info.p));
        MMW_TRY(copy_d2h(z_out, slot.p, (size_t)K * sizeof(int), st));
        int rem = 0;
        MMW_TRY(copy_d2h(&rem, info.p, sizeof(int), st));
        *rem_out = rem;
        return MMW_OK;
    }
    // ---- mmw_gm_rand / mmw_gm_rand_draw: MAX_RAND with the draws of kernels_gm_rand.h made where the state lies.  Every attempt has its
    // own user order, hence its own schedule: the attempts run one after another on the stream, each as draw -> rank -> preference ->
    // mmw_gm_assign's chain, and k_round_pick chooses among their counts.  Nothing crosses to the device; K + nattempt + 1 integers cross back.
    static int rand_check(const std::string& who, int32_t Z, int32_t nattempt, int pick_rule, const void* z_out, const void* rem_out, const void* pick_out) {
        if (Z < 1) return fail(MMW_ERR_ARG, who + ": Z = " + std::to_string(Z) + " must be >= 1");
        if (nattempt < 1 || nattempt > ROUND_MAX_ATTEMPTS)
            return fail(MMW_ERR_ARG, who + ": nattempt = " + std::to_string(nattempt) + " must be in [1, " + std::to_string(ROUND_MAX_ATTEMPTS) + "]");
        if (pick_rule != 0 && pick_rule != 1)
            return fail(MMW_ERR_ARG, who + ": pick_rule = " + std::to_string(pick_rule) + " must be 0 (the first feasible attempt, else the last) or 1 (the fewest users left over)");
        if (!z_out || !rem_out || !pick_out) return fail(MMW_ERR_ARG, who + ": null pointer");
        if ((size_t)GB_WAVES * Z * 4 > 150 * 1024) return fail(MMW_ERR_ARG, who + ": Z = " + std::to_string(Z) + ": 32 Z bytes exceed the greedy kernel's LDS");
        return MMW_OK;
    }
    // attempt `a`'s draw, order and preference table on the device: rpval, rkey, ord and pref hold them afterwards
    int rand_tables(int32_t Z, uint64_t seed, uint32_t a) {
        const int K = S.K;
        hipLaunchKernelGGL(k_gm_rand_key, dim3(grid_elems((size_t)K)), dim3(BLOCK), 0, st, K, seed, a, rkey.p, rkey.p + K);
        hipLaunchKernelGGL(k_rank_count, dim3((K + BLOCK - 1) / BLOCK, RANK_SPLIT), dim3(BLOCK), 0, st, K, (const double*)(rkey.p + K), rank_part.p);
        hipLaunchKernelGGL(k_rank_scatter, dim3((K + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, K, (const int*)rank_part.p, ord.p);
        hipLaunchKernelGGL(k_gm_rand_pref, dim3(grid_elems((size_t)K * ((Z + 1) / 2))), dim3(BLOCK), 0, st, K, Z, seed, a, rpval.p);
        hipLaunchKernelGGL(k_slot_pref, dim3(K, 1), dim3(BLOCK), (size_t)Z * sizeof(double), st, K, Z, (const double*)rpval.p, pref.p);
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    int rand(int32_t Z, int32_t nattempt, uint64_t seed, int pick_rule, int32_t* z_out, int32_t* rem_out, int32_t* pick_out) {
        MMW_TRY(rand_check("mmw_gm_rand", Z, nattempt, pick_rule, z_out, rem_out, pick_out));
        const int K = S.K;
        if (K > ROUND_PICK_MAX_K) return fail(MMW_ERR_ARG, "mmw_gm_rand: K = " + std::to_string(K) + " exceeds the pick's limit " + std::to_string(ROUND_PICK_MAX_K));
        if (device < 0) {
            std::vector<double> pv((size_t)K * Z), key(K);
            std::vector<int32_t> order(K), prf((size_t)K * Z), slots((size_t)nattempt * K);
            for (int a = 0; a < nattempt; ++a) {
                gm_rand_draw_host(K, Z, seed, (uint32_t)a, pv.data(), key.data());
                gm_rand_order_host(K, Z, pv.data(), key.data(), order.data(), prf.data());
                S.assign_host(Z, order.data(), prf.data(), slots.data() + (size_t)a * K, rem_out + a);
            }
            const int pick = gm_rand_pick_host(rem_out, nattempt, pick_rule);
            std::copy(slots.begin() + (size_t)pick * K, slots.begin() + (size_t)(pick + 1) * K, z_out);
            *pick_out = pick;
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        MMW_TRY(greedy_buffers(Z));
        MMW_TRY(rpval.alloc((size_t)K * Z)); MMW_TRY(rkey.alloc((size_t)2 * K)); MMW_TRY(rank_part.alloc((size_t)RANK_SPLIT * K));
        MMW_TRY(rslot.alloc((size_t)nattempt * K)); MMW_TRY(rrem.alloc(nattempt)); MMW_TRY(rwin.alloc(K)); MMW_TRY(rpick.alloc(2));
        for (int a = 0; a < nattempt; ++a) {
            MMW_TRY(rand_tables(Z, seed, (uint32_t)a));
            MMW_TRY(greedy_chain(Z, rslot.p + (size_t)a * K, rrem.p + a));
        }
        hipLaunchKernelGGL(k_round_pick, dim3((unsigned)((K + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, K, nattempt, pick_rule, (const int*)rrem.p, (const int*)rslot.p,
                           rwin.p, rpick.p);
        MMW_HIP(hipGetLastError());
        std::vector<int32_t> back((size_t)K + nattempt + 1);
        MMW_HIP(hipMemcpyAsync(back.data(), rwin.p, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, st));
        MMW_HIP(hipMemcpyAsync(back.data() + K, rrem.p, (size_t)nattempt * sizeof(int), hipMemcpyDeviceToHost, st));
        MMW_HIP(hipMemcpyAsync(back.data() + K + nattempt, rpick.p, sizeof(int), hipMemcpyDeviceToHost, st));
        MMW_HIP(hipStreamSynchronize(st));
        std::copy(back.begin(), back.begin() + K, z_out);
        std::copy(back.begin() + K, back.begin() + K + nattempt, rem_out);
        *pick_out = back[(size_t)K + nattempt];
        return MMW_OK;
    }
    int rand_draw(int32_t Z, uint64_t seed, int32_t attempt, double* pref_val_out, double* order_key_out) {
        if (Z < 1) return fail(MMW_ERR_ARG, "mmw_gm_rand_draw: Z = " + std::to_string(Z) + " must be >= 1");
        if (attempt < 0) return fail(MMW_ERR_ARG, "mmw_gm_rand_draw: attempt = " + std::to_string(attempt) + " must be >= 0");
        if ((size_t)GB_WAVES * Z * 4 > 150 * 1024) return fail(MMW_ERR_ARG, "mmw_gm_rand_draw: Z = " + std::to_string(Z) + ": 32 Z bytes exceed the greedy kernel's LDS");
        const int K = S.K;
        if (device < 0) {
            gm_rand_draw_host(K, Z, seed, (uint32_t)attempt, pref_val_out, order_key_out);
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(device));
        if (order_key_out) {
            MMW_TRY(rkey.alloc((size_t)2 * K));
            hipLaunchKernelGGL(k_gm_rand_key, dim3(grid_elems((size_t)K)), dim3(BLOCK), 0, st, K, seed, (uint32_t)attempt, rkey.p, rkey.p + K);
            MMW_HIP(hipGetLastError());
            MMW_TRY(copy_d2h(order_key_out, rkey.p, (size_t)K * sizeof(double), st));
        }
        if (pref_val_out) {
            MMW_TRY(rpval.alloc((size_t)K * Z));
            hipLaunchKernelGGL(k_gm_rand_pref, dim3(grid_elems((size_t)K * ((Z + 1) / 2))), dim3(BLOCK), 0, st, K, Z, seed, (uint32_t)attempt, rpval.p);
            MMW_HIP(hipGetLastError());
            MMW_TRY(copy_d2h(pref_val_out, rpval.p, (size_t)K * Z * sizeof(double), st));
        }
        return MMW_OK;
    }
};
