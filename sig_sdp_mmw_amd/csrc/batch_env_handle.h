// Batched problem generator and scorer (mmw_batch_env_*): B small instances, one workgroup each (csrc/kernels_batch_env.h), beside the
// batched solver (batch_handle.h), whose resident factors mmw_batch_round_env rounds against the state this handle holds.
//
// One int32 and one fp64 arena.  The front of each is laid out at creation (positions, receive powers, association, AP members, row
// pointers, h_max: their sizes follow from K and A); the lists behind it change size with every move, so a move is a count pass, ONE
// readback of the B totals, the arena grown if the lists no longer fit (grow-only; the front is copied over device to device), then
// the fill pass.
#pragma once
#include "batch_handle.h"
#include "kernels_batch_env.h"

static_assert(BENV_MAX_A <= BGM_MAX_G, "the association is k_batch_gm's group id: one owner word per access point in LDS");

struct mmw_batch_env {
    int device = 0, B = 0;
    hipStream_t st = nullptr;
    EnvParams P{};
    double min_sinr = 1.0;
    int64_t Ktot = 0, f_front = 0, i_front = 0;
    bool moved = false;
    std::vector<int> K;
    std::vector<BatchEnvDesc> desc;
    std::vector<int> tot;  // [B][BENV_TOTALS] of the last move
    std::vector<RoundLists> rlists;
    DevBuf<BatchEnvDesc> d_desc;
    DevBuf<double> fa, zbuf, obuf;
    DevBuf<int> ia, d_tot;
    GmWork gmw;
    ~mmw_batch_env() {
        if (!st) return;
        (void)hipSetDevice(device);
        (void)hipStreamDestroy(st);
    }
    int init(int dev, int32_t B_, const int32_t* K_, const int32_t* A_, const double* const* ap_xy, double fre_Hz, double txp_offset,
             double min_s_n_ratio, double min_sinr_, double noise_dbm) {
        device = dev; B = B_; min_sinr = min_sinr_;
        P.L0 = 20.0 * std::log10(fre_Hz / 1e6) + 16 - 28;
        P.noise_dbm = noise_dbm;
        P.min_sinr_db = 10.0 * std::log10(min_sinr_);
        P.txp_off_db = 10.0 * std::log10(txp_offset);
        P.thr = min_s_n_ratio;
        K.assign(K_, K_ + B);
        desc.assign(B, BatchEnvDesc{});
        // every instance's positions first, side by side: a move uploads them in one copy
        int64_t of = 0, oi = 0;
        for (int b = 0; b < B; ++b) {
            desc[b].K = K_[b]; desc[b].A = A_[b];
            desc[b].o_k = Ktot;
            desc[b].f_sta = 2 * Ktot;
            Ktot += K_[b];
        }
        of = a32(2 * Ktot);
        for (int b = 0; b < B; ++b) {
            BatchEnvDesc& d = desc[b];
            const int64_t k = d.K, a = d.A;
            d.f_ap = of; of = a32(of + 2 * a);
            d.f_rx = of; of = a32(of + k * a);
            d.f_hmax = of; of = a32(of + k);
            d.f_sinr0 = of; of = a32(of + k);
            d.i_asso = oi; oi = a32(oi + k);
            d.i_apcnt = oi; oi = a32(oi + a);
            d.i_apptr = oi; oi = a32(oi + a + 1);
            d.i_apmem = oi; oi = a32(oi + k);
            d.i_sptr = oi; oi = a32(oi + k + 1);
            d.i_soptr = oi; oi = a32(oi + k + 1);
            d.i_qptr = oi; oi = a32(oi + k + 1);
        }
        f_front = of; i_front = oi;
        MMW_HIP(hipSetDevice(device));
        MMW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        MMW_TRY(fa.alloc((size_t)f_front));
        MMW_TRY(ia.alloc((size_t)i_front));
        for (int b = 0; b < B; ++b) MMW_TRY(copy_h2d(fa.p + desc[b].f_ap, ap_xy[b], (size_t)2 * desc[b].A * sizeof(double), st));
        MMW_TRY(d_desc.alloc((size_t)B));
        MMW_TRY(d_tot.alloc((size_t)B * BENV_TOTALS));
        MMW_TRY(zbuf.alloc((size_t)(Ktot + B)));
        MMW_TRY(obuf.alloc((size_t)(2 * Ktot)));
        tot.assign((size_t)B * BENV_TOTALS, 0);
        return MMW_OK;
    }
    // the arena with room for `need` elements, its first `front` elements kept
    template <typename T> int grow(DevBuf<T>& buf, int64_t front, int64_t need) {
        if ((size_t)need <= buf.cap) { buf.n = (size_t)need; return MMW_OK; }
        DevBuf<T> nb;
        MMW_TRY(nb.alloc((size_t)(need + need / 4)));  // headroom: the totals drift by a few per cent from move to move
        MMW_HIP(hipMemcpyAsync(nb.p, buf.p, (size_t)front * sizeof(T), hipMemcpyDeviceToDevice, st));
        MMW_HIP(hipStreamSynchronize(st));
        std::swap(buf.p, nb.p); std::swap(buf.n, nb.n); std::swap(buf.cap, nb.cap);
        buf.n = (size_t)need;
        return MMW_OK;
    }
    int move(const double* const* sta_xy) {
        MMW_HIP(hipSetDevice(device));
        moved = false;
        std::vector<double> hs((size_t)2 * Ktot);
        for (int b = 0; b < B; ++b) std::copy(sta_xy[b], sta_xy[b] + (size_t)2 * K[b], hs.begin() + desc[b].f_sta);
        MMW_TRY(copy_h2d(fa.p, hs.data(), hs.size() * sizeof(double), st));
        MMW_TRY(copy_h2d(d_desc.p, desc.data(), desc.size() * sizeof(BatchEnvDesc), st));
        hipLaunchKernelGGL(k_batch_env_rx, dim3((unsigned)B), dim3(BATCH_THREADS), 0, st, d_desc.p, P, min_sinr, fa.p, ia.p, d_tot.p);
        MMW_HIP(hipGetLastError());
        MMW_TRY(copy_d2h(tot.data(), d_tot.p, tot.size() * sizeof(int), st));
        int64_t of = f_front, oi = i_front;
        rlists.assign(B, RoundLists{});
        for (int b = 0; b < B; ++b) {
            BatchEnvDesc& d = desc[b];
            const int64_t ns = tot[(size_t)b * BENV_TOTALS], no = tot[(size_t)b * BENV_TOTALS + 1], nq = tot[(size_t)b * BENV_TOTALS + 2];
            d.i_sidx = oi; oi = a32(oi + ns);
            d.i_soidx = oi; oi = a32(oi + no);
            d.i_qidx = oi; oi = a32(oi + nq);
            d.f_sval = of; of = a32(of + ns);
            d.f_soval = of; of = a32(of + no);
            d.f_sohmax = of; of = a32(of + no);
            d.f_qval = of; of = a32(of + nq);
            rlists[b] = {d.i_soptr, d.i_soidx, d.i_qptr, d.i_qidx, d.f_soval, d.f_sohmax, d.f_hmax};
        }
        MMW_TRY(grow(fa, f_front, of));
        MMW_TRY(grow(ia, i_front, oi));
        MMW_TRY(copy_h2d(d_desc.p, desc.data(), desc.size() * sizeof(BatchEnvDesc), st));
        hipLaunchKernelGGL(k_batch_env_fill, dim3((unsigned)B), dim3(BATCH_THREADS), 0, st, d_desc.p, P.thr, fa.p, ia.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(st));
        moved = true;
        return MMW_OK;
    }
    int check_inst(const char* who, int b) const {
        if (b < 0 || b >= B) return fail(MMW_ERR_ARG, std::string(who) + ": instance index out of range");
        if (!moved) return fail(MMW_ERR_STATE, std::string(who) + ": no positions yet (mmw_batch_env_move)");
        return MMW_OK;
    }
    int sizes(int b, int64_t out[4]) const {
        MMW_TRY(check_inst("mmw_batch_env_sizes", b));
        out[0] = desc[b].K; out[1] = desc[b].A; out[2] = tot[(size_t)b * BENV_TOTALS]; out[3] = tot[(size_t)b * BENV_TOTALS + 2];
        return MMW_OK;
    }
    int state(int b, int32_t* Sp, int32_t* Si, double* Sx, int32_t* Qp, int32_t* Qi, double* Qx, double* h) {
        MMW_TRY(check_inst("mmw_batch_env_state", b));
        MMW_HIP(hipSetDevice(device));
        const BatchEnvDesc& d = desc[b];
        const size_t k = (size_t)d.K, ns = (size_t)tot[(size_t)b * BENV_TOTALS], nq = (size_t)tot[(size_t)b * BENV_TOTALS + 2];
        MMW_TRY(copy_d2h(Sp, ia.p + d.i_sptr, (k + 1) * sizeof(int), st));
        MMW_TRY(copy_d2h(Si, ia.p + d.i_sidx, ns * sizeof(int), st));
        MMW_TRY(copy_d2h(Sx, fa.p + d.f_sval, ns * sizeof(double), st));
        MMW_TRY(copy_d2h(Qp, ia.p + d.i_qptr, (k + 1) * sizeof(int), st));
        MMW_TRY(copy_d2h(Qi, ia.p + d.i_qidx, nq * sizeof(int), st));
        MMW_TRY(copy_d2h(Qx, fa.p + d.f_qval, nq * sizeof(double), st));
        return copy_d2h(h, fa.p + d.f_hmax, k * sizeof(double), st);
    }
    int evaluate(const double* const* z_vec, const int32_t* Z, double packet_bit, double bandwidth, double slot_time, double* const* sinr_out,
                 double* const* bler_out) {
        if (!moved) return fail(MMW_ERR_STATE, "mmw_batch_env_evaluate: no positions yet (mmw_batch_env_move)");
        for (int b = 0; b < B; ++b) {
            if (!z_vec[b] || !sinr_out[b] || (bler_out && !bler_out[b])) return fail(MMW_ERR_ARG, "mmw_batch_env_evaluate: instance " + std::to_string(b) + ": null pointer");
            if (Z[b] < 1) return fail(MMW_ERR_ARG, "mmw_batch_env_evaluate: instance " + std::to_string(b) + ": Z must be positive");
        }
        MMW_HIP(hipSetDevice(device));
        std::vector<double> hz((size_t)(Ktot + B));
        for (int b = 0; b < B; ++b) {
            std::copy(z_vec[b], z_vec[b] + K[b], hz.begin() + desc[b].o_k);
            hz[(size_t)Ktot + b] = (double)Z[b];
        }
        MMW_TRY(copy_h2d(zbuf.p, hz.data(), hz.size() * sizeof(double), st));
        hipLaunchKernelGGL(k_batch_env_evaluate, dim3((unsigned)B), dim3(BATCH_THREADS), 0, st, d_desc.p, fa.p, ia.p, zbuf.p, Ktot, packet_bit, bandwidth,
                           slot_time, bler_out ? 1 : 0, obuf.p);
        MMW_HIP(hipGetLastError());
        std::vector<double> ho((size_t)(bler_out ? 2 : 1) * Ktot);
        MMW_TRY(copy_d2h(ho.data(), obuf.p, ho.size() * sizeof(double), st));
        for (int b = 0; b < B; ++b) {
            std::copy(ho.begin() + desc[b].o_k, ho.begin() + desc[b].o_k + K[b], sinr_out[b]);
            if (bler_out) std::copy(ho.begin() + Ktot + desc[b].o_k, ho.begin() + Ktot + desc[b].o_k + K[b], bler_out[b]);
        }
        return MMW_OK;
    }
    // MAX_GAIN / MAX_ASSO (kernels_batch_gm.h) on the state of the last move: the association is the group id, Q's values are the
    // fill pass's ones
    int gm(int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out, int32_t* rem_out, double* key_out) {
        const std::string who = "mmw_batch_env_gm";
        if (!moved) return fail(MMW_ERR_STATE, who + ": no positions yet (mmw_batch_env_move)");
        MMW_TRY(batch_gm_args(who, kind, nattempt));
        std::vector<int> tk;
        MMW_TRY(batch_takers(who.c_str(), B, take, nullptr, tk));
        std::vector<GmDesc> gd;
        for (int b : tk) {
            const BatchEnvDesc& d = desc[b];
            GmDesc g{};
            g.K = d.K; g.G = d.A; g.kind = kind; g.Zb = Z[b] <= 0 ? d.K : Z[b]; g.nattempt = nattempt;
            set_lists(g, rlists[b]);
            g.g_grp = d.i_asso; g.g_qdata = d.f_qval;
            gd.push_back(g);
        }
        MMW_HIP(hipSetDevice(device));
        return gmw.run(st, B, tk, gd, ia.p, fa.p, ia.p, fa.p, z_out, zz_out, rem_out, key_out);
    }
    // MAX_RAND with its draws on the device (k_batch_gm_rand) on the state of the last move
    GmRandWork grw;
    int gm_rand(const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out, int32_t* rem_out,
                int32_t* used_out) {
        const std::string who = "mmw_batch_env_gm_rand";
        if (!moved) return fail(MMW_ERR_STATE, who + ": no positions yet (mmw_batch_env_move)");
        MMW_TRY(batch_gm_rand_args(who, nattempt, Z, seeds, z_out, rem_out, used_out));
        std::vector<int> tk, run;
        MMW_TRY(batch_takers(who.c_str(), B, take, nullptr, tk));
        MMW_TRY(batch_gm_rand_takers(who, tk, K.data(), Z, run));
        std::vector<GmRandDesc> gd;
        for (int b : run) {
            GmRandDesc g{};
            g.K = K[b]; g.Z = Z[b]; g.nattempt = nattempt; g.stop_first = stop_at_first != 0; g.seed = seeds[b];
            set_lists(g, rlists[b]);
            g.s_qidx = rlists[b].qidx;
            gd.push_back(g);
        }
        MMW_HIP(hipSetDevice(device));
        return grw.run(st, B, run, gd, nattempt, ia.p, fa.p, z_out, rem_out, used_out);
    }
};
// mmw_batch_round_env: mmw_batch_round of the batch's resident factors against the state the environment holds
inline int batch_round_env(mmw_batch* bt, mmw_batch_env* e, const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds,
                           int32_t* z_out, int32_t* rem_out, int32_t* used_out) {
    const char* who = "mmw_batch_round_env";
    if (bt->core.host_only) return BatchCore::host_only_batch();
    if (e->device != bt->core.device) return fail(MMW_ERR_ARG, std::string(who) + ": the environment lives on another device");
    if (e->B != bt->core.B) return fail(MMW_ERR_ARG, std::string(who) + ": the batch holds " + std::to_string(bt->core.B) + " instances, the environment " + std::to_string(e->B));
    if (!e->moved) return fail(MMW_ERR_STATE, std::string(who) + ": no positions yet (mmw_batch_env_move)");
    const BatchEpilogue::RoundSource src{who, e->ia.p, e->fa.p, e->rlists.data(), e->K.data()};
    return bt->round(take, nattempt, stop_at_first, seeds, z_out, rem_out, used_out, &src);
}
