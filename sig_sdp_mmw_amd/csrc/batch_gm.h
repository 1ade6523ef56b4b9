// The sweeps' greedy baselines in the batched solver (mmw_batch_gm, kernels_batch_gm.h): what the pattern does not keep of Q -- its
// values, and the clique structure decided at creation (GmState::find_cliques) -- goes up once, beside the epilogue's rounding lists.
// A batch built on the device (batch_from_env.h) decides it for ALL its instances at the first baseline, from its own copy of Q.
#pragma once
#include "batch_epilogue.h"
#include "kernels_batch_gm.h"

struct BatchGm {
    struct GmExtra {
        std::vector<double> q_data;
        std::vector<int32_t> grp;  // clique id per user, -1: no Q row
        int G = 0;
        bool clique = false;
    };
    std::vector<GmExtra> gmx;
    std::vector<int64_t> gm_ogrp, gm_oq;
    DevBuf<int> gm_i;
    DevBuf<double> gm_f;
    GmWork gmw;
    bool decided = false;  // a batch built on the device: gmx holds every instance's decision
    void extra(int b, int32_t K, const int32_t* Qp, const int32_t* Qi, const double* Qx) {
        GmState g;
        g.K = K;
        g.q_indptr.assign(Qp, Qp + K + 1); g.q_indices.assign(Qi, Qi + Qp[K]);
        g.q_data.assign(Qx, Qx + Qp[K]);
        GmExtra& x = gmx[b];
        x.clique = g.find_cliques();
        x.G = g.G;
        x.grp = std::move(g.grp);
        x.q_data = std::move(g.q_data);
    }
    // Every instance at once, whichever take part in this call: lists() uploads the decisions of the whole batch one time, so none
    // may be missing then.  Only Q is fetched; the host patterns stay as they are.
    void decide_all(const BatchCore& c) {
        if (!c.on_device || decided) return;
        std::vector<int32_t> qp, qi;
        std::vector<double> qx;
        for (int b = 0; b < c.B; ++b) {
            c.fetch_q(b, qp, qi, qx);
            extra(b, c.pat(b).K, qp.data(), qi.data(), qx.data());
        }
        decided = true;
    }
    // the instance's state as the greedy procedures read it (host-only batch)
    GmState state(const BatchCore& c, int b) const {
        const HostPattern& P = c.full(b);
        GmState g;
        g.K = P.K; g.G = gmx[b].G; g.clique = gmx[b].clique;
        g.so_indptr = P.so_indptr; g.so_indices = P.so_indices; g.so_data = P.so_data;
        for (int32_t n : P.so_indices) g.so_hmax.push_back(P.h_max[n]);
        g.q_indptr = P.q_indptr; g.q_indices = P.q_indices; g.q_data = gmx[b].q_data;
        g.grp = gmx[b].grp; g.h_max = P.h_max;
        return g;
    }
    int lists(const BatchCore& c) {
        if (!gm_ogrp.empty()) return MMW_OK;
        std::vector<int> hi;
        std::vector<double> hf;
        std::vector<int64_t> og(c.B), oq(c.B);
        for (int b = 0; b < c.B; ++b) {
            og[b] = (int64_t)hi.size(); hi.insert(hi.end(), gmx[b].grp.begin(), gmx[b].grp.end());
            oq[b] = (int64_t)hf.size(); hf.insert(hf.end(), gmx[b].q_data.begin(), gmx[b].q_data.end());
        }
        MMW_TRY(gm_i.upload(hi, c.st));
        MMW_TRY(gm_f.upload(hf, c.st));
        gm_ogrp = std::move(og); gm_oq = std::move(oq);
        return MMW_OK;
    }
    int run(const BatchCore& c, BatchEpilogue& epi, int kind, const int32_t* take, const int32_t* Z, int32_t nattempt, int32_t* z_out, int32_t* zz_out,
            int32_t* rem_out, double* key_out) {
        const std::string who = "mmw_batch_gm";
        MMW_TRY(batch_gm_args(who, kind, nattempt));
        std::vector<int> tk;
        MMW_TRY(c.takers(who.c_str(), take, tk));
        decide_all(c);
        for (int b : tk) {
            const std::string inst = who + ": instance " + std::to_string(b);
            if (c.pat(b).K > EPI_MAX_K) return fail(MMW_ERR_ARG, inst + ": K = " + std::to_string(c.pat(b).K) + " exceeds the limit " + std::to_string(EPI_MAX_K) + " (it stays on a GreedyHandle)");
            if (!gmx[b].clique) return fail(MMW_ERR_ARG, inst + ": Q_asso is not a union of cliques with weights >= 1 (it stays on a GreedyHandle)");
        }
        if (c.host_only) {
            for (int b = 0; b < c.B; ++b) zz_out[b] = rem_out[b] = -1;
            std::vector<double> key;
            for (int b : tk) {
                const GmState g = state(c, b);
                const int K = g.K, Zb = Z[b] <= 0 ? K : Z[b];
                g.key_host(kind, key);
                int entered = 0, stop = GM_STOP_SLOTS, total = 0;
                g.run_host(key.data(), Zb, nattempt, z_out, entered, stop, total);
                zz_out[b] = stop == GM_STOP_ALL_ASSIGNED ? entered : Zb;
                rem_out[b] = K - total;
                z_out += K;
                if (key_out) { std::copy(key.begin(), key.end(), key_out); key_out += K; }
            }
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(epi.round_lists(c));
        MMW_TRY(lists(c));
        std::vector<GmDesc> gd;
        for (int b : tk) {
            GmDesc g{};
            g.K = c.pat(b).K; g.G = gmx[b].G; g.kind = kind; g.Zb = Z[b] <= 0 ? g.K : Z[b]; g.nattempt = nattempt;
            set_lists(g, epi.rlists[b]);
            g.g_grp = gm_ogrp[b]; g.g_qdata = gm_oq[b];
            gd.push_back(g);
        }
        return gmw.run(c.st, c.B, tk, gd, epi.lists_i(c), epi.lists_f(c), gm_i.p, gm_f.p, z_out, zz_out, rem_out, key_out);
    }
    // mmw_batch_gm_rand: MAX_RAND with its draws on the device (k_batch_gm_rand) on the state the batch was built from.  It reads the
    // rounding's lists and works in buffers of its own: the arenas, the resident fields and the factors are not touched.
    GmRandWork grw;
    int rand(const BatchCore& c, BatchEpilogue& epi, const int32_t* take, const int32_t* Z, int32_t nattempt, int stop_at_first, const uint64_t* seeds,
             int32_t* z_out, int32_t* rem_out, int32_t* used_out) {
        const std::string who = "mmw_batch_gm_rand";
        MMW_TRY(batch_gm_rand_args(who, nattempt, Z, seeds, z_out, rem_out, used_out));
        std::vector<int> tk, run, Ks(c.B);
        MMW_TRY(c.takers(who.c_str(), take, tk));
        for (int b = 0; b < c.B; ++b) Ks[b] = c.pat(b).K;
        MMW_TRY(batch_gm_rand_takers(who, tk, Ks.data(), Z, run));
        if (c.host_only) {
            batch_gm_rand_blank(c.B, nattempt, rem_out, used_out);
            for (int b : run) {
                const GmState g = state(c, b);
                std::vector<int32_t> rem(nattempt, -1);
                used_out[b] = batch_gm_rand_host(g, Z[b], nattempt, stop_at_first, seeds[b], z_out, rem.data());
                std::copy(rem.begin(), rem.end(), rem_out + (size_t)b * nattempt);
                z_out += (size_t)nattempt * g.K;
            }
            return MMW_OK;
        }
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(epi.round_lists(c));
        std::vector<GmRandDesc> gd;
        for (int b : run) {
            GmRandDesc g{};
            g.K = Ks[b]; g.Z = Z[b]; g.nattempt = nattempt; g.stop_first = stop_at_first != 0; g.seed = seeds[b];
            set_lists(g, epi.rlists[b]);
            g.s_qidx = epi.rlists[b].qidx;
            gd.push_back(g);
        }
        return grw.run(c.st, c.B, run, gd, nattempt, epi.lists_i(c), epi.lists_f(c), z_out, rem_out, used_out);
    }
};
