// mmw_batch_create_from_env: the batch for the states a BatchEnv holds, built on the device (kernels_batch_pattern.h) -- the batched
// form of mmw_create_from_env (solver_create.h).  The count launch reads the environment's own descriptor table; ONE readback brings
// the sizes, l_indptr, S_sum, the squared row sums and h_max of all instances; the host lays out the arenas (BatchCore::offsets) and
// computes norm_H and cH (update_slots: they depend on Z, and computed there their bits are mmw_batch_create's); one upload carries
// the descriptors and those scalars; the fill launch writes both arenas and the batch's own copy of the state; one launch writes the
// initial point.  Nothing of the environment is referenced afterwards.
#pragma once
#include "batch_env_handle.h"
#include "batch_handle.h"

inline int batch_init_from_env(mmw_batch& bt, mmw_batch_env& e, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit) {
    const std::string name = "mmw_batch_create_from_env";
    BatchCore& c = bt.core;
    const int B = e.B;
    if (!e.moved) return fail(MMW_ERR_STATE, name + ": instance 0: the environment holds no positions yet (mmw_batch_env_move)");
    for (int b = 0; b < B; ++b) {
        const std::string who = name + ": instance " + std::to_string(b);
        if (nit[b] < 1) return fail(MMW_ERR_ARG, who + ": nit must be >= 1");
        if (e.K[b] < 2) return fail(MMW_ERR_ARG, who + ": K must be >= 2");
        if (Z[b] < 2) return fail(MMW_ERR_ARG, who + ": Z must be >= 2 (the constraints divide by Z-1)");
        HostPattern sizes;  // K and D alone decide the first two limits
        sizes.K = e.K[b];
        sizes.n_l = sizes.n_asso = 0;
        const std::string err = BatchCore::check_limits(sizes, Z[b] * rank_radio);
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_batch: instance " + std::to_string(b) + ": " + err + " (run it on a handle)");
    }
    c.device = e.device; c.host_only = false; c.B = B; c.rank_radio = rank_radio;
    c.eta.assign(B, eta); c.nit.assign(nit, nit + B); c.iter.assign(B, 0); c.active.assign(B, 1);
    c.H.assign(B, HostPattern{});
    bt.greedy.gmx.resize(B);
    MMW_HIP(hipSetDevice(c.device));
    MMW_HIP(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    // ---- count pass and the one readback
    const int64_t Ktot = e.Ktot;
    DevBuf<double> rb;
    DevBuf<int> wi;
    MMW_TRY(rb.alloc((size_t)bpat_rb_doubles(Ktot, B)));
    MMW_TRY(wi.alloc((size_t)bpat_wi_ints(Ktot, B)));
    hipLaunchKernelGGL(k_batch_pattern_count, dim3((unsigned)B), dim3(BATCH_THREADS), 0, c.st, e.d_desc.p, e.P.thr, (const double*)e.fa.p, (const int*)e.ia.p,
                       Ktot, rb.p, wi.p);
    MMW_HIP(hipGetLastError());
    std::vector<double> hrb(rb.n);
    MMW_TRY(copy_d2h(hrb.data(), rb.p, hrb.size() * sizeof(double), c.st));
    const int32_t* hint = reinterpret_cast<const int32_t*>(hrb.data() + 3 * Ktot);
    for (int b = 0; b < B; ++b) {
        HostPattern& P = c.H[b];
        const int K = e.K[b];
        const int64_t ok = e.desc[b].o_k;
        const int32_t* lp = hint + bpat_rb_int(ok, b);
        P.K = K;
        P.l_indptr.assign(lp, lp + K + 1);
        P.n_l = lp[K + 1]; P.n_st = lp[K + 2]; P.n_gain = lp[K + 3]; P.n_asso = lp[K + 4];
        P.S_sum.assign(hrb.begin() + ok, hrb.begin() + ok + K);
        P.sq_sum.assign(hrb.begin() + Ktot + ok, hrb.begin() + Ktot + ok + K);
        P.h_max.assign(hrb.begin() + 2 * Ktot + ok, hrb.begin() + 2 * Ktot + ok + K);
        P.norm_H.assign(K, 0.0);
        P.cH.assign(K, 0.0);
        const std::string who = name + ": instance " + std::to_string(b);
        if (P.n_l != (int64_t)lp[K] || 2 * P.n_asso != (int64_t)e.tot[(size_t)b * BENV_TOTALS + 2]) return fail(MMW_ERR_STATE, who + ": internal: the count pass disagrees with the environment");
        const std::string err = update_slots(P, Z[b]);
        if (!err.empty()) return fail(MMW_ERR_ARG, who + ": " + err);
    }
    // ---- the arenas, the state's copy, the one upload
    int64_t oi = 0, of = 0;
    MMW_TRY(c.offsets(c.desc, oi, of));
    c.sat.assign(B, BatchPatItem{});
    int64_t ci = 0, cf = 0, os = 0;
    for (int b = 0; b < B; ++b) {
        BatchPatItem& t = c.sat[b];
        const int64_t K = e.K[b], ns = e.tot[(size_t)b * BENV_TOTALS], no = e.tot[(size_t)b * BENV_TOTALS + 1], nq = e.tot[(size_t)b * BENV_TOTALS + 2];
        t.o_scal = os; os += K;
        t.c_sptr = ci; ci = a32(ci + K + 1);
        t.c_soptr = ci; ci = a32(ci + K + 1);
        t.c_qptr = ci; ci = a32(ci + K + 1);
        t.c_sidx = ci; ci = a32(ci + ns);
        t.c_soidx = ci; ci = a32(ci + no);
        t.c_qidx = ci; ci = a32(ci + nq);
        t.v_hmax = cf; cf = a32(cf + K);
        t.v_sval = cf; cf = a32(cf + ns);
        t.v_soval = cf; cf = a32(cf + no);
        t.v_sohmax = cf; cf = a32(cf + no);
        t.v_qval = cf; cf = a32(cf + nq);
    }
    constexpr size_t DW = sizeof(BatchDesc) / sizeof(double), IW = sizeof(BatchPatItem) / sizeof(double);
    static_assert(sizeof(BatchPatItem) % sizeof(double) == 0, "the staging buffer is one array of doubles");
    const size_t w_desc = 0, w_item = w_desc + DW * B, w_invn = w_item + IW * B, w_cH = w_invn + (size_t)os, w_y0 = w_cH + (size_t)os;
    std::vector<double> stage(w_y0 + (size_t)B);
    std::memcpy(stage.data() + w_desc, c.desc.data(), sizeof(BatchDesc) * B);
    std::memcpy(stage.data() + w_item, c.sat.data(), sizeof(BatchPatItem) * B);
    for (int b = 0; b < B; ++b) {
        const HostPattern& P = c.H[b];
        for (int k = 0; k < P.K; ++k) stage[w_invn + c.sat[b].o_scal + k] = 1.0 / P.norm_H[k];
        std::copy(P.cH.begin(), P.cH.end(), stage.begin() + w_cH + c.sat[b].o_scal);
        stage[w_y0 + b] = 1.0 / (double)c.desc[b].C;
    }
    MMW_TRY(c.ia.alloc((size_t)oi));
    MMW_TRY(c.fa.alloc((size_t)of));
    MMW_TRY(c.si.alloc((size_t)ci));
    MMW_TRY(c.sf.alloc((size_t)cf));
    MMW_TRY(c.d_desc.alloc((size_t)B));
    MMW_HIP(hipMemsetAsync(c.ia.p, 0, (size_t)oi * sizeof(int), c.st));  // the padding between the arrays, as the host layout leaves it
    MMW_HIP(hipMemsetAsync(c.fa.p, 0, (size_t)of * sizeof(double), c.st));  // the iterate's zeros too: the init launch only places X = I and Y
    MMW_TRY(c.rl.upload(stage, c.st));
    const BatchDesc* dd = (const BatchDesc*)(c.rl.p + w_desc);
    hipLaunchKernelGGL(k_batch_pattern_fill, dim3((unsigned)B), dim3(BATCH_THREADS), 0, c.st, e.d_desc.p, dd, (const BatchPatItem*)(c.rl.p + w_item), e.P.thr,
                       (const double*)e.fa.p, (const int*)e.ia.p, Ktot, (const double*)rb.p, (const int*)wi.p, (const double*)(c.rl.p + w_invn),
                       (const double*)(c.rl.p + w_cH), c.ia.p, c.fa.p, c.si.p, c.sf.p);
    MMW_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_batch_pattern_init, dim3((unsigned)B), dim3(BATCH_THREADS), 0, c.st, dd, (const double*)(c.rl.p + w_y0), (const int*)c.ia.p, c.fa.p, 0);
    MMW_HIP(hipGetLastError());
    MMW_HIP(hipStreamSynchronize(c.st));  // the work buffers go out of scope, and the environment is free to move
    c.on_device = true;
    c.lazy.assign(B, 1);
    return MMW_OK;
}
