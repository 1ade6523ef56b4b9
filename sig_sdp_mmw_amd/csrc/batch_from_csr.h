// mmw_batch_create_from_csr: the batch for B CSR states that lie on the device (mmw_csr, csr_device.h), built there
// (kernels_batch_csr_pattern.h) -- the batched form of mmw_create_from_csr (solver_create.h: init_csr), shaped like batch_from_env.h.  One
// upload carries the per-instance table of the seven pointers and sizes; the count launch validates every instance and leaves what ONE
// readback needs: the verdicts, the sizes, l_indptr, S_sum, the squared row sums and h_max of all instances; the host lays out the arenas
// (BatchCore::offsets) and computes norm_H and cH (update_slots: they depend on Z, and computed there their bits are mmw_batch_create's);
// one upload carries the descriptors and those scalars; the fill launch writes both arenas and the batch's own copy of the state; one
// launch writes the initial point.  No mmw_csr is referenced afterwards.  Host-only states (device -1) take mmw_batch_create's own path.
#pragma once
#include "batch_handle.h"
#include "kernels_batch_csr_pattern.h"

inline int batch_init_from_csr(mmw_batch& bt, int32_t B, mmw_csr* const* csr, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit) {
    const std::string name = "mmw_batch_create_from_csr";
    BatchCore& c = bt.core;
    // ---- what is refused before anything is allocated or launched
    for (int b = 0; b < B; ++b)
        if (!csr[b]) return fail(MMW_ERR_ARG, name + ": instance " + std::to_string(b) + ": null pointer");
    const CsrDevice& first = csr[0]->c;
    for (int b = 0; b < B; ++b) {
        const CsrDevice& s = csr[b]->c;
        const std::string who = name + ": instance " + std::to_string(b);
        if (s.host_only != first.host_only)
            return fail(MMW_ERR_ARG, who + ": host-only states (device -1) and states on a device cannot share a batch (instance 0 is of the other kind)");
        if (!s.host_only && s.device != first.device)
            return fail(MMW_ERR_ARG, who + ": the state lies on device " + std::to_string(s.device) + ", instance 0 on device " + std::to_string(first.device));
        if (nit[b] < 1) return fail(MMW_ERR_ARG, who + ": nit must be >= 1");
        if (s.V.K < 2) return fail(MMW_ERR_ARG, who + ": K must be >= 2");
        if (Z[b] < 2) return fail(MMW_ERR_ARG, who + ": Z must be >= 2 (the constraints divide by Z-1)");
        HostPattern sizes;  // K and D alone decide the first two limits
        sizes.K = s.V.K;
        sizes.n_l = sizes.n_asso = 0;
        const std::string err = BatchCore::check_limits(sizes, Z[b] * rank_radio);
        if (!err.empty()) return fail(MMW_ERR_ARG, "mmw_batch: instance " + std::to_string(b) + ": " + err + " (run it on a handle)");
    }
    if (first.host_only) {  // the shared per-row checks in a plain loop, then mmw_batch_create's own path on the host copies
        static const int32_t no_i = 0;
        static const double no_d = 0.0;
        std::vector<int32_t> K(B);
        std::vector<const int32_t*> sp(B), si(B), qp(B), qi(B);
        std::vector<const double*> sx(B), qx(B), hm(B);
        for (int b = 0; b < B; ++b) {
            const CsrView& V = csr[b]->c.V;
            unsigned long long err[CSR_PHASES];
            csr_check_host(V, err);
            for (int p = 0; p < CSR_PHASES; ++p)
                if (err[p] != CSR_OK) return fail(MMW_ERR_ARG, name + ": instance " + std::to_string(b) + ": " + csr_err_text(err[p]));
            K[b] = V.K;
            sp[b] = V.Sp; qp[b] = V.Qp; hm[b] = V.h;
            si[b] = V.Si ? V.Si : &no_i; sx[b] = V.Sx ? V.Sx : &no_d;  // (an empty list may be a null pointer here, never read)
            qi[b] = V.Qi ? V.Qi : &no_i; qx[b] = V.Qx ? V.Qx : &no_d;
        }
        return bt.init(-1, B, K.data(), Z, rank_radio, eta, nit, sp.data(), si.data(), sx.data(), qp.data(), qi.data(), qx.data(), hm.data());
    }
    c.device = first.device; c.host_only = false; c.B = B; c.rank_radio = rank_radio;
    c.eta.assign(B, eta); c.nit.assign(nit, nit + B); c.iter.assign(B, 0); c.active.assign(B, 1);
    c.H.assign(B, HostPattern{});
    bt.greedy.gmx.resize(B);
    MMW_HIP(hipSetDevice(c.device));
    MMW_HIP(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    // ---- the table, the count pass and the one readback
    std::vector<BcsrItem> items((size_t)B);
    int64_t Ktot = 0, nwi = 0, nwf = 0;
    for (int b = 0; b < B; ++b) {
        BcsrItem& t = items[b];
        t.V = csr[b]->c.V;
        t.o_k = Ktot; Ktot += t.V.K;
        t.o_wi = nwi; nwi += bcsr_wi_ints(t.V.K, t.V.nnzS);
        t.o_wf = nwf; nwf += bcsr_wf_doubles(t.V.nnzS);
    }
    constexpr size_t TW = sizeof(BcsrItem) / sizeof(double);
    std::vector<double> table(TW * B);
    std::memcpy(table.data(), items.data(), sizeof(BcsrItem) * B);
    DevBuf<double> d_items, rb, wf;
    DevBuf<int> wi;
    MMW_TRY(d_items.upload(table, c.st));
    MMW_TRY(rb.alloc((size_t)bcsr_rb_doubles(Ktot, B)));
    MMW_TRY(wi.alloc((size_t)std::max<int64_t>(nwi, 1)));
    MMW_TRY(wf.alloc((size_t)std::max<int64_t>(nwf, 1)));
    const BcsrItem* di = (const BcsrItem*)d_items.p;
    hipLaunchKernelGGL(k_batch_csr_count, dim3((unsigned)B), dim3(BATCH_THREADS), 0, c.st, di, Ktot, rb.p, wi.p, wf.p);
    MMW_HIP(hipGetLastError());
    std::vector<double> hrb(rb.n);
    MMW_TRY(copy_d2h(hrb.data(), rb.p, hrb.size() * sizeof(double), c.st));
    const unsigned long long* herr = reinterpret_cast<const unsigned long long*>(hrb.data());
    for (int b = 0; b < B; ++b)  // the lowest failing instance; an instance with a failed check has written nothing else
        for (int p = 0; p < CSR_PHASES; ++p)
            if (herr[(size_t)CSR_PHASES * b + p] != CSR_OK)
                return fail(MMW_ERR_ARG, name + ": instance " + std::to_string(b) + ": " + csr_err_text(herr[(size_t)CSR_PHASES * b + p]));
    const double* hvec = hrb.data() + bcsr_rb_vec(B);
    const int32_t* hint = reinterpret_cast<const int32_t*>(hrb.data() + bcsr_rb_int0(Ktot, B));
    std::vector<int64_t> n_so((size_t)B);
    for (int b = 0; b < B; ++b) {
        HostPattern& P = c.H[b];
        const CsrView& V = items[b].V;
        const int K = V.K;
        const int64_t ok = items[b].o_k;
        const int32_t* lp = hint + bcsr_rb_int(ok, b);
        P.K = K;
        P.l_indptr.assign(lp, lp + K + 1);
        P.n_l = lp[K + 1]; P.n_st = lp[K + 2]; P.n_gain = lp[K + 3]; P.n_asso = lp[K + 4];
        n_so[b] = lp[K + 5];
        P.S_sum.assign(hvec + ok, hvec + ok + K);
        P.sq_sum.assign(hvec + Ktot + ok, hvec + Ktot + ok + K);
        P.h_max.assign(hvec + 2 * Ktot + ok, hvec + 2 * Ktot + ok + K);
        P.norm_H.assign(K, 0.0);
        P.cH.assign(K, 0.0);
        const std::string who = name + ": instance " + std::to_string(b);
        if (P.n_l != (int64_t)lp[K] || 2 * P.n_asso != (int64_t)V.nnzQ || n_so[b] > (int64_t)V.nnzS || P.n_st > n_so[b])
            return fail(MMW_ERR_STATE, who + ": internal: the count pass disagrees with the state's sizes");
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
        const int64_t K = items[b].V.K, ns = items[b].V.nnzS, no = n_so[b], nq = items[b].V.nnzQ;
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
    hipLaunchKernelGGL(k_batch_csr_fill, dim3((unsigned)B), dim3(BATCH_THREADS), 0, c.st, di, dd, (const BatchPatItem*)(c.rl.p + w_item), Ktot, (const double*)rb.p,
                       wi.p, wf.p, (const double*)(c.rl.p + w_invn), (const double*)(c.rl.p + w_cH), c.ia.p, c.fa.p, c.si.p, c.sf.p);
    MMW_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_batch_pattern_init, dim3((unsigned)B), dim3(BATCH_THREADS), 0, c.st, dd, (const double*)(c.rl.p + w_y0), (const int*)c.ia.p, c.fa.p, 0);
    MMW_HIP(hipGetLastError());
    MMW_HIP(hipStreamSynchronize(c.st));  // the work buffers go out of scope, and every mmw_csr may be destroyed
    c.on_device = true;
    c.lazy.assign(B, 1);
    return MMW_OK;
}
