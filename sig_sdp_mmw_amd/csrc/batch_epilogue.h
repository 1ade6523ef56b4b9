// The epilogue of the batched solver on the device (mmw_batch_factor / mmw_batch_round, kernels_batch_epilogue.h; the factor over several
// workgroups: mmw_batch_set_factor_split, kernels_batch_factor_split.h).  Buffers of its own, made on first use and sized for the taking
// instances of the call; the state's rounding lists go up once (they do not depend on the slot count).
#pragma once
#include <type_traits>

#include "batch_core.h"
#include "kernels_batch_epilogue.h"
#include "kernels_batch_factor_split.h"

// where a state's rounding lists (S_gain without its diagonal, Q_asso, h_max: csrc/pattern.h) lie in an int32 and an fp64 buffer
struct RoundLists { int64_t soptr, soidx, qptr, qidx, sodata, sohmax, hmax; };
template <typename Desc> void set_lists(Desc& d, const RoundLists& l) {
    d.s_soptr = l.soptr; d.s_soidx = l.soidx; d.s_qptr = l.qptr;
    d.s_sodata = l.sodata; d.s_sohmax = l.sohmax; d.s_hmax = l.hmax;
    if constexpr (std::is_same_v<Desc, RoundDesc>) d.s_qidx = l.qidx;  // the greedy baselines read no column of Q (GmDesc)
}

struct BatchEpilogue {
    std::vector<FactorDesc> fdesc;  // per instance: where its factor of the last mmw_batch_factor lies (rank 0: none)
    DevBuf<double> ew, rw, rs_f, rvbuf;
    DevBuf<int> ei, ri, rs_i;
    DevBuf<FactorDesc> d_fdesc;
    DevBuf<RoundDesc> d_rdesc;
    DevBuf<FactorRandomDesc> d_frdesc;
    // the factor's split: workgroups per instance and round (empty: one launch, k_batch_factor); the item table, the spans, the slab
    // and the sweep records are buffers of its own, rebuilt per call
    struct FactorSplit {
        std::vector<int> parts;
        DevBuf<FactorItem> d_items;
        DevBuf<FactorSpan> d_spans;
        DevBuf<double> slab, rec;
        double call[4] = {0.0, 0.0, 0.0, 0.0};  // MMW_F_FACTOR_CALL: the last mmw_batch_factor {path, launches, host sweeps, largest grid}
    } fs;
    std::vector<RoundLists> rlists;

    // where the rounding lists lie: the upload of round_lists, or the state's copy a batch built on the device keeps (batch_core.h)
    const int* lists_i(const BatchCore& c) const { return c.on_device ? c.si.p : rs_i.p; }
    const double* lists_f(const BatchCore& c) const { return c.on_device ? c.sf.p : rs_f.p; }
    void on_restart() { fdesc.clear(); }  // a new run, or buffers laid out anew: the factors held so far are gone
    bool has_factor(int b) const { return !fdesc.empty() && fdesc[b].rank != 0; }
    static int no_factor(const std::string& who, int b) { return fail(MMW_ERR_STATE, who + ": instance " + std::to_string(b) + " has no factor (mmw_batch_factor)"); }
    int set_split(const BatchCore& c, const int32_t* p) { return c.host_only ? BatchCore::host_only_batch() : check_parts("mmw_batch_set_factor_split", p, c.B, fs.parts); }
    int factor(const BatchCore& c, const int32_t* take, const int32_t* rank, const double* const* xavg) {
        if (c.host_only) return BatchCore::host_only_batch();
        std::vector<int> tk;
        MMW_TRY(c.takers("mmw_batch_factor", take, tk));
        std::vector<int> rk(c.B, 0);
        for (int b : tk) {
            const BatchDesc& d = c.desc[b];
            const std::string who = "mmw_batch_factor: instance " + std::to_string(b);
            if (d.K > EPI_MAX_K) return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(d.K) + " exceeds the epilogue limit " + std::to_string(EPI_MAX_K) + " (factor it on a handle: mmw_batch_export)");
            if (!(xavg && xavg[b]) && c.iter[b] < c.nit[b])
                return fail(MMW_ERR_STATE, who + " has run " + std::to_string(c.iter[b]) + " of its " + std::to_string(c.nit[b]) + " iterations");
            rk[b] = rank ? rank[b] : std::min(d.K - 1, (d.Z - 1) * c.rank_radio);
            if (rk[b] < 1 || rk[b] > d.K) return fail(MMW_ERR_ARG, who + ": rank must be in [1, K]");
        }
        std::vector<FactorDesc> fd(c.B, FactorDesc{});
        std::vector<FactorDesc> launch;
        int64_t of = a32((int64_t)tk.size() * EPI_INFO_STRIDE), oi = 0;  // the records first, side by side: one copy brings them back
        int64_t ninfo = 0;
        for (int b : tk) {
            const BatchDesc& d = c.desc[b];
            FactorDesc& f = fd[b];
            const int64_t K = d.K;
            f.o_info = EPI_INFO_STRIDE * ninfo++;
            f.K = d.K; f.rank = rk[b]; f.nnzL = d.nnzL; f.cap = EPI_SWEEP_CAP;
            f.o_lrow = d.o_lrow; f.o_col = d.o_col;
            const bool parity = xavg && xavg[b];
            f.src_work = parity ? 1 : 0;
            f.div = parity ? 1.0 : (double)c.nit[b];
            f.o_src = d.o_xavg;
            if (parity) { f.o_src = of; of = a32(of + d.nnzL); }
            f.o_A = of; of = a32(of + K * K);
            f.o_fac = of; of = a32(of + K * f.rank);
            f.o_nrm = of; of = a32(of + K);
            f.o_ord = oi; oi = a32(oi + K);
            launch.push_back(f);
        }
        return run_factor(c, tk, fd, launch, of, oi, xavg);
    }
    // The Jacobi of a call for the descriptors laid out by mmw_batch_factor or mmw_batch_factor_spectral: the work buffers, the single
    // launch or the split chain, the records and the stderr line at the sweep cap.
    int run_factor(const BatchCore& c, const std::vector<int>& tk, std::vector<FactorDesc>& fd, const std::vector<FactorDesc>& launch, int64_t of,
                   int64_t oi, const double* const* xavg) {
        on_restart();  // the buffers are laid out anew: earlier factors are gone whatever happens below
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(ew.alloc((size_t)of));
        MMW_TRY(ei.alloc((size_t)oi));
        for (int b : tk)
            if (xavg && fd[b].src_work) MMW_TRY(copy_h2d(ew.p + fd[b].o_src, xavg[b], (size_t)fd[b].nnzL * sizeof(double), c.st));
        MMW_TRY(d_fdesc.alloc(launch.size()));
        MMW_TRY(copy_h2d(d_fdesc.p, launch.data(), launch.size() * sizeof(FactorDesc), c.st));
        bool split = false;
        for (int b : tk) split = split || (!fs.parts.empty() && fs.parts[b] > 1);
        if (split) {
            MMW_TRY(factor_split(c, tk, launch));
        } else {
            hipLaunchKernelGGL(k_batch_factor, dim3((unsigned)launch.size()), dim3(BATCH_THREADS), 0, c.st, d_fdesc.p, c.ia.p, c.fa.p, ew.p, ei.p, lists_i(c), lists_f(c));
            fs.call[0] = 0.0; fs.call[1] = 1.0; fs.call[2] = 0.0; fs.call[3] = (double)launch.size();
        }
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(c.st));
        // A factor that used up its sweeps while rows still rotated is handed out (its rows are orthogonal to the |cos| it reports),
        // and said so: nothing above looks at the record on its own.
        std::vector<double> rec((size_t)tk.size() * EPI_INFO_STRIDE);
        MMW_TRY(copy_d2h(rec.data(), ew.p, rec.size() * sizeof(double), c.st));
        for (size_t t = 0; t < tk.size(); ++t) {
            const double* r = rec.data() + t * EPI_INFO_STRIDE;
            if (r[0] >= EPI_SWEEP_CAP && r[1] > EPI_ROT_TOL)
                fprintf(stderr, "mmw_batch_factor: instance %d (K = %d): still rotating after the cap of %d sweeps, largest |cos| of a row pair %.3g\n",
                        tk[t], c.desc[tk[t]].K, EPI_SWEEP_CAP, r[1]);
        }
        fdesc = std::move(fd);
        return MMW_OK;
    }
    // The factor as head / one launch per round / tail for all taking instances (kernels_batch_factor_split.h); `launch` is on the
    // device already (d_fdesc).  One synchronisation per sweep: the host reads the sweep records, ends the instances the device has
    // ended (no rotation, or the cap) and takes their items out of the table, so the grids shrink with the instances still rotating.
    int factor_split(const BatchCore& c, const std::vector<int>& tk, const std::vector<FactorDesc>& launch) {
        const int n = (int)tk.size();
        std::vector<FactorSpan> spans((size_t)n);
        std::vector<FactorItem> items;
        int nslot = 0;
        for (int t = 0; t < n; ++t) {
            const int K = launch[t].K, parts = fs.parts[tk[t]];
            const int P = factor_pairs(K), per = factor_item_pairs(K, parts), G = factor_item_count(K, parts);
            spans[t] = FactorSpan{nslot, G};
            for (int g = 0; g < G; ++g) items.push_back(FactorItem{t, g * per, std::min(per, P - g * per), factor_rounds(K), nslot++});
        }
        std::stable_sort(items.begin(), items.end(), [](const FactorItem& a, const FactorItem& b) { return a.rounds > b.rounds; });
        MMW_TRY(fs.d_spans.upload(spans, c.st));
        MMW_TRY(fs.d_items.upload(items, c.st));
        MMW_TRY(fs.slab.alloc((size_t)nslot * FSPLIT_SLOT));
        MMW_TRY(fs.rec.alloc((size_t)n * FSPLIT_REC));
        hipLaunchKernelGGL(k_batch_factor_head, dim3((unsigned)n), dim3(BATCH_THREADS), 0, c.st, d_fdesc.p, fs.d_spans.p, c.ia.p, c.fa.p, ew.p, fs.slab.p, fs.rec.p,
                           lists_i(c), lists_f(c));
        int64_t launches = 1, sweeps = 0;
        size_t widest = std::max((size_t)n, items.size());
        std::vector<char> live((size_t)n, 1);
        std::vector<double> rec((size_t)n * FSPLIT_REC);
        int nlive = n;
        while (nlive > 0 && sweeps < EPI_SWEEP_CAP) {
            size_t cnt = items.size();  // items with more than r rounds: a prefix of the table
            for (int r = 0;; ++r) {
                while (cnt > 0 && items[cnt - 1].rounds <= r) --cnt;
                if (cnt == 0) break;
                hipLaunchKernelGGL(k_batch_factor_round, dim3((unsigned)cnt), dim3(BATCH_THREADS), 0, c.st, d_fdesc.p, fs.d_items.p, ew.p, fs.slab.p, fs.rec.p, r);
                ++launches;
            }
            hipLaunchKernelGGL(k_batch_factor_sweep, dim3((unsigned)n), dim3(WAVE), 0, c.st, d_fdesc.p, fs.d_spans.p, fs.slab.p, fs.rec.p);
            ++launches;
            ++sweeps;
            MMW_HIP(hipGetLastError());
            MMW_TRY(copy_d2h(rec.data(), fs.rec.p, rec.size() * sizeof(double), c.st));
            bool ended = false;
            for (int t = 0; t < n; ++t)
                if (live[t] && rec[(size_t)t * FSPLIT_REC + 3] != 0.0) { live[t] = 0; --nlive; ended = true; }
            if (ended && nlive > 0) {
                std::vector<FactorItem> keep;
                for (const FactorItem& w : items)
                    if (live[w.inst]) keep.push_back(w);
                items = std::move(keep);
                MMW_TRY(fs.d_items.upload(items, c.st));
            }
        }
        hipLaunchKernelGGL(k_batch_factor_tail, dim3((unsigned)n), dim3(BATCH_THREADS), 0, c.st, d_fdesc.p, fs.rec.p, ew.p, ei.p);
        ++launches;
        fs.call[0] = 1.0; fs.call[1] = (double)launches; fs.call[2] = (double)sweeps; fs.call[3] = (double)widest;
        return MMW_OK;
    }
    // spectral_sdp_solver.run_with_state (sdp_solver.py:165-185): the row-normalised top-Z eigenvector block of the state's Laplacian as
    // the resident factor, rank Z (kernels_batch_spectral.h); the Jacobi, its split and its records are mmw_batch_factor's
    int factor_spectral(const BatchCore& c, const int32_t* take, const int32_t* Z) {
        if (c.host_only) return BatchCore::host_only_batch();
        std::vector<int> tk;
        MMW_TRY(c.takers("mmw_batch_factor_spectral", take, tk));
        for (int b : tk) {
            const BatchDesc& d = c.desc[b];
            const std::string who = "mmw_batch_factor_spectral: instance " + std::to_string(b);
            if (d.K > EPI_MAX_K) return fail(MMW_ERR_ARG, who + ": K = " + std::to_string(d.K) + " exceeds the epilogue limit " + std::to_string(EPI_MAX_K) + " (spectral_sdp_solver takes it on the host)");
            const int z = Z ? Z[b] : d.Z;
            if (z < 1 || z > d.K) return fail(MMW_ERR_ARG, who + ": Z = " + std::to_string(z) + " must be in [1, K = " + std::to_string(d.K) + "]");
        }
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(round_lists(c));
        std::vector<FactorDesc> fd(c.B, FactorDesc{});
        std::vector<FactorDesc> launch;
        int64_t of = a32((int64_t)tk.size() * EPI_INFO_STRIDE), oi = 0, ninfo = 0;
        for (int b : tk) {
            FactorDesc& f = fd[b];
            const int64_t K = c.desc[b].K;
            f.kind = 1; f.unit_rows = 1; f.div = 1.0;
            f.K = (int)K; f.rank = Z ? Z[b] : c.desc[b].Z; f.cap = EPI_SWEEP_CAP;
            f.s_soptr = rlists[b].soptr; f.s_soidx = rlists[b].soidx; f.s_sodata = rlists[b].sodata;
            f.o_info = EPI_INFO_STRIDE * ninfo++;
            f.o_A = of; of = a32(of + K * K);
            f.o_fac = of; of = a32(of + K * f.rank);
            f.o_nrm = of; of = a32(of + K);
            f.o_rown = of; of = a32(of + K);
            f.o_ord = oi; oi = a32(oi + K);
            launch.push_back(f);
        }
        return run_factor(c, tk, fd, launch, of, oi, nullptr);
    }
    // rand_sdp_solver.run_with_state (sdp_solver.py:109-114): the instance's sketch of (seed, iteration 0) as its resident factor, rank D
    int factor_random(const BatchCore& c, const int32_t* take, const uint64_t* seeds) {
        if (c.host_only) return BatchCore::host_only_batch();
        std::vector<int> tk;
        MMW_TRY(c.takers("mmw_batch_factor_random", take, tk));
        for (int b : tk)
            if (c.desc[b].K > EPI_MAX_K)
                return fail(MMW_ERR_ARG, "mmw_batch_factor_random: instance " + std::to_string(b) + ": K = " + std::to_string(c.desc[b].K) +
                                             " exceeds the epilogue limit " + std::to_string(EPI_MAX_K) + " (round it on a handle)");
        std::vector<FactorDesc> fd(c.B, FactorDesc{});
        std::vector<FactorRandomDesc> launch;
        int64_t of = a32((int64_t)tk.size() * EPI_INFO_STRIDE), ninfo = 0;
        for (int b : tk) {
            FactorDesc& f = fd[b];
            f.K = c.desc[b].K; f.rank = c.desc[b].D; f.unit_rows = 1;
            f.o_info = EPI_INFO_STRIDE * ninfo++;
            f.o_fac = of; of = a32(of + (int64_t)f.K * f.rank);
            launch.push_back(FactorRandomDesc{f.K, f.rank, seeds[b], f.o_fac, f.o_info});
        }
        on_restart();  // the buffers are laid out anew: earlier factors are gone whatever happens below
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(ew.alloc((size_t)of));
        MMW_TRY(d_frdesc.upload(launch, c.st));
        hipLaunchKernelGGL(k_batch_factor_random, dim3((unsigned)launch.size()), dim3(BATCH_THREADS), 0, c.st, d_frdesc.p, ew.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(c.st));
        fdesc = std::move(fd);
        return MMW_OK;
    }
    // MMW_F_FACTOR / MMW_F_FACTOR_INFO / MMW_F_FACTOR_ROWNORM of the instance's resident factor
    int read(const BatchCore& c, int b, int which, double* out, int64_t n) {
        if (!has_factor(b)) return no_factor("mmw_batch_read_f64", b);
        const FactorDesc& f = fdesc[b];
        if (which == MMW_F_FACTOR_ROWNORM && f.kind != 1)
            return fail(MMW_ERR_STATE, "mmw_batch_read_f64: instance " + std::to_string(b) + ": its factor is not a spectral one (mmw_batch_factor_spectral)");
        const int64_t len = which == MMW_F_FACTOR ? (int64_t)f.K * f.rank : which == MMW_F_FACTOR_ROWNORM ? (int64_t)f.K : EPI_INFO;
        if (n != len) return fail(MMW_ERR_ARG, "mmw_batch_read_f64: wrong length " + std::to_string(n) + ", expected " + std::to_string(len));
        MMW_HIP(hipSetDevice(c.device));
        const int64_t o = which == MMW_F_FACTOR ? f.o_fac : which == MMW_F_FACTOR_ROWNORM ? f.o_rown : f.o_info;
        return copy_d2h(out, ew.p + o, (size_t)len * sizeof(double), c.st);
    }
    // the rounding lists of the state the batch was built from, all instances, once
    int round_lists(const BatchCore& c) {
        if (!rlists.empty()) return MMW_OK;
        std::vector<RoundLists> rl(c.B);
        if (c.on_device) {  // the lists are on the device already, in the layout the environment gave them
            for (int b = 0; b < c.B; ++b) {
                const BatchPatItem& t = c.sat[b];
                rl[b] = {t.c_soptr, t.c_soidx, t.c_qptr, t.c_qidx, t.v_soval, t.v_sohmax, t.v_hmax};
            }
            rlists = std::move(rl);
            return MMW_OK;
        }
        std::vector<int> hi;
        std::vector<double> hf;
        auto pad = [](auto& v) { v.resize((v.size() + 31) & ~(size_t)31); };
        for (int b = 0; b < c.B; ++b) {
            const HostPattern& P = c.H[b];
            RoundLists& r = rl[b];
            r.soptr = (int64_t)hi.size(); hi.insert(hi.end(), P.so_indptr.begin(), P.so_indptr.end());
            r.soidx = (int64_t)hi.size(); hi.insert(hi.end(), P.so_indices.begin(), P.so_indices.end());
            r.qptr = (int64_t)hi.size(); hi.insert(hi.end(), P.q_indptr.begin(), P.q_indptr.end());
            r.qidx = (int64_t)hi.size(); hi.insert(hi.end(), P.q_indices.begin(), P.q_indices.end());
            pad(hi);
            r.sodata = (int64_t)hf.size(); hf.insert(hf.end(), P.so_data.begin(), P.so_data.end());
            r.sohmax = (int64_t)hf.size();
            for (int32_t n : P.so_indices) hf.push_back(P.h_max[n]);
            r.hmax = (int64_t)hf.size(); hf.insert(hf.end(), P.h_max.begin(), P.h_max.end());
            pad(hf);
        }
        MMW_TRY(rs_i.upload(hi, c.st));
        MMW_TRY(rs_f.upload(hf, c.st));
        rlists = std::move(rl);
        return MMW_OK;
    }
    // The rounding lists of another state of the same users (mmw_batch_round_env, batch_env_handle.h): where they lie, and per
    // instance their offsets.  Null: the lists of the state the batch was built from.
    struct RoundSource {
        const char* who;
        const int* si;
        const double* sf;
        const RoundLists* lists;  // [B]
        const int* K;             // [B] users of every instance of the other state
    };
    int round(const BatchCore& c, const int32_t* take, int32_t nattempt, int stop_at_first, const uint64_t* seeds, int32_t* z_out, int32_t* rem_out,
              int32_t* used_out, const RoundSource* src = nullptr) {
        const std::string who = src ? src->who : "mmw_batch_round";
        if (c.host_only) return BatchCore::host_only_batch();
        if (nattempt < 1 || nattempt > 4096) return fail(MMW_ERR_ARG, who + ": nattempt must be in [1, 4096]");
        std::vector<int> tk;
        MMW_TRY(c.takers(who.c_str(), take, tk));
        for (int b : tk) {
            if (!has_factor(b) || fdesc[b].K != c.desc[b].K) return no_factor(who, b);
            if (src && src->K[b] != c.desc[b].K)
                return fail(MMW_ERR_ARG, who + ": instance " + std::to_string(b) + ": K = " + std::to_string(c.desc[b].K) + " in the batch, " +
                                             std::to_string(src->K[b]) + " in the environment");
        }
        MMW_HIP(hipSetDevice(c.device));
        if (!src) MMW_TRY(round_lists(c));
        std::vector<RoundDesc> rd;
        int64_t of = 0, oi = 0;
        for (int b : tk) oi += (int64_t)nattempt * fdesc[b].K + nattempt + 1;  // slots, remainders and attempts run of every instance: what goes back
        const int64_t nback = oi;
        oi = a32(oi);
        int64_t oz = 0;
        for (int b : tk) {
            const FactorDesc& f = fdesc[b];
            const int64_t K = f.K, Z = c.desc[b].Z;
            RoundDesc r{};
            r.K = f.K; r.Z = c.desc[b].Z; r.Dp = f.rank; r.nattempt = nattempt; r.stop_first = stop_at_first != 0;
            r.index_order = f.unit_rows;
            r.seed = seeds[b];
            r.o_fac = f.o_fac;
            set_lists(r, src ? src->lists[b] : rlists[b]);
            r.r_randv = of; of = a32(of + Z * f.rank);
            r.r_inprod = of; of = a32(of + K * Z);
            r.r_gain = of; of = a32(of + K * Z);
            r.r_nrm = of; of = a32(of + K);
            r.r_order = oi; oi = a32(oi + K);
            r.r_pref = oi; oi = a32(oi + K * Z);
            r.r_z = oz; oz += (int64_t)nattempt * K;
            r.r_rem = oz; oz += nattempt + 1;
            rd.push_back(r);
        }
        MMW_TRY(rw.alloc((size_t)of));
        MMW_TRY(ri.alloc((size_t)oi));
        MMW_TRY(d_rdesc.alloc(rd.size()));
        MMW_TRY(copy_h2d(d_rdesc.p, rd.data(), rd.size() * sizeof(RoundDesc), c.st));
        hipLaunchKernelGGL(k_batch_round, dim3((unsigned)rd.size()), dim3(BATCH_THREADS), 0, c.st, d_rdesc.p, ew.p, src ? src->si : lists_i(c),
                           src ? src->sf : lists_f(c), rw.p, ri.p);
        MMW_HIP(hipGetLastError());
        MMW_HIP(hipStreamSynchronize(c.st));
        std::vector<int> host((size_t)nback);
        MMW_TRY(copy_d2h(host.data(), ri.p, host.size() * sizeof(int), c.st));
        for (int b = 0; b < c.B; ++b) {
            used_out[b] = 0;
            for (int a = 0; a < nattempt; ++a) rem_out[(size_t)b * nattempt + a] = -1;
        }
        int32_t* z = z_out;
        for (size_t t = 0; t < tk.size(); ++t) {
            const RoundDesc& r = rd[t];
            const size_t nz = (size_t)nattempt * r.K;
            std::copy(host.begin() + r.r_z, host.begin() + r.r_z + nz, z);
            z += nz;
            std::copy(host.begin() + r.r_rem, host.begin() + r.r_rem + nattempt, rem_out + (size_t)tk[t] * nattempt);
            used_out[tk[t]] = host[r.r_rem + nattempt];
        }
        return MMW_OK;
    }
    int round_randv(const BatchCore& c, int b, uint64_t seed, int32_t attempt, double* out, int64_t n) {
        MMW_TRY(c.check_inst(b));
        if (c.host_only) return BatchCore::host_only_batch();
        if (attempt < 0) return fail(MMW_ERR_ARG, "mmw_batch_round_randv: attempt must be >= 0");
        if (!has_factor(b)) return no_factor("mmw_batch_round_randv", b);
        const int Z = c.desc[b].Z, Dp = fdesc[b].rank;
        if (n != (int64_t)Z * Dp) return fail(MMW_ERR_ARG, "mmw_batch_round_randv: wrong length for a Z x rank block");
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(rvbuf.alloc((size_t)n));
        hipLaunchKernelGGL(k_batch_randv, dim3(1), dim3(BATCH_THREADS), 0, c.st, Z, Dp, seed, (uint32_t)attempt, rvbuf.p);
        MMW_HIP(hipGetLastError());
        return copy_d2h(out, rvbuf.p, (size_t)n * sizeof(double), c.st);
    }
};
