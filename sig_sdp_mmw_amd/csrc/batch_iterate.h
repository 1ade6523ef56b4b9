// The two options of mmw_batch_iterate, each with the buffers it owns: the duality-gap log (mmw_batch_set_gap, kernels_batch.h) and the
// split of an instance over several workgroups (mmw_batch_set_split, kernels_batch_split.h).
#pragma once
#include "batch_core.h"
#include "batch_head.h"
#include "kernels_batch_split.h"

// The gap log: a buffer of its own, made when the gap is first enabled, so the arenas do not move.
struct BatchGap {
    bool ever = false, on = false;
    int mcap = GAP_DEFAULT_M;
    std::vector<GapDesc> gdesc;
    DevBuf<double> ga;
    DevBuf<GapDesc> d_gdesc;
    // offsets of every instance's gap work space (nnzL + 5 K doubles, all instances first) and log (4 doubles per announced
    // iteration, all logs after the work spaces); every log row NaN
    int layout(const BatchCore& c) {
        gdesc.assign(c.B, GapDesc{});
        int64_t og = 0;
        for (int b = 0; b < c.B; ++b) { gdesc[b].o_work = og; og = a32(og + (int64_t)c.desc[b].nnzL + 5 * (int64_t)c.desc[b].K); }
        const int64_t log0 = og;
        for (int b = 0; b < c.B; ++b) { gdesc[b].o_log = og; og = a32(og + 4 * (int64_t)c.nit[b]); }
        const std::vector<double> init((size_t)(og - log0), std::numeric_limits<double>::quiet_NaN());
        MMW_HIP(hipSetDevice(c.device));
        MMW_TRY(ga.alloc((size_t)og));
        MMW_TRY(copy_h2d(ga.p + log0, init.data(), init.size() * sizeof(double), c.st));
        MMW_TRY(d_gdesc.alloc((size_t)c.B));
        return MMW_OK;
    }
    int set(const BatchCore& c, int enabled, int32_t m_cap) {
        if (c.host_only) return BatchCore::host_only_batch();
        if (m_cap > GAP_MAX_M) return fail(MMW_ERR_ARG, "mmw_batch_set_gap: m_cap must be at most " + std::to_string(GAP_MAX_M));
        if (enabled && !ever) { MMW_TRY(layout(c)); ever = true; }
        on = enabled != 0;
        mcap = m_cap <= 0 ? GAP_DEFAULT_M : m_cap;
        return MMW_OK;
    }
    int read(const BatchCore& c, int b, double* out, int64_t n) {
        MMW_TRY(c.check_inst(b));
        if (c.host_only) return BatchCore::host_only_batch();
        if (!ever) return fail(MMW_ERR_STATE, "mmw_batch_read_gap: the gap was never enabled on this batch (mmw_batch_set_gap)");
        if (n != 4 * (int64_t)c.iter[b]) return fail(MMW_ERR_ARG, "mmw_batch_read_gap: wrong length " + std::to_string(n) + ", expected 4 x " + std::to_string(c.iter[b]) + " iterations done");
        if (n == 0) return MMW_OK;
        MMW_HIP(hipSetDevice(c.device));
        return copy_d2h(out, ga.p + gdesc[b].o_log, (size_t)n * sizeof(double), c.st);
    }
    // the call's descriptors on the device, when the gap is on
    int stage(const BatchCore& c) {
        if (!on) return MMW_OK;
        for (int b = 0; b < c.B; ++b) gdesc[b].m_cap = mcap;
        return copy_h2d(d_gdesc.p, gdesc.data(), gdesc.size() * sizeof(GapDesc), c.st);
    }
    int on_restart(const BatchCore& c) { return ever ? layout(c) : MMW_OK; }  // an empty log for the new run
};

// Workgroups per instance (empty: one each, the single-launch kernel); the work tables and the slab of per-slice Taylor degrees are
// buffers of its own, rebuilt from `parts` and the current D per call.
struct BatchSplit {
    std::vector<int> parts;
    DevBuf<SplitSlice> d_wexpm;
    DevBuf<SplitRange> d_wx;
    DevBuf<double> slab;
    int set(const BatchCore& c, const int32_t* p) { return c.host_only ? BatchCore::host_only_batch() : check_parts("mmw_batch_set_split", p, c.B, parts); }
    bool wanted(const std::vector<BatchDesc>& dd) const {
        for (size_t b = 0; b < dd.size() && !parts.empty(); ++b)
            if (dd[b].nrun > 0 && parts[b] > 1) return true;
        return false;
    }
    // One iteration as three launches for all instances (kernels_batch_split.h); `dd` is on the device already.  head: the staged
    // head split (batch_head.h) while it is on -- its launches stand for k_batch_split_head and k_batch_split_x -- else null.
    int run(const BatchCore& c, const BatchGap& gap, const std::vector<BatchDesc>& dd, const double* rv, BatchHead* head = nullptr) {
        std::vector<SplitSlice> we;
        std::vector<SplitRange> wx;
        int nmax = 0;
        for (int b = 0; b < c.B; ++b) {
            const BatchDesc& d = dd[b];
            if (d.nrun <= 0) continue;
            nmax = std::max(nmax, d.nrun);
            const int cp = parts.empty() ? 1 : parts[b];  // (empty: the head split alone is on)
            const int W = split_width(d.D, cp), G = split_slices(d.D, cp), slab0 = (int)we.size();
            for (int g = 0; g < G; ++g) we.push_back(SplitSlice{b, g, W, slab0 + g});
            for (int p = 0; p < cp; ++p) wx.push_back(SplitRange{b, p, cp, slab0, G});
        }
        MMW_TRY(d_wexpm.upload(we, c.st));
        MMW_TRY(d_wx.upload(wx, c.st));
        MMW_TRY(slab.alloc(we.size()));
        for (int it = 0; it < nmax; ++it) {
            if (head)
                head->front(c, gap.on ? gap.d_gdesc.p : nullptr, gap.ga.p, it);
            else if (gap.on)
                hipLaunchKernelGGL(k_batch_split_head<true>, dim3(c.B), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, c.ia.p, c.fa.p, gap.d_gdesc.p, gap.ga.p, it);
            else
                hipLaunchKernelGGL(k_batch_split_head<false>, dim3(c.B), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, c.ia.p, c.fa.p, (const GapDesc*)nullptr, (double*)nullptr, it);
            hipLaunchKernelGGL(k_batch_split_expm, dim3((unsigned)we.size()), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, d_wexpm.p, c.ia.p, c.fa.p, rv, slab.p, it);
            if (head)
                head->x(c, d_wx, slab.p, it);
            else
                hipLaunchKernelGGL(k_batch_split_x, dim3((unsigned)wx.size()), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, d_wx.p, c.ia.p, c.fa.p, slab.p, it);
        }
        return MMW_OK;
    }
};
