// The row split of mmw_batch_iterate (mmw_batch_set_row_split, kernels_batch_rows.h): row parts per instance, multiplied with the
// column slices of BatchSplit.  The work tables, the plan records, the slabs and the stop state are buffers of its own.
#pragma once
#include "batch_iterate.h"
#include "kernels_batch_rows.h"

struct BatchRows {
    std::vector<int> rows;  // row parts per instance (empty: one each)
    DevBuf<RowsWork> d_work;
    DevBuf<SplitRange> d_wx;
    DevBuf<double> rec, slab_t, slab_f, st_prev, deg;
    DevBuf<int> st_on, flags, cnt;
    double call[4] = {0.0, 0.0, 0.0, 0.0};  // MMW_F_SPLIT_CALL: the last mmw_batch_iterate {path, launches, idle launches, widest launch}
    int set(const BatchCore& c, const int32_t* p) {
        return c.host_only ? BatchCore::host_only_batch() : check_parts("mmw_batch_set_row_split", p, c.B, rows, MMW_BATCH_MAX_ROW_PARTS);
    }
    bool wanted(const std::vector<BatchDesc>& dd) const {
        for (size_t b = 0; b < dd.size() && !rows.empty(); ++b)
            if (dd[b].nrun > 0 && rows[b] > 1) return true;
        return false;
    }
    void record(int path, int64_t launches, int64_t idle, int64_t widest) {
        call[0] = path; call[1] = (double)launches; call[2] = (double)idle; call[3] = (double)widest;
    }
    // One iteration as head, plan, the launches of the longest schedule and x, for all instances (kernels_batch_rows.h); `dd` is on the
    // device already.  colparts: BatchSplit's setting (empty: one slice each).  head: the staged head split (batch_head.h) while it is
    // on -- its launches stand for k_batch_split_head, k_batch_rows_plan and k_batch_split_x -- else null.
    int run(const BatchCore& c, const BatchGap& gap, const std::vector<int>& colparts, const std::vector<BatchDesc>& dd, const double* rv,
            BatchHead* head = nullptr) {
        std::vector<RowsWork> wk;
        std::vector<SplitRange> wx;
        std::vector<int32_t> bd;
        int nmax = 0, nsid = 0;
        int64_t nslab = 0;
        for (int b = 0; b < c.B; ++b) {
            const BatchDesc& d = dd[b];
            if (d.nrun <= 0) continue;
            nmax = std::max(nmax, d.nrun);
            const int cp = colparts.empty() ? 1 : colparts[b], rp = rows[b];
            const int W = split_width(d.D, cp), G = split_slices(d.D, cp), sid0 = nsid;
            bd.resize((size_t)rp + 1);
            batch_row_bounds(c.pat(b).l_indptr.data(), d.K, rp, bd.data());
            for (int g = 0; g < G; ++g) {
                for (int p = 0; p < rp; ++p) wk.push_back(RowsWork{b, g, W, p, rp, bd[p], bd[p + 1], (int)nslab, nsid});
                nslab += (int64_t)rp * W;
                ++nsid;
            }
            for (int p = 0; p < G * rp; ++p) wx.push_back(SplitRange{b, p, G * rp, sid0, G});
        }
        hipStream_t st = c.st;
        MMW_TRY(d_work.upload(wk, st));
        MMW_TRY(d_wx.upload(wx, st));
        MMW_TRY(rec.alloc((size_t)ROWS_REC * c.B));
        MMW_TRY(slab_t.alloc((size_t)2 * nslab));
        MMW_TRY(slab_f.alloc((size_t)2 * nslab));
        MMW_TRY(st_prev.alloc((size_t)nslab));
        MMW_TRY(st_on.alloc((size_t)nslab));
        MMW_TRY(deg.alloc((size_t)nsid));
        MMW_TRY(flags.alloc((size_t)2 * nsid));
        MMW_TRY(cnt.alloc(1));
        MMW_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int), st));
        std::vector<double> hrec((size_t)ROWS_REC * c.B);
        int64_t launches = 0;
        const int* pending = nullptr;  // the flags of an iteration's last step launch, tallied by the next plan launch
        const unsigned nwk = (unsigned)wk.size();
        for (int it = 0; it < nmax; ++it) {
            if (head)
                head->front(c, gap.on ? gap.d_gdesc.p : nullptr, gap.ga.p, it);
            else if (gap.on)
                hipLaunchKernelGGL(k_batch_split_head<true>, dim3(c.B), dim3(BATCH_THREADS), 0, st, c.d_desc.p, c.ia.p, c.fa.p, gap.d_gdesc.p, gap.ga.p, it);
            else
                hipLaunchKernelGGL(k_batch_split_head<false>, dim3(c.B), dim3(BATCH_THREADS), 0, st, c.d_desc.p, c.ia.p, c.fa.p, (const GapDesc*)nullptr, (double*)nullptr, it);
            if (head)
                head->plan(c, rec.p, pending, nsid, cnt.p, it);
            else
                hipLaunchKernelGGL(k_batch_rows_plan, dim3(c.B), dim3(BATCH_THREADS), 0, st, c.d_desc.p, c.ia.p, c.fa.p, rec.p, pending, nsid, cnt.p, it);
            MMW_HIP(hipGetLastError());
            MMW_TRY(copy_d2h(hrec.data(), rec.p, hrec.size() * sizeof(double), st));  // the iteration's one synchronisation
            int lmax = 0;
            for (int b = 0; b < c.B; ++b)
                if (it < dd[b].nrun) lmax = std::max(lmax, (int)hrec[(size_t)ROWS_REC * b + 2] * (1 + (int)hrec[(size_t)ROWS_REC * b + 3]));
            for (int l = 0; l < lmax; ++l)
                hipLaunchKernelGGL(k_batch_rows_step, dim3(nwk), dim3(BATCH_THREADS), 0, st, c.d_desc.p, d_work.p, rec.p, c.ia.p, c.fa.p, rv, slab_t.p,
                                   slab_f.p, st_prev.p, st_on.p, deg.p, flags.p, cnt.p, (int)nslab, nsid, it, l);
            pending = flags.p + (size_t)((lmax - 1) & 1) * nsid;
            if (head)
                head->x(c, d_wx, deg.p, it);
            else
                hipLaunchKernelGGL(k_batch_split_x, dim3((unsigned)wx.size()), dim3(BATCH_THREADS), 0, st, c.d_desc.p, d_wx.p, c.ia.p, c.fa.p, deg.p, it);
            MMW_HIP(hipGetLastError());
            launches += head ? lmax : 2 + lmax + 1;
        }
        // the record: the idle launches the device tallied, and the last launch's flags read here
        std::vector<int> hf((size_t)nsid);
        int idle = 0;
        MMW_TRY(copy_d2h(&idle, cnt.p, sizeof(int), st));
        MMW_TRY(copy_d2h(hf.data(), pending, hf.size() * sizeof(int), st));
        idle += std::all_of(hf.begin(), hf.end(), [](int x) { return x == 0; });
        if (head) launches += head->launches;
        record(2, launches, idle, std::max<int64_t>(std::max<int64_t>(std::max<int64_t>(nwk, (int64_t)wx.size()), c.B), head ? head->widest : 0));
        return MMW_OK;
    }
};
