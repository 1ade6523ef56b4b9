// The head split of mmw_batch_iterate (mmw_batch_set_head_split, kernels_batch_head.h): row parts per instance for everything in front
// of the exponential and for the row sums behind it.  BatchSplit::run and BatchRows::run (batch_iterate.h, batch_rows.h) keep their
// loops and call front / plan / x below where they launch k_batch_split_head / k_batch_rows_plan / k_batch_split_x without it.  The
// work table, the LOSS constants and the plan's per-row scratch are buffers of its own.
#pragma once
#include "batch_core.h"
#include "kernels_batch_head.h"

struct BatchHead {
    std::vector<int> parts;  // head parts per instance (empty: one each, the head on one workgroup)
    DevBuf<HeadWork> d_work;
    DevBuf<int64_t> soff;     // per instance: where its (dg[K], o[K]) start in scr
    DevBuf<double> dcon, scr;
    int64_t launches = 0, widest = 0;                // of the call in progress
    double call[4] = {0.0, 0.0, 0.0, 0.0};           // MMW_F_HEAD_CALL: the last mmw_batch_iterate {on, head-path launches, widest of them, 0}
    int set(const BatchCore& c, const int32_t* p) {
        return c.host_only ? BatchCore::host_only_batch() : check_parts("mmw_batch_set_head_split", p, c.B, parts, MMW_BATCH_MAX_HEAD_PARTS);
    }
    bool wanted(const std::vector<BatchDesc>& dd) const {
        for (size_t b = 0; b < dd.size() && !parts.empty(); ++b)
            if (dd[b].nrun > 0 && parts[b] > 1) return true;
        return false;
    }
    void off() { call[0] = call[1] = call[2] = call[3] = 0.0; }
    void done() { call[0] = 1.0; call[1] = (double)launches; call[2] = (double)widest; call[3] = 0.0; }
    // the call's work table and scratch: one workgroup per (running instance, row part), the ranges those of batch_row_bounds
    int stage(const BatchCore& c, const std::vector<BatchDesc>& dd) {
        std::vector<HeadWork> wk;
        std::vector<int64_t> so((size_t)c.B, 0);
        std::vector<int32_t> bd;
        int64_t ns = 0;
        for (int b = 0; b < c.B; ++b) {
            const BatchDesc& d = dd[b];
            so[b] = ns;
            if (d.nrun <= 0) continue;
            ns += 2 * (int64_t)d.K;
            const int hp = parts[b];
            bd.resize((size_t)hp + 1);
            batch_row_bounds(c.pat(b).l_indptr.data(), d.K, hp, bd.data());
            for (int p = 0; p < hp; ++p) wk.push_back(HeadWork{b, p, hp, bd[p], bd[p + 1]});
        }
        MMW_TRY(d_work.upload(wk, c.st));
        MMW_TRY(soff.upload(so, c.st));
        MMW_TRY(dcon.alloc((size_t)c.B));
        MMW_TRY(scr.alloc((size_t)ns));
        launches = 0;
        widest = 0;
        return MMW_OK;
    }
    void count(int64_t n, int64_t width) { launches += n; widest = std::max(widest, width); }
    // [gap] avg, dual, fold, loss of iteration `it`; gd null: the gap is off
    void front(const BatchCore& c, const GapDesc* gd, double* ga, int it) {
        const dim3 per_part((unsigned)d_work.n), per_inst((unsigned)c.B), nt(BATCH_THREADS);
        hipStream_t st = c.st;
        if (gd) hipLaunchKernelGGL(k_batch_head_gap, per_inst, nt, 0, st, c.d_desc.p, c.ia.p, c.fa.p, gd, ga, it);
        hipLaunchKernelGGL(k_batch_head_avg, per_part, nt, 0, st, c.d_desc.p, d_work.p, c.ia.p, c.fa.p, it);
        hipLaunchKernelGGL(k_batch_head_dual, per_part, nt, 0, st, c.d_desc.p, d_work.p, c.ia.p, c.fa.p, it);
        hipLaunchKernelGGL(k_batch_head_fold, per_inst, nt, 0, st, c.d_desc.p, c.fa.p, dcon.p, it);
        hipLaunchKernelGGL(k_batch_head_loss, per_part, nt, 0, st, c.d_desc.p, d_work.p, c.ia.p, c.fa.p, dcon.p, soff.p, scr.p, it);
        count(gd ? 5 : 4, std::max<int64_t>((int64_t)d_work.n, c.B));
    }
    // the row-split path's plan, from the (dg, o) front left
    void plan(const BatchCore& c, double* rec, const int* pending, int nsid, int* cnt, int it) {
        hipLaunchKernelGGL(k_batch_head_plan, dim3((unsigned)c.B), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, c.fa.p, soff.p, scr.p, rec, pending, nsid, cnt, it);
        count(1, c.B);
    }
    // the row sums of X_half, then X on the pattern over the path's entry ranges
    void x(const BatchCore& c, const DevBuf<SplitRange>& wx, const double* slab, int it) {
        hipLaunchKernelGGL(k_batch_head_xrows, dim3((unsigned)d_work.n), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, d_work.p, c.fa.p, it);
        hipLaunchKernelGGL(k_batch_head_x, dim3((unsigned)wx.n), dim3(BATCH_THREADS), 0, c.st, c.d_desc.p, wx.p, c.ia.p, c.fa.p, slab, it);
        count(2, std::max<int64_t>((int64_t)d_work.n, (int64_t)wx.n));
    }
};
