// Developer reports on stderr, as free functions: the phase stamps of a diagnostic launch (MMW_STAMPS, MMW_SD_STAMPS, MMW_DUAL_STAMPS), the host blockings' statistics.
#pragma once
#include <map>

#include "blocking.h"
#include "pattern.h"
#include "runtime.h"

namespace mmw {

// Phase stamps of one diagnostic launch: allocated and zeroed on request; p() stays null otherwise, and a kernel handed null writes none.
struct StampBuf {
    DevBuf<unsigned long long> buf;
    unsigned long long* p() const { return buf.p; }
    int request(bool want, size_t n, hipStream_t st) {
        if (!want) return MMW_OK;
        MMW_TRY(buf.alloc(n));
        MMW_HIP(hipMemsetAsync(buf.p, 0, n * sizeof(unsigned long long), st));
        return MMW_OK;
    }
};
// diagnostic: per-workgroup phase stamps written by a blocked kernel (16 slots per workgroup, slot 9 = end,
// 10 = HW_ID, 11 = XCC_ID): mean time per phase and how many workgroups were resident per CU
inline int dump_stamps(hipStream_t st, const unsigned long long* dev) {
    std::vector<unsigned long long> h((size_t)16 * 8192);
    MMW_HIP(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MMW_HIP(hipStreamSynchronize(st));
    double acc[10] = {0};
    int cnt = 0;
    unsigned long long tmin = ~0ull, tmax = 0;
    for (int w = 0; w < 8192; ++w) {
        const unsigned long long* q = &h[(size_t)w * 16];
        if (!q[0] || !q[9]) continue;
        ++cnt;
        tmin = std::min(tmin, q[0]);
        tmax = std::max(tmax, q[9]);
        for (int k = 1; k < 10; ++k) if (q[k] && q[k - 1]) acc[k] += (double)(q[k] - q[k - 1]);
    }
    fprintf(stderr, "[stamps] %d workgroups, span %.1f us; mean us per phase:", cnt, (double)(tmax - tmin) * 0.01);
    for (int k = 1; k < 10; ++k) fprintf(stderr, " p%d=%.2f", k, acc[k] / std::max(cnt, 1) * 0.01);
    {
        double g = 0; int c = 0;
        for (int w = 0; w < 8192; ++w) {
            const unsigned long long* q = &h[(size_t)w * 16];
            if (q[4] && q[12]) { g += (double)(q[12] - q[4]); ++c; }
        }
        if (c) fprintf(stderr, " gather-issue(p5 part)=%.2f", g / c * 0.01);
    }
    fprintf(stderr, "\n");
    // residency: workgroups whose [start, end) intervals overlap on the same (XCC, SE, SH, CU)
    std::map<unsigned long long, std::vector<std::pair<unsigned long long, int>>> ev;
    double wgdur = 0;
    for (int w = 0; w < 8192; ++w) {
        const unsigned long long* q = &h[(size_t)w * 16];
        if (!q[0] || !q[9] || !q[10]) continue;
        const unsigned long long cu = ((q[11] & 0xF) << 16) | (q[10] & 0xFF00);  // xcc | se, sh, cu bits of HW_ID
        ev[cu].push_back({q[0], +1});
        ev[cu].push_back({q[9], -1});
        wgdur += (double)(q[9] - q[0]);
    }
    double t1 = 0, t2 = 0, t3 = 0;
    for (auto& kv : ev) {
        auto& v = kv.second;
        std::sort(v.begin(), v.end());
        int live = 0;
        for (size_t i = 0; i + 1 < v.size(); ++i) {
            live += v[i].second;
            const double dt = (double)(v[i + 1].first - v[i].first);
            if (live == 1) t1 += dt; else if (live == 2) t2 += dt; else if (live >= 3) t3 += dt;
        }
    }
    {   // the ten longest workgroups: when they started, how long they ran, where
        std::vector<std::pair<double, int>> byd;
        for (int w = 0; w < 8192; ++w) {
            const unsigned long long* q = &h[(size_t)w * 16];
            if (q[0] && q[9]) byd.push_back({(double)(q[9] - q[0]) * 0.01, w});
        }
        std::sort(byd.rbegin(), byd.rend());
        for (size_t i = 0; i < byd.size() && i < 10; ++i) {
            const unsigned long long* q = &h[(size_t)byd[i].second * 16];
            fprintf(stderr, "[stamps]   wg %4d start +%.1f us dur %.1f us first-tile %.1f us cu %llx\n", byd[i].second, (double)(q[0] - tmin) * 0.01,
                    byd[i].first, q[5] && q[4] ? (double)(q[5] - q[4]) * 0.01 : 0.0, ((q[11] & 0xF) << 16) | (q[10] & 0xFF00));
        }
        double late = 0; int nl = 0;
        for (auto& pr : byd) { const unsigned long long* q = &h[(size_t)pr.second * 16]; const double st0 = (double)(q[0] - tmin) * 0.01; if (st0 > 5.0) { late += st0; ++nl; } }
        fprintf(stderr, "[stamps]   %d workgroups started later than +5 us (mean +%.1f us)\n", nl, nl ? late / nl : 0.0);
        const size_t nd = byd.size();
        auto dur = [&](size_t i) { return byd[nd - 1 - i].first; };  // the durations in ascending order
        if (nd)
            fprintf(stderr, "[stamps] workgroup us: min %.1f p25 %.1f p50 %.1f p75 %.1f p95 %.1f max %.1f\n", dur(0), dur(nd / 4),
                    dur(nd / 2), dur(nd * 3 / 4), dur(nd * 95 / 100), dur(nd - 1));
    }
    if (!ev.empty())
        fprintf(stderr, "[stamps] %zu distinct CUs; mean workgroup %.2f us; per CU: %.1f us with 1 resident, %.1f us with 2, %.1f us with 3+\n", ev.size(),
                wgdur / std::max(cnt, 1) * 0.01, t1 / ev.size() * 0.01, t2 / ev.size() * 0.01, t3 / ev.size() * 0.01);
    return MMW_OK;
}
// MMW_DUAL_STAMPS: per-wave phase clocks of one fused DUAL launch (k_dual_h) of `gd` workgroups
inline int dump_dual_stamps(hipStream_t st, const unsigned long long* dev, int gd) {
    std::vector<unsigned long long> h((size_t)gd * WAVES_PER_BLOCK * 8);
    MMW_HIP(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MMW_HIP(hipStreamSynchronize(st));
    double sum[5] = {0}, slow[5] = {0};
    std::vector<std::pair<unsigned long long, size_t>> byl;
    int nw = 0;
    for (size_t w = 0; w < h.size() / 8; ++w) {
        const unsigned long long* q = &h[w * 8];
        if (!q[5]) continue;
        ++nw;
        const unsigned long long p1 = q[1] ? q[1] : q[0], p2 = q[2] ? q[2] : p1, p3 = q[3], p4 = q[4];
        sum[0] += (double)(p1 - q[0]); sum[1] += (double)(p2 - p1); sum[2] += (double)(p3 - p2); sum[3] += (double)(p4 - p3); sum[4] += (double)(q[5] - p4);
        byl.push_back({q[5] - q[0], w});
    }
    std::sort(byl.rbegin(), byl.rend());
    const size_t top = std::max<size_t>(1, byl.size() / 20);
    for (size_t i = 0; i < top && i < byl.size(); ++i) {
        const unsigned long long* q = &h[byl[i].second * 8];
        const unsigned long long p1 = q[1] ? q[1] : q[0], p2 = q[2] ? q[2] : p1;
        slow[0] += (double)(p1 - q[0]); slow[1] += (double)(p2 - p1); slow[2] += (double)(q[3] - p2); slow[3] += (double)(q[4] - q[3]); slow[4] += (double)(q[5] - q[4]);
    }
    if (nw)
        fprintf(stderr, "[dual stamps] %d workgroups, %d waves; clocks per wave: row pointers %.0f, rows (entries + gathers + sums) %.0f, rows' tails %.0f, violation part %.0f, fold + stores %.0f; "
                        "slowest twentieth: %.0f / %.0f / %.0f / %.0f / %.0f\n",  // (the counters of different XCDs share no origin: no launch-wide span)
                gd, nw, sum[0] / nw, sum[1] / nw, sum[2] / nw, sum[3] / nw, sum[4] / nw, slow[0] / top, slow[1] / top, slow[2] / top, slow[3] / top, slow[4] / top);
    return MMW_OK;
}
// MMW_SD_STAMPS: per-wave phase clocks of one matrix-core SDDMM launch (k_sddmm_mfma) of `grid` workgroups, `n_st` stamps
inline int dump_sddmm_stamps(hipStream_t st, const unsigned long long* dev, size_t n_st, dim3 grid, int mfma_mt) {
    std::vector<unsigned long long> h(n_st);
    MMW_HIP(hipMemcpyAsync(h.data(), dev, n_st * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MMW_HIP(hipStreamSynchronize(st));
    double sum[8] = {0}, life_max = 0;
    int nw = 0;
    for (size_t w = 0; w < n_st / 8; ++w) {
        const unsigned long long* q = &h[w * 8];
        if (!q[4]) continue;
        ++nw;
        for (int k = 0; k < 8; ++k) sum[k] += (double)q[k];
        life_max = std::max(life_max, (double)q[4]);
    }
    {   // the slowest twentieth of the waves: where their time went
        std::vector<std::pair<unsigned long long, size_t>> byl;
        for (size_t w = 0; w < n_st / 8; ++w) if (h[w * 8 + 4]) byl.push_back({h[w * 8 + 4], w});
        std::sort(byl.rbegin(), byl.rend());
        const size_t top = std::max<size_t>(1, byl.size() / 20);
        double ts[8] = {0};
        for (size_t i = 0; i < top && i < byl.size(); ++i) for (int k = 0; k < 8; ++k) ts[k] += (double)h[byl[i].second * 8 + k];
        if (!byl.empty())
            fprintf(stderr, "[sddmm stamps] slowest %zu waves: prologue %.0f, wait+barrier %.0f, issue %.0f, reads+products %.0f, sums %.0f, stores %.0f, lifetime %.0f; by (wg.y): ", top,
                    ts[0] / top, ts[1] / top, ts[2] / top, ts[3] / top, ts[5] / top, ts[7] / top, ts[4] / top);
        int cnt[8] = {0};
        for (size_t i = 0; i < top && i < byl.size(); ++i) { const size_t wg = byl[i].second / (size_t)(4 * mfma_mt); const unsigned y = (unsigned)(wg / grid.x); if (y < 8) ++cnt[y]; }
        for (unsigned y = 0; y < grid.y && y < 8; ++y) fprintf(stderr, "%d ", cnt[y]);
        fprintf(stderr, "\n");
    }
    if (nw)
        fprintf(stderr, "[sddmm stamps] grid %u x %u, %d working waves; shader clocks per wave: prologue %.0f, wait+barrier %.0f, issue %.0f, reads+products %.0f, "
                        "row/column sums %.0f, tile+stores+atomics %.0f, lifetime %.0f (max %.0f)\n",
                grid.x, grid.y, nw, sum[0] / nw, sum[1] / nw, sum[2] / nw, sum[3] / nw, sum[5] / nw, sum[7] / nw, sum[4] / nw, life_max);
    return MMW_OK;
}
// MMW_STAMPS on the matrix-core SpMM (mmw_bench_spmm): per-wave phase clocks of one launch
inline int dump_mf_stamps(hipStream_t st, const unsigned long long* dev) {
    std::vector<unsigned long long> h((size_t)16 * 8192);
    MMW_HIP(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MMW_HIP(hipStreamSynchronize(st));
    double sum[5] = {0}, steps = 0, life_max = 0, epi = 0;
    int n = 0;
    for (size_t w = 0; w < h.size() / 8; ++w) {
        const unsigned long long* q = &h[w * 8];
        if (!q[4]) continue;
        ++n;
        for (int k = 0; k < 5; ++k) sum[k] += (double)q[k];
        steps += (double)q[5];
        life_max = std::max(life_max, (double)q[4]);
        epi += (double)q[7];
    }
    {   // the slowest twentieth of the waves, and lifetime against the block's k-steps
        std::vector<std::pair<unsigned long long, size_t>> byl;
        for (size_t w = 0; w < h.size() / 8; ++w) if (h[w * 8 + 4]) byl.push_back({h[w * 8 + 4], w});
        std::sort(byl.rbegin(), byl.rend());
        const size_t top = std::max<size_t>(1, byl.size() / 20);
        double ts[8] = {0};
        for (size_t i = 0; i < top && i < byl.size(); ++i) for (int k = 0; k < 8; ++k) ts[k] += (double)h[byl[i].second * 8 + k];
        if (!byl.empty())
            fprintf(stderr, "[mf stamps] slowest %zu waves: chunks %.1f, prologue %.0f, wait+barrier %.0f, issue %.0f, products %.0f, epilogue %.0f, lifetime %.0f\n", top, ts[5] / top,
                    ts[0] / top, ts[1] / top, ts[2] / top, ts[3] / top, ts[7] / top, ts[4] / top);
        double lo = 0, hi = 0; int nlo = 0, nhi = 0;
        for (auto& pr : byl) { const unsigned long long* q = &h[pr.second * 8]; if (q[5] <= 6) { lo += (double)q[4]; ++nlo; } else if (q[5] >= 9) { hi += (double)q[4]; ++nhi; } }
        fprintf(stderr, "[mf stamps] lifetime of waves with <= 6 chunks: %.0f (%d waves); with >= 9 chunks: %.0f (%d waves)\n", nlo ? lo / nlo : 0.0, nlo, nhi ? hi / nhi : 0.0, nhi);
    }
    if (n)
        fprintf(stderr, "[mf stamps] %d waves, %.1f k-steps each; shader clocks per wave: prologue %.0f, wait+barrier %.0f (%.0f/step), issue %.0f (%.0f/step), "
                        "products %.0f (%.0f/step), epilogue %.0f, lifetime %.0f (max %.0f)\n", n, steps / n, sum[0] / n, sum[1] / n, sum[1] / steps,
                sum[2] / n, sum[2] / steps, sum[3] / n, sum[3] / steps, epi / n, sum[4] / n, life_max);
    return MMW_OK;
}
// MMW_HOST_BLOCKING on a host-only handle (developer aid): both blockings built on the host, their statistics on stderr
inline void report_host_blocking(HostBlocking& HB, const HostPattern& H, int K, const BlockingLimits& lim, const Switches& sw) {
    const double t0 = tnow();
    build_blocking(HB, K, H.l_indptr, H.l_indices, lim);
    build_sd_tables(HB, K, H.l_indptr, H.l_indices);
    fprintf(stderr, "[mmw] host blocking %.1f ms: usable %d half-tile %d blocks %d rows/block %.1f union/block %.1f reuse %.2f entries %lld (nnz %lld, +%.1f%% padding) sd2_rounds %d\n",
            (tnow() - t0) * 1e3, (int)HB.usable, (int)HB.fits_half_tile, HB.nb(), (double)K / std::max(1, HB.nb()),
            (double)HB.un_cols.size() / std::max(1, HB.nb()), HB.reuse, (long long)HB.nent, (long long)H.nnzL(),
            100.0 * ((double)HB.nent / (double)H.nnzL() - 1.0), HB.sd2_rounds);
    const double t1 = tnow();
    build_mfma_blocking(HB, K, H.l_indptr, H.l_indices, sw.mf_rows, sw.mf_union_cap);
    fprintf(stderr, "[mmw] matrix-core blocking %.1f ms: ok %d blocks %d rows/block %.1f reuse %.2f row tiles %d k-steps %d\n", (tnow() - t1) * 1e3,
            (int)HB.fits_mfma, HB.nbm(), (double)K / std::max(1, HB.nbm()), HB.m_reuse, HB.mfma_mt, HB.kbase.empty() ? 0 : HB.kbase.back());
    if (live_switch(LIVE_HOST_BLOCKING_HIST)) {  // k-steps of every block, in launch order
        for (int b = 0; b < HB.nbm(); ++b) fprintf(stderr, "%d:%d ", HB.m_desc[(size_t)b * 8 + 1], HB.kbase[b + 1] - HB.kbase[b]);
        fprintf(stderr, "\n");
    }
}
}  // namespace mmw
