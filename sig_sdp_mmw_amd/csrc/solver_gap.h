// The logged duality gap of a solver handle (mmw_set_gap / mmw_read_gap; kernels_gap.h): what the loop (solver_loop.h) enqueues per
// iteration while the gap is on, the ring of row slots, and the host's log.
//   enqueue   a row goes out through the first scheduled check at or after the largest |steps| this run has read back (before any:
//             first_steps, by default the cap), into slot i of the ring for the i-th row in flight; a row without a slot goes through
//             the cap in a spare slot, so it never needs continuing
//   collect   where the loop synchronises anyway -- settle(), or after each iteration of the path that reads its plans back -- the
//             slots' states are looked at (their copy rode behind the chunk); a row not done is continued from its slot, in rounds
//             that double its steps, until it is done or capped
//   discard   the rows in flight are forgotten: the replay enqueues them again
//   restart   (reset, set_slots, warm): the log is cleared, the setting and the buffers stay
#pragma once
#include <cmath>
#include <limits>

#include "kernels_gap.h"
#include "pattern.h"
#include "runtime.h"

namespace mmw {

constexpr int GAPH_RING_MAX = 33;
constexpr int GAPH_ROWS_IN_FLIGHT = 64;  // records of rows not yet read back (a chunk has at most 33 iterations)
constexpr size_t GAPH_RING_BYTES = (size_t)1 << 30;  // the ring's byte limit (MMW_F_GAP_INFO reports what was taken)

// where a row of (K, m_cap) is checked: 10, 20, ... with the interval growing by a quarter, last at min(K, m_cap)
inline std::vector<int> gap_check_list(int K, int m_cap) {
    const int mmax = std::min(K, m_cap);
    std::vector<int> c;
    int next = std::min(mmax, 10);
    for (;;) {
        c.push_back(next);
        if (next >= mmax) break;
        next = std::min(mmax, next + std::max(next / 4, 10));
    }
    return c;
}

template <typename T> struct GapPhase {
    bool on = false, ever = false;
    int m_cap = GAP_DEFAULT_M, first_steps = 0;
    int K = 0, slabs = 0, lpr = 8, nslots = 0;
    size_t nnz = 0, slot_doubles = 0, bytes = 0;
    DevBuf<double> ring, shared;
    DevBuf<GapState> states;
    DevBuf<double> c_sab, c_sba, c_h, c_ssum, c_invn, c_cH;  // fp32 handles: the pattern's constants in float64 (GapConsts)
    bool consts_stale = true;                                // 1 / norm_H and cH follow the slot count: uploaded again after a restart
    bool sab_widened = false;                                // the handle was built on the device: its gains exist as floats only
    DevBuf<double> records;  // 5 doubles per row in flight (GapRowDev::out)
    PinnedBuf pin;
    std::vector<double> log;  // 4 per announced iteration
    std::vector<int> checks;
    struct Pending { int iter, slot, rec, enq; bool continued; };
    std::vector<Pending> pend;
    bool copy_queued = false;
    int known_steps = 0;
    long long n_rows = 0, n_cont = 0, n_capped = 0, n_launch = 0;
    int max_steps = 0;

    static size_t a32d(size_t n) { return (n + 31) & ~(size_t)31; }
    void clear_log(int nit) {
        log.assign((size_t)4 * nit, std::numeric_limits<double>::quiet_NaN());
        for (int i = 0; i < nit; ++i) log[(size_t)4 * i + 3] = 0.0;
        pend.clear();
        copy_queued = false;
        known_steps = 0;
        consts_stale = true;
    }
    int configure(int enabled, int32_t cap, int32_t first, int K_, size_t nnz_, int nit) {
        if (cap > GAP_MAX_M) return fail(MMW_ERR_ARG, "mmw_set_gap: m_cap = " + std::to_string(cap) + " exceeds " + std::to_string(GAP_MAX_M) + ", the tridiagonal a check holds in LDS");
        m_cap = cap <= 0 ? GAP_DEFAULT_M : cap;
        first_steps = first <= 0 ? 0 : first;
        on = enabled != 0;
        K = K_; nnz = nnz_;
        checks = gap_check_list(K, m_cap);
        if (!ever) clear_log(nit);
        ever = true;
        if (!on || ring.p) return MMW_OK;
        // lanes per row from the mean row length: 8 as in the batch, up to a wave for long rows
        const double mean = (double)nnz / (double)std::max(K, 1);
        lpr = mean <= 16.0 ? 8 : mean <= 48.0 ? 16 : mean <= 96.0 ? 32 : 64;
        const int ng = BLOCK / lpr;
        slabs = std::max(1, std::min((K + ng - 1) / ng, GAPH_MAX_SLABS));
        slot_doubles = a32d(nnz) + 4 * a32d((size_t)K) + 2 * a32d(GAP_MAX_M) + 2 * a32d(GAPH_MAX_SLABS);
        const size_t shared_doubles = 2 * a32d((size_t)K) + 32 + a32d(2 * (size_t)GAPH_MAX_SLABS + 1);
        const size_t per = slot_doubles * sizeof(double);
        nslots = (int)std::min<size_t>(GAPH_RING_MAX, GAPH_RING_BYTES / per > 0 ? GAPH_RING_BYTES / per - 1 : 0);  // (one more is the spare)
        MMW_TRY(ring.alloc(slot_doubles * (size_t)(nslots + 1)));
        MMW_TRY(shared.alloc(shared_doubles));
        MMW_TRY(states.alloc((size_t)nslots + 1));
        MMW_TRY(records.alloc((size_t)5 * GAPH_ROWS_IN_FLIGHT));
        MMW_TRY(pin.ensure((size_t)5 * GAPH_ROWS_IN_FLIGHT * sizeof(double)));
        bytes = (slot_doubles * (size_t)(nslots + 1) + shared_doubles + (size_t)5 * GAPH_ROWS_IN_FLIGHT) * sizeof(double) + ((size_t)nslots + 1) * sizeof(GapState);
        return MMW_OK;
    }
    GapRowDev row_dev(int slot, int rec) const {
        double* b = ring.p + slot_doubles * (size_t)slot;
        GapRowDev R;
        R.gl = b; b += a32d(nnz);
        R.u = b; b += a32d((size_t)K);
        R.w = b; b += a32d((size_t)K);
        R.v[0] = b; b += a32d((size_t)K);
        R.v[1] = b; b += a32d((size_t)K);
        R.ta = b; b += a32d(GAP_MAX_M);
        R.tb = b; b += a32d(GAP_MAX_M);
        R.apart = b; b += a32d(GAPH_MAX_SLABS);
        R.bpart = b;
        R.st = states.p + slot;
        R.out = records.p + (size_t)5 * rec;
        return R;
    }
    GapBuildDev build_dev() const {
        GapBuildDev B;
        B.wrs = shared.p;
        B.wwH = B.wrs + a32d((size_t)K);
        B.ysc = B.wwH + a32d((size_t)K);
        B.mpart = B.ysc + 32;
        return B;
    }
    // An fp64 handle's pattern arrays are the constants.  An fp32 handle gets the host pattern's doubles; the gains of a handle built on
    // the device (no host copy of sab / sba) are its floats widened: there e_max and L(Ybar) carry the gains' fp32 rounding.
    int consts(hipStream_t st, const HostPattern& H, const PatternDev<T>& P, GapConsts& Cn) {
        if constexpr (sizeof(T) == 8) {
            Cn = GapConsts{P.sab, P.sba, P.h_max, P.S_sum, P.inv_norm_H, P.cH};
            return MMW_OK;
        } else {
            if (consts_stale) {
                std::vector<double> invn((size_t)K);
                for (int k = 0; k < K; ++k) invn[k] = 1.0 / H.norm_H[k];
                MMW_TRY(c_invn.upload(invn, st));
                MMW_TRY(c_cH.upload(H.cH, st));
                if (!c_h.p) {
                    MMW_TRY(c_h.upload(H.h_max, st));
                    MMW_TRY(c_ssum.upload(H.S_sum, st));
                    sab_widened = H.sab.size() != nnz || H.sba.size() != nnz;
                    if (!sab_widened) {
                        MMW_TRY(c_sab.upload(H.sab, st));
                        MMW_TRY(c_sba.upload(H.sba, st));
                    } else {
                        MMW_TRY(c_sab.alloc(nnz));
                        MMW_TRY(c_sba.alloc(nnz));
                        hipLaunchKernelGGL((k_gap_widen<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, st, nnz, P.sab, P.sba, c_sab.p, c_sba.p);
                        MMW_HIP(hipGetLastError());
                    }
                }
                consts_stale = false;
            }
            Cn = GapConsts{c_sab.p, c_sba.p, c_h.p, c_ssum.p, c_invn.p, c_cH.p};
            return MMW_OK;
        }
    }
    int first_check_at_or_after(int m) const {
        for (int c : checks)
            if (c >= m) return c;
        return checks.back();
    }
    // steps (from, to] of the row in `slot`, with the checks scheduled among them
    int enqueue_steps(hipStream_t st, const int* indptr, const int* col, int slot, int rec, int from, int to) {
        const GapRowDev R = row_dev(slot, rec);
        const GapBuildDev B = build_dev();
        const int mmax = checks.back();
        size_t ci = 0;
        while (ci < checks.size() && checks[ci] <= from) ++ci;
        for (int j = from + 1; j <= to; ++j) {
            hipLaunchKernelGGL(k_gap_mv, dim3(slabs), dim3(BLOCK), 0, st, indptr, col, K, j, lpr, R, B);
            hipLaunchKernelGGL(k_gap_up, dim3(slabs), dim3(BLOCK), 0, st, K, j, R);
            n_launch += 2;
            if (ci < checks.size() && checks[ci] == j) {
                hipLaunchKernelGGL(k_gap_check, dim3(1), dim3(GAPH_CHECK_THREADS), 0, st, K, j, mmax, slabs, R);
                ++n_launch;
                ++ci;
            }
        }
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    // the row of iteration `iter`, which is about to start: n = iter + 1 terms lie in xavg (+ xdef, the X still deferred to the next
    // LOSS pass) and yavg.  P says which order X is in.
    int enqueue_row(hipStream_t st, const HostPattern& H, const PatternDev<T>& P, const int* lrow, const T* xavg, const T* xdef, const T* yavg, int iter) {
        if (!on) return MMW_OK;
        if ((int)pend.size() >= GAPH_ROWS_IN_FLIGHT) return fail(MMW_ERR_STATE, "internal: more gap rows in flight than a chunk has iterations");
        const int rec = (int)pend.size();
        const bool has_slot = (int)pend.size() < nslots;
        const int slot = has_slot ? (int)pend.size() : nslots;
        const int guess = known_steps > 0 ? known_steps : (first_steps > 0 ? first_steps : checks.back());
        const int to = has_slot ? first_check_at_or_after(guess) : checks.back();
        if (to >= checks.back()) ++n_capped;  // (no slot, or nothing read back yet and no first_steps: such a row is never continued)
        const GapRowDev R = row_dev(slot, rec);
        const GapBuildDev B = build_dev();
        const double nterm = (double)(iter + 1);
        GapConsts Cn;
        MMW_TRY(consts(st, H, P, Cn));
        hipLaunchKernelGGL((k_gap_build_a<T>), dim3(slabs + 1), dim3(BLOCK), 0, st, P, xavg, xdef, yavg, nterm, Cn, B, R, slabs);
        const int ne = (int)std::min<size_t>((nnz + BLOCK - 1) / BLOCK, 2048);
        hipLaunchKernelGGL((k_gap_build_b<T>), dim3(slabs + std::max(ne, 1)), dim3(BLOCK), 0, st, P, lrow, yavg, nterm, Cn, B, R, slabs);
        n_launch += 2;
        MMW_TRY(enqueue_steps(st, P.indptr, P.col, slot, rec, 0, to));
        pend.push_back(Pending{iter, slot, rec, to, false});
        copy_queued = false;
        return MMW_OK;
    }
    // the states' copy rides behind the call's last launch: the synchronisation that settles the chunk brings it along
    int queue_copy(hipStream_t st) {
        if (pend.empty() || copy_queued) return MMW_OK;
        MMW_HIP(hipMemcpyAsync(pin.p, records.p, (size_t)5 * pend.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        copy_queued = true;
        return MMW_OK;
    }
    void drop_pending() { pend.clear(); copy_queued = false; }
    int collect(hipStream_t st, const int* indptr, const int* col) {
        if (pend.empty()) return MMW_OK;
        MMW_TRY(queue_copy(st));
        if (hipStreamQuery(st) != hipSuccess) {  // (after settle's own synchronisation the stream is idle)
            (void)hipGetLastError();
            MMW_HIP(hipStreamSynchronize(st));
        }
        for (;;) {
            const double* hr = static_cast<const double*>(pin.p);
            bool open = false;
            for (Pending& p : pend) {
                if (p.iter < 0) continue;
                const double* r = hr + (size_t)5 * p.rec;
                if (r[4] != 0.0) {
                    if ((size_t)4 * p.iter + 3 < log.size()) std::copy(r, r + 4, log.begin() + (size_t)4 * p.iter);
                    const int as = std::abs((int)r[3]);
                    known_steps = std::max(known_steps, as);
                    max_steps = std::max(max_steps, as);
                    ++n_rows;
                    p.iter = -1;
                    continue;
                }
                if (p.enq >= checks.back()) return fail(MMW_ERR_STATE, "internal: a gap row enqueued through the cap is not done");
                const int to = first_check_at_or_after(std::max(2 * p.enq, known_steps));
                MMW_TRY(enqueue_steps(st, indptr, col, p.slot, p.rec, p.enq, to));
                p.enq = to;
                if (!p.continued) ++n_cont;
                p.continued = true;
                open = true;
            }
            if (!open) break;
            copy_queued = false;
            MMW_TRY(queue_copy(st));
            MMW_HIP(hipStreamSynchronize(st));
        }
        drop_pending();
        return MMW_OK;
    }
    int read(int iters_done, double* out, int64_t n) const {
        if (!ever) return fail(MMW_ERR_STATE, "mmw_read_gap: the gap was never enabled on this handle (mmw_set_gap)");
        if (n != (int64_t)4 * iters_done) return fail(MMW_ERR_ARG, "mmw_read_gap: wrong length " + std::to_string(n) + ", expected 4 x " + std::to_string(iters_done) + " iterations done");
        if (n) std::copy(log.begin(), log.begin() + n, out);
        return MMW_OK;
    }
    int info(double* out, int64_t n) const {
        if (n != 6) return fail(MMW_ERR_ARG, "gap info has 6 entries");
        const double v[6] = {(double)n_rows, (double)n_cont, (double)n_capped, (double)n_launch, (double)max_steps, (double)bytes};
        std::copy(v, v + 6, out);
        return MMW_OK;
    }
};

}  // namespace mmw
