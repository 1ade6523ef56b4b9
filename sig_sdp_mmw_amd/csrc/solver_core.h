// What every part of the solver handle reads (solver.h): the device and its stream, the switches, the host pattern and its device copy,
// the iterate's buffers with the layout X is held in, the engine of the exponential, the locality blockings and the timers.  The parts
// (solver_loop.h, solver_replay.h, solver_read.h) take the core as an argument and hold their own state.
#pragma once
#include <cstring>
#include <memory>
#include <atomic>
#include <thread>

#include "block_tables.h"
#include "chunk_policy.h"
#include "dev_reports.h"
#include "env_device.h"
#include "kernels_gm.h"
#include "pattern_device.h"
#include "solver_extras.h"

using namespace mmw;

namespace {
template <typename T> struct SolverCore;
// Which buffers hold the iterate's X and its running sum: the CSR-ordered xval / xavg of the core, or -- while `tiles` is set -- xs_val /
// xs_avg in the matrix-core SDDMM's tile order (kernels_mfma.h; bt.b_e2w maps a CSR entry to its slot).  `live` is the pair the iterate is in.
//   reset: CSR order (the initial point is written there)   discard: the order the snapshot was taken in   warm restart: unchanged
template <typename T> struct XLayout {
    DevBuf<T> xs_val, xs_avg;
    bool tiles = false;
    struct Pair { DevBuf<T>* val; DevBuf<T>* avg; size_t n; };
    Pair live(SolverCore<T>& c) { return tiles ? Pair{&xs_val, &xs_avg, c.bt.n_xs} : Pair{&c.xval, &c.xavg, (size_t)c.H.nnzL()}; }
    // CSR-ordered copies of X and its running sum for whoever needs them (API reads, the factor, the gap, the kernels of the other SDDMM
    // forms) while the iterate keeps them in tile order; the tile buffers stay the iterate's
    int csr_view(SolverCore<T>& c) {
        if (!tiles) return MMW_OK;
        const size_t nnz = (size_t)c.H.nnzL();
        hipLaunchKernelGGL((k_x_tiles_to_csr<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, c.st, nnz, c.bt.b_e2w.p, xs_val.p, c.xval.p, xs_avg.p, c.xavg.p);
        MMW_HIP(hipGetLastError());
        return MMW_OK;
    }
    int to_csr(SolverCore<T>& c) {
        MMW_TRY(csr_view(c));
        tiles = false;
        return MMW_OK;
    }
    int to_tiles(SolverCore<T>& c) {
        if (tiles) return MMW_OK;
        if (!c.bt.b_e2w.p || c.bt.n_xs == 0) return fail(MMW_ERR_STATE, "internal: no tile order on this handle");
        const size_t nnz = (size_t)c.H.nnzL();
        hipLaunchKernelGGL((k_x_csr_to_tiles<T>), dim3(grid_elems(nnz)), dim3(BLOCK), 0, c.st, nnz, c.bt.b_e2w.p, c.xval.p, xs_val.p, c.xavg.p, xs_avg.p);
        MMW_HIP(hipGetLastError());
        tiles = true;
        return MMW_OK;
    }
};
template <typename T> struct SolverCore {
    const Switches sw;  // read once by mmw_create / mmw_create_from_env (switches.h); everything below this handle gets a reference
    explicit SolverCore(const Switches& s) : sw(s), eng(sw) {}
    int device = 0;
    bool host_only = false;
    hipStream_t st = nullptr;
    HostPattern H;
    int K = 0, Z = 0, D = 0, rank_radio = 2, nit = 0, iter = 0;
    double eta = 0.1;
    bool kt_shipped = false;  // set_profile(2)
    bool kt_exact() const { return kt.on && !kt_shipped; }  // set_profile(1): synchronous plans, every kernel class in launches of its own
    // pattern on the device
    DevBuf<int> d_indptr, d_col, d_pid, d_mirror, d_diag, d_apos, d_lrow;
    DevBuf<T> d_sab, d_sba, d_h, d_ssum, d_invn, d_cH;
    // iterate state
    DevBuf<T> lval, xval, xavg, Y, yavg, e_accu, e_this, Xh;
    XLayout<T> x;
    BlockTables<T> bt;  // the locality blockings: host tables, device tables, kernel argument structs (block_tables.h)
    bool lblk_stale = false;  // bt.lval_blk lags lval (the matrix-core kernel ran the last products)
    ExpmEngine<T> eng;
    KernelTimers kt;
    PhaseTimers pt;
    int upload_slot_scalars() {  // the two row vectors that follow the slot count: 1 / norm_H and cH
        std::vector<double> invn(K);
        for (int k = 0; k < K; ++k) invn[k] = 1.0 / H.norm_H[k];
        MMW_TRY(d_invn.upload_cast(invn, st));
        return d_cH.upload_cast(H.cH, st);
    }
    int upload_row_vectors() {  // the K-vectors both creators end their pattern upload with
        MMW_TRY(d_h.upload_cast(H.h_max, st));
        MMW_TRY(d_ssum.upload_cast(H.S_sum, st));
        return upload_slot_scalars();
    }
    PatternDev<T> pat() const {
        PatternDev<T> P;
        P.K = K; P.Z = Z; P.E_asso = (int)H.E_asso(); P.C = (int)H.C(); P.nnzL = (int)H.nnzL();
        P.indptr = d_indptr.p; P.col = d_col.p; P.pid = d_pid.p; P.mirror = d_mirror.p; P.diag_pos = d_diag.p;
        P.asso_pos = d_apos.p; P.sab = d_sab.p; P.sba = d_sba.p; P.h_max = d_h.p; P.S_sum = d_ssum.p;
        P.inv_norm_H = d_invn.p; P.cH = d_cH.p;
        if (x.tiles) { P.e2w = bt.b_e2w.p; P.xasso = bt.b_xasso.p; P.xdiag_base = (int)bt.HB.m_nedges; }
        return P;
    }
    BlkDev blkdev() const { return bt.blkdev(K, eng.lay.Dpad, sw.full_tile); }
    int alloc_iterate() {
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        MMW_TRY(lval.alloc(nnz)); MMW_TRY(xval.alloc(nnz)); MMW_TRY(xavg.alloc(nnz));
        MMW_TRY(Y.alloc(C)); MMW_TRY(yavg.alloc(C)); MMW_TRY(e_accu.alloc(C)); MMW_TRY(e_this.alloc(C));
        return MMW_OK;
    }
    // the reference's initial point (mmw.py:62-68): Y = 1/C, X = I, L = 0, sums zero
    int initial_point() {
        const size_t nnz = (size_t)H.nnzL(), C = (size_t)H.C();
        MMW_HIP(hipMemsetAsync(lval.p, 0, nnz * sizeof(T), st));
        if (bt.lval_blk.p) MMW_HIP(hipMemsetAsync(bt.lval_blk.p, 0, (size_t)bt.HB.nent * sizeof(T), st));
        if (bt.afrag.p) MMW_HIP(hipMemsetAsync(bt.afrag.p, 0, bt.afrag_n * sizeof(unsigned), st));
        if (bt.afrag16.p) MMW_HIP(hipMemsetAsync(bt.afrag16.p, 0, bt.afrag_n * sizeof(unsigned short), st));
        eng.last_mfma_ok = true;
        lblk_stale = false;
        x.tiles = false;  // the initial point is written in CSR order; the first matrix-core SDDMM call moves it
        MMW_HIP(hipMemsetAsync(xval.p, 0, nnz * sizeof(T), st));
        MMW_HIP(hipMemsetAsync(xavg.p, 0, nnz * sizeof(T), st));
        MMW_HIP(hipMemsetAsync(e_accu.p, 0, C * sizeof(T), st));
        MMW_HIP(hipMemsetAsync(e_this.p, 0, C * sizeof(T), st));
        hipLaunchKernelGGL((k_set_identity<T>), dim3(grid_elems(K)), dim3(BLOCK), 0, st, K, d_diag.p, xval.p, xavg.p);
        const T y0 = (T)(1.0 / (double)C);
        hipLaunchKernelGGL((k_fill<T>), dim3(grid_elems(C)), dim3(BLOCK), 0, st, C, Y.p, y0);
        hipLaunchKernelGGL((k_fill<T>), dim3(grid_elems(C)), dim3(BLOCK), 0, st, C, yavg.p, y0);
        MMW_HIP(hipGetLastError());
        pt.clear_samples();
        return MMW_OK;
    }
    // Warm start of the next probe of the binary search (opt-in; the reference restarts every probe from Y = 1/C, X = I,
    // mmw.py:62-68): the accumulated violations e_accu, the accumulated loss L_accu and the last X / Y are kept, the
    // running sums restart from that X / Y, the iteration counter from zero.
    int sums_from_current() {
        const typename XLayout<T>::Pair xl = x.live(*this);
        MMW_HIP(hipMemcpyAsync(xl.avg->p, xl.val->p, xl.n * sizeof(T), hipMemcpyDeviceToDevice, st));
        MMW_HIP(hipMemcpyAsync(yavg.p, Y.p, (size_t)H.C() * sizeof(T), hipMemcpyDeviceToDevice, st));
        pt.clear_samples();
        return MMW_OK;
    }
};
}  // namespace
