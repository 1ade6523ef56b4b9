// mmw_bench_spmm (developer aid): the handle's SpMM kernels timed on its current L, outside the loop.  Solver<T>::bench_spmm has checked the
// arguments and settled the handle; the engine's switches this flips are put back before it returns.
#pragma once
#include "solver_loop.h"

namespace {
template <typename T> int solver_bench_spmm(SolverCore<T>& co, SolverLoop<T>& lp, int blocked, int reps, double* avg_us) {
    hipLaunchKernelGGL((k_sketch_rng<T>), dim3(grid_rows(co.K)), dim3(BLOCK), 0, co.st, co.K, co.D, co.eng.lay.Dpad, 99ull, 0u, co.eng.start_block(), (double*)nullptr);
    const bool keep = co.eng.use_blk, keep_mf = co.eng.use_mfma;
    co.eng.use_blk = blocked != 0;
    if (blocked == 2 && !co.eng.use_mfma) return fail(MMW_ERR_STATE, "no matrix-core SpMM for this handle (fp32, blocks of <= 32 rows)");
    co.eng.use_mfma = blocked == 2;
    StampBuf stamps;
    const bool want_stamps = blocked && live_switch(LIVE_STAMPS);
    MMW_TRY(stamps.request(want_stamps, (size_t)16 * 8192, co.st));
    hipEvent_t e0, e1;
    MMW_HIP(hipEventCreate(&e0));
    MMW_HIP(hipEventCreate(&e1));
    const bool lz = live_switch(LIVE_BENCH_LANCZOS);  // time the Lanczos epilogue (alpha partials) instead of the plain product
    const unsigned short* pl = nullptr;
    if (blocked == 2) {  // the planes are the producer's job: outside the timed launches
        co.eng.planes_ready[0] = false;
        MMW_TRY(co.eng.make_planes(0));
        pl = co.eng.planes_of(0);
    }
    // MMW_BENCH_FIRST: the first-order product as the loop launches it (fp16 operands and its whole epilogue; the operands are whatever the
    // last iteration left -- only the time is of interest)
    const bool fo = blocked == 2 && live_switch(LIVE_BENCH_FIRST) && sizeof(T) == 4 && lp.rsfx.p != nullptr;
    int ntr1 = 0;
    if (fo) {
        if (lp.xh_planes.n < 2 * co.eng.bs) MMW_TRY(lp.xh_planes.alloc(2 * co.eng.bs));
        const size_t need = (size_t)co.eng.first_grid_max();
        if (lp.tr1_part.n < need) {
            MMW_TRY(lp.tr1_part.alloc(need));
            MMW_HIP(hipMemsetAsync(lp.tr1_part.p, 0, need * sizeof(double), co.st));
        }
        hipLaunchKernelGGL(k_plane_f16, dim3(grid_elems(co.eng.bs / 4)), dim3(BLOCK), 0, co.st, co.eng.bs / 4, reinterpret_cast<const float4*>(co.eng.start_block()),
                           reinterpret_cast<uint2*>(co.eng.planes_of(0)));
    }
    auto one = [&]() {
        if (fo) {
            co.eng.planes_ready[0] = true;
            co.eng.planes0_f16 = true;
            return co.eng.apply_first((T*)nullptr, 0.5, 1, true, lp.xh_planes.p, lp.rsfx.p + co.K, lp.tr1_part.p, &ntr1);
        }
        return lz ? co.eng.template launch_spmm<SPMM_LANCZOS>(co.eng.start_block(), co.eng.Tm.p, nullptr, 0.5, 0.0, 1.0, nullptr, 0, pl)
                  : co.eng.template launch_spmm<SPMM_PLAIN>(co.eng.start_block(), co.eng.Tm.p, nullptr, 0.5, 0.0, 1.0, nullptr, 0, pl);
    };
    int rc = one();  // warm
    MMW_HIP(hipEventRecord(e0, co.st));
    for (int r = 0; r < reps && rc == MMW_OK; ++r) rc = one();
    MMW_HIP(hipEventRecord(e1, co.st));
    MMW_HIP(hipStreamSynchronize(co.st));
    if (want_stamps) {  // one more launch that leaves its stamps (matrix-core kernel: per-wave phase clocks)
        unsigned long long*& slot = blocked == 2 ? g_mf_stamps : g_blk_stamps;
        slot = stamps.p();
        rc = one();
        slot = nullptr;
        MMW_TRY(blocked == 2 ? dump_mf_stamps(co.st, stamps.p()) : dump_stamps(co.st, stamps.p()));
    }
    co.eng.use_blk = keep;
    co.eng.use_mfma = keep_mf;
    float ms = 0;
    MMW_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (avg_us) *avg_us = ms * 1e3 / (reps > 0 ? reps : 1);
    return rc;
}
}  // namespace
