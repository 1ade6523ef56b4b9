// What the solver handle hands out (solver.h): the device fields of mmw_read_f64 behind one fp64 staging buffer, and mmw_sketch.  Solver<T>
// answers the host-held fields itself and settles and synchronises the handle before it comes here; nothing here changes the iterate.
#pragma once
#include "solver_loop.h"
#include "solver_replay.h"

namespace {
template <typename T> struct SolverReads {
    using Core = SolverCore<T>;
    DevBuf<double> out64;  // max(nnzL, C, K Dpad): sized by init_common and set_slots
    int resize(const Core& co) { return out64.alloc(std::max(std::max((size_t)co.H.nnzL(), (size_t)co.H.C()), co.eng.bs)); }
    int export_T(Core& co, const T* src, size_t n, double* out, int64_t have) {
        if ((int64_t)n != have) return fail(MMW_ERR_ARG, "mmw_read_f64: wrong length " + std::to_string(have) + ", expected " + std::to_string(n));
        hipLaunchKernelGGL((k_to_f64<T>), dim3(grid_elems(n)), dim3(BLOCK), 0, co.st, n, src, out64.p);
        MMW_HIP(hipGetLastError());
        MMW_TRY(copy_d2h(out, out64.p, (size_t)n * sizeof(double), co.st));
        return MMW_OK;
    }
    int export_block(Core& co, const T* src, double* out, int64_t have) {
        const size_t n = (size_t)co.K * co.D;
        if ((int64_t)n != have) return fail(MMW_ERR_ARG, "mmw_read_f64: wrong length for a K x D block");
        hipLaunchKernelGGL((k_export_block<T>), dim3(grid_elems(n)), dim3(BLOCK), 0, co.st, co.K, co.D, co.eng.lay.Dpad, src, out64.p);
        MMW_HIP(hipGetLastError());
        MMW_TRY(copy_d2h(out, out64.p, (size_t)n * sizeof(double), co.st));
        return MMW_OK;
    }
    static int export_vals(std::initializer_list<double> v, double* out, int64_t have, const char* wrong_length) {  // a few numbers of fixed count
        if (have != (int64_t)v.size()) return fail(MMW_ERR_ARG, wrong_length);
        std::copy(v.begin(), v.end(), out);
        return MMW_OK;
    }
    // The Philox sketch of (seed, iteration) exactly as the loop draws it -- the generator is counter-based, so this is the block
    // iteration `iteration` of a device-RNG run with that seed multiplied, whatever chunk it ran in (parity tests give it to the oracle).
    int sketch(Core& co, uint64_t seed, int32_t iteration, double* out, int64_t n) {
        hipLaunchKernelGGL((k_sketch_rng<T>), dim3(grid_rows(co.K)), dim3(BLOCK), 0, co.st, co.K, co.D, co.eng.lay.Dpad, seed, (uint32_t)iteration, co.eng.Tm.p, (double*)nullptr);
        MMW_HIP(hipGetLastError());
        return export_block(co, co.eng.Tm.p, out, n);
    }
    int read_f64(Core& co, SolverLoop<T>& lp, const EmaxRecord& emax, Extras<T>& extras, int which, double* out, int64_t n) {
        const size_t nnz = (size_t)co.H.nnzL(), C = (size_t)co.H.C();
        switch (which) {
            case MMW_F_Y: return export_T(co, co.Y.p, C, out, n);
            case MMW_F_E_ACCU: return export_T(co, co.e_accu.p, C, out, n);
            case MMW_F_E_THIS: return export_T(co, co.e_this.p, C, out, n);
            case MMW_F_E_MAX: {
                if (n != 1) return fail(MMW_ERR_ARG, "the maximum violation is one number");
                if (emax.value_if_current(co.iter, &out[0])) return MMW_OK;  // reduced behind the last mmw_iterate's work and fetched by mmw_sync
                hipLaunchKernelGGL((k_max_of<T>), dim3(1), dim3(1024), 0, co.st, C, co.e_this.p, out64.p);
                MMW_HIP(hipGetLastError());
                return copy_d2h(out, out64.p, sizeof(double), co.st);
            }
            case MMW_F_LVAL: return export_T(co, co.lval.p, nnz, out, n);
            case MMW_F_XVAL: MMW_TRY(co.x.csr_view(co)); return export_T(co, co.xval.p, nnz, out, n);
            case MMW_F_XAVG: MMW_TRY(co.x.csr_view(co)); return export_T(co, co.xavg.p, nnz, out, n);
            case MMW_F_YAVG: return export_T(co, co.yavg.p, C, out, n);
            case MMW_F_XHALF: return export_block(co, co.Xh.p, out, n);
            case MMW_F_SKETCH: {
                if (!lp.carry.last_was_rng || co.iter == 0) return fail(MMW_ERR_STATE, "the sketch can be read back only after a device-generated iteration");
                hipLaunchKernelGGL((k_sketch_rng<T>), dim3(grid_rows(co.K)), dim3(BLOCK), 0, co.st, co.K, co.D, co.eng.lay.Dpad, lp.carry.last_seed, (uint32_t)(co.iter - 1), co.eng.Tm.p, (double*)nullptr);
                return export_block(co, co.eng.Tm.p, out, n);
            }
            case MMW_F_PHASE_US: return export_vec(co.pt.phase_us, out, n, "mmw_read_f64");
            case MMW_F_EXPM_INFO:
                return export_vals({co.eng.last.rho, (double)(co.eng.last.m_eff > 0 ? co.eng.last.m_eff : co.eng.last.m), (double)co.eng.last.nsub, co.eng.last.mu}, out, n, "expm info has 4 entries");
            case MMW_F_BLOCKING:
                return export_vals({co.eng.use_blk ? 1.0 : 0.0, (double)(co.bt.HB.usable ? co.bt.HB.nb() : 0), (double)co.bt.HB.reuse, (double)lp.pol.replays}, out, n, "blocking info has 4 entries");
            case MMW_F_SPMM_KIND:
                return export_vals({!co.eng.use_blk ? 0.0 : (co.eng.use_mfma ? 3.0 : (co.eng.blk.half_tile ? 2.0 : 1.0)), co.eng.use_mfma && co.eng.last_mfma_ok ? 1.0 : 0.0}, out, n, "spmm kind has 2 entries");
            case MMW_F_DUAL_INFO:
                return export_vals({(double)lp.n_rs_iters, (double)lp.n_fused_iters, (double)lp.n_first_iters, (double)lp.n_first16_iters}, out, n, "dual info has 4 entries");
            case MMW_F_GAP_INFO: return lp.gap.info(out, n);
            case MMW_F_FACTOR: return extras.read_factor(out, n);
            case MMW_F_FACTOR_ROWNORM: return extras.read_rownorm(out, n);
            case MMW_F_SPECTRAL_INFO: {
                if (n != 8) return fail(MMW_ERR_ARG, "spectral info has 8 entries");
                std::copy(extras.spec_info, extras.spec_info + 8, out);
                return MMW_OK;
            }
            case MMW_F_SPECTRAL_EIG: return export_vec(extras.spec_eig, out, n, "mmw_read_f64(SPECTRAL_EIG)");
            case MMW_F_KERNEL_US: {
                if (n != 2 * KT_NSLOT) return fail(MMW_ERR_ARG, "kernel timers have 2*9 entries");
                for (int i = 0; i < KT_NSLOT; ++i) { out[2 * i] = co.kt.total_us[i]; out[2 * i + 1] = co.kt.count[i]; }
                return MMW_OK;
            }
            default: return fail(MMW_ERR_ARG, "mmw_read_f64: unknown field");
        }
    }
};
}  // namespace
