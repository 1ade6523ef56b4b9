// The planning policy of the loop's chunks without readback (solver.h, Solver::iterate / settle): how long the next chunk may be, at
// what Lanczos order it is launched, whether it takes the first-order / one-half form, and the history of a run those guesses rest on.
// Host arithmetic only, no HIP call; the last plan read back (ExpmEngine::last), the switches, `iter` of the current run and max_order come in as arguments.
#pragma once
#include <algorithm>
#include <cmath>

#include "kernels_expm.h"
#include "kernels_mfma.h"
#include "switches.h"

namespace mmw {

struct ChunkPolicy {
    int age0 = 0;              // iterations L_accu had accumulated when this run started (a warm restart continues it): the matrix's norm and
                               // every estimate derived from it grow with age() = age0 + iter, not with the run's own counter
    int age(int iter) const { return age0 + iter; }
    double rho_prev = 0.0, rho_last = 0.0;
    int age_prev = -1, age_last = -1;
    bool warm_fresh = false;  // no chunk of this warm-started run has been settled yet: its first chunk is short and carries a spare step
    bool lagged_missed = false;  // an extrapolated plan of this run did not cover its matrix: the run's matrix outgrows the extrapolation, exact plans until the next reset
    bool plan_seen = false;  // the engine's last plan was read back in this run (settle)
    // the last chunk ran the shipped path to its end, was settled without a violation and nothing has touched the iterate since: the next
    // chunk's first iteration may continue on the lagged plan and the shifted softmax instead of restarting them exactly
    bool chain_ok = false;
    int replays = 0;
    int m_guess = 3;
    bool first_guess = false;  // the chunk being enqueued takes the first-order exponential (first_order_ok at its start)
    bool first_a16_guess = false;    // ... with the matrix as one fp16 half
    bool exact_plans_only = false;  // a cautious second attempt at a discarded chunk is running (settle)
    // mmw_reset.  Keeps: `replays` (the handle's lifetime count, MMW_F_BLOCKING[3]); rho_prev / rho_last (unread while age_prev /
    // age_last are -1); the three per-chunk guesses (set in front of every chunk that reads them).
    void on_reset() {
        age0 = 0; warm_fresh = false; age_prev = age_last = -1;
        chain_ok = false; plan_seen = false; lagged_missed = false; m_guess = 3;
    }
    // mmw_set_slots_warm after `iter` iterations.  Keeps, besides what on_reset keeps: plan_seen and m_guess -- the previous probe's last
    // plan is the best guess there is, and the run's first chunk launches one step more than it used (plan_chunk, warm_fresh).
    void on_warm_restart(int iter) {
        age0 += iter; warm_fresh = true; age_prev = age_last = -1;
        chain_ok = false; lagged_missed = false;
    }
    // a chunk was discarded (settle): its successor restarts plan and softmax exactly.  Keeps everything else: the history the discarded
    // chunk was planned on is still the run's.
    void on_discard() { chain_ok = false; }
    void note_plan(const ExpmPlan& p, int iter) {  // a plan has just been read back (settle): remember the bound and the age it belongs to
        if (age_last >= 0 && age(iter) > age_last) { rho_prev = rho_last; age_prev = age_last; }
        rho_last = p.rho; age_last = age(iter);
    }
    // Growth of the matrix's norm bound over the coming `ahead` iterations, as a ratio: at least linear in the age, and at least what
    // the last two plans read back in this run showed (after a warm restart with fewer slots the violations -- and with them the
    // increments of L -- are larger than the age suggests), with a factor 1.5 on that slope.
    double growth_ratio(int iter, int ahead) const {
        double r = (double)(age(iter) + ahead + 1) / (double)std::max(age(iter), 1);
        if (age_prev >= 0 && age_last > age_prev && rho_last > 0.0 && rho_last > rho_prev) {
            const double slope = (rho_last - rho_prev) / (double)(age_last - age_prev);
            r = std::max(r, (rho_last + 1.5 * slope * (double)(ahead + 1)) / rho_last);
        }
        return r;
    }
    // Steps to launch without reading the plan back: what the last application used, plus one spare step unless its
    // estimate met the tolerance with a factor 8 to spare (L grows by a fraction of itself per iteration; the plan is looked
    // at every 16 iterations; a batch that needs more anyway is replayed from its snapshot).
    // `ahead`: iterations the launch order has to hold for (the coming chunk).  The estimate after m steps grows like ||L||^(2m) and
    // ||L|| like the iteration count: no spare step only if the estimate, grown over the chunk, still meets the tolerance with a
    // factor 2 (and never without the factor 8 at the moment of the readback).
    // The coming chunk of `ahead` iterations may take the exponential as ONE product, y = u + (L/2 - mu I) u (ExpmEngine::apply_first):
    // the last plan read back holds the bound that form would have met (first_est, from k_lz_scalars or from the form's own check); it
    // grows like rho * q ~ t^2, and the same margins as for dropping the spare Lanczos step apply.
    // The certificate (kernels_mfma.h, first_verify) adds to that truncation bound what the fp16 operands lose: the plane of u at its
    // measured rounding (F16_PLANE_EXPECT predicts it) and the matrix image at c_A (one fp16 half: 2^-11; hi + lo: 2^-21), both times the
    // row-sum bound absn, which grows linearly.  a16: the chunk would read the matrix as one half.
    // `fp32`: the handle's dtype; `plane_rounding`: the rounding of the fp16 plane the certificate will charge (Solver::plane_rounding).
    bool first_order_ok(const ExpmPlan& p, const Switches& sw, int iter, int ahead, bool fp32, double plane_rounding, bool a16 = false) const {
        if (sw.no_first_order || !fp32 || !p.apost || p.m_eff != 1 || p.first_est == 0u) return false;
        const double est = plan_estimate(p.first_est);
        const double g1 = growth_ratio(iter, ahead), absn_g = p.absn * g1;
        if (!(absn_g < 0.03)) return false;  // the entries times 2^20 stay inside fp16's range
        if (a16 ? !((F16_PLANE_EXPECT + F16_UNIT) * absn_g <= p.tol) : !(F16_PLANE_EXPECT * absn_g <= p.tol)) return false;  // ExpmPlan::f16a_ok / f16_ok over the chunk
        // every iteration of the form is certified (a miss costs a replay of the chunk, nothing else): the truncation bound has to meet the
        // tolerance with a factor 4 now, and the whole predicted bound with a tenth to spare after the growth over the chunk
        const double rounding = std::exp(p.rho * g1) * (absn_g * (plane_rounding + (a16 ? F16_UNIT : F16_CA_TWO)) + F16_SUBNORMAL_ROW);
        return est <= p.tol / 4.0 && est * g1 * g1 + rounding <= 0.9 * p.tol;
    }
    int next_launch_order(const ExpmPlan& p, int max_order, int iter, int ahead = 0) const {
        if (p.m_eff <= 0) return std::min(max_order, p.m + 1);
        int spare = 1;
        if (p.apost && p.m_eff >= 1 && p.m_eff <= MAX_ORDER) {
            const double est = plan_estimate(p.conv[p.m_eff]);
            const double grow = std::pow(growth_ratio(iter, ahead), 2.0 * p.m_eff);
            if (est <= p.tol / 8.0 && est * grow <= p.tol / 2.0) spare = 0;
        }
        if (p.m_eff >= p.m_apriori) spare = 0;  // the a-priori order is never exceeded
        return std::min(max_order, p.m_eff + spare);
    }
    // How many more iterations one Lanczos step should stay accepted: its error estimate grows about quadratically with the norm of
    // L, which grows linearly with the iteration count, so est(t + c) ~ est(t) ((t + c) / t)^2 <= tol gives c <= t (sqrt(tol / est) - 1);
    // half of that.  0 unless the last plan read back stopped after one step.
    int room_iterations(const ExpmPlan& p, int iter) const {
        if (!p.apost || p.m_eff != 1) return 0;
        const double est = plan_estimate(p.conv[1]);
        if (!(est > 0.0)) return 32;
        double c = 0.5 * (double)age(iter) * (std::sqrt(p.tol / est) - 1.0);
        if (age_prev >= 0 && age_last > age_prev && rho_last > rho_prev && rho_last > 0.0)  // ... or with the slope the last two plans showed (growth_ratio)
            c = std::min(c, 0.5 * (std::sqrt(p.tol / est) - 1.0) * rho_last * (double)(age_last - age_prev) / (1.5 * (rho_last - rho_prev)));
        return c > 32.0 ? 32 : (c < 0.0 ? 0 : (int)c);
    }
    // the last plan read back accepted ONE Lanczos step with a factor 8 to spare (where the order is already rising -- the graphs
    // without locality -- a long chunk launched with too few stages is a long replay: measured 5 187 -> 2 686 it/s at er-5pct-2k)
    bool plan_has_room(const ExpmPlan& p) const { return p.apost && p.m_eff == 1 && plan_estimate(p.conv[1]) <= p.tol / 8.0; }
    // Lagged planning pays where one Lanczos step is accepted with room to spare (its extrapolated norm bound is ~1/t larger than
    // the exact one, which must not cost a second product: on graphs without locality a product is 10x the two kernels saved).
    bool lagged_ok(const ExpmPlan& p, const Switches& sw) const {
        if (sw.no_lagged_plan || lagged_missed || !p.apost || p.m_eff != 1) return false;
        return plan_estimate(p.conv[1]) <= p.tol / 2.0;
    }
    // Length of the next chunk, `left` iterations remaining.  Chunks are short while L still grows fast (its norm is proportional to the
    // iteration count): half as many iterations as have been done (4 ... 32); as many as have been done (8 ... 32) while one Lanczos
    // step is accepted with a factor 2 to spare.
    int chunk_length(const ExpmPlan& p, const Switches& sw, int iter, int left) const {
        // ... or as many as the last settled plan's estimate leaves room for (room_iterations)
        int cap = lagged_ok(p, sw) ? std::max(8, std::min(32, age(iter))) : std::max(4, std::min(32, age(iter) / 2));
        // (holding the chunk to the run's age until two plans have shown how fast the matrix grows would spare the hard probes of a
        // bisection one discarded chunk -- at slot counts near infeasibility the norm grew 16x over iterations 4..35, not the 9x of a
        // linear law -- but costs every run one more readback in its first 32 iterations: measured, not kept)
        if (chain_ok && age(iter) >= 4) cap = std::max(cap, std::min(32, room_iterations(p, iter)));
        if (warm_fresh) cap = 8;
        int chunk = std::min(left, cap);
        if (left - chunk == 1) ++chunk;  // no trailing chunk of one iteration: it would run synchronously and break the chain of chunks
        return chunk;
    }
    // The guesses a chunk of `chunk` iterations is enqueued with (`have_a16`: the handle holds the matrix's one-half fp16 image).
    void plan_chunk(const ExpmPlan& p, const Switches& sw, int max_order, int iter, int chunk, bool fp32, bool have_a16, double plane_rounding) {
        if (plan_seen) m_guess = next_launch_order(p, max_order, iter, chunk);  // before the first readback of a run: the default set by reset()
        first_guess = plan_seen && first_order_ok(p, sw, iter, chunk, fp32, plane_rounding);  // (requires that the last plan read back stopped after one step)
        if (first_guess) m_guess = 1;
        first_a16_guess = first_guess && !sw.no_first_a16 && have_a16 && first_order_ok(p, sw, iter, chunk, fp32, plane_rounding, true);
        if (warm_fresh) {  // the plan at hand belongs to the previous probe's slot count: one spare step, no first-order form
            m_guess = std::min(max_order, std::max(2, p.m_eff + 1));
            first_guess = false;
        }
    }
    // The cautious second attempt at a discarded chunk (settle, which also sets exact_plans_only around it): Lanczos steps at the a-priori order plus one.
    void plan_cautious(const ExpmPlan& p, int max_order) {
        first_guess = false;
        first_a16_guess = false;
        m_guess = std::min(max_order, std::max(std::max(p.m_apriori, p.m_eff), m_guess) + 1);
    }
};
}  // namespace mmw
