// launch_plan.hpp — which kernel instantiation, in which grid, one mpcrl_solve of a small model (cartpole, linear system) launches:
// the whole decision as one pure host function of a handful of integers.  Nothing here needs HIP or a device (a host compiler
// builds this header on its own; tests/test_launch_plan_cpu.py sweeps it through mpcrl_debug_launch_plan).  mpcrl_api.hip feeds it
// the handle's fields (choose_shape) and maps the answer to a template instantiation (dispatch); mpcrl_query_time_sliced answers
// from the same plan, so what the caller is told and what is launched cannot differ.
#pragma once
#include <algorithm>

#include "../../include/mpcrl.h"

namespace mpcrl {

// What the plan needs to know of a model class (small_traits<M>() in small_kernel.hpp is the only place the classes are consulted):
// max_ipw = most instances a wavefront takes; park_words, park_cap = the time-sliced kernel's parked state (below); has_soft = soft
// bounds (slack state): no time-sliced kernel; seg_skip = the segmented reductions leave levels out at run time: no SHORT form;
// box_rows = cartpole: the BOX instantiations and the exact-QP one exist; lq = linear system: the kernels of linear_kernel.hpp exist.
struct SmallTraits {
    int nx, nu, max_ipw, park_words, park_cap;
    bool has_soft, seg_skip, box_rows, lq;
};

// The parked instance of the time-sliced kernel (small_solve_sliced_kernel): x, nu, u, lam, t of every stage.  It lives in LDS
// while (N + 1) * sliced_park_words fits sliced_park_cap — 21 stages for cartpole's dimensions, next to the stage slots of its
// matrix-core sweep — and in the instance's stored-iterate arrays in HBM beyond that.
constexpr int sliced_park_words(int nx, int nu) { return 2 * nx + nu + 4 * (nx + nu); }
constexpr int sliced_park_cap(int nx, int nu) { return (nx == 4 && nu == 1) ? 21 * sliced_park_words(nx, nu) : 64 * sliced_park_words(nx, nu); }
constexpr bool sliced_parks_in_lds(const SmallTraits &t, int N) { return (N + 1) * t.park_words <= t.park_cap; }

// The kernels of the small models exist in two forms of their segmented reductions (small_kernel.hpp, seg_reduce): SHORT for horizons
// whose instances take at most 32 lanes, where the tree has no level at distance 32, and the full tree for the longer ones.  A model
// whose reductions leave levels out at run time (seg_skip: the linear system) has the full form only.
constexpr bool seg_short(const SmallTraits &t, int N) { return !t.seg_skip && N + 1 <= 32; }
// Only the combinations a launch can reach are instantiated: the full tree means N + 1 >= 33 stages, and an instance of that many
// parks in LDS only if the cap has room for them (cartpole's 21 stages: no).
constexpr bool lds_park_reachable(const SmallTraits &t, bool is_short) { return is_short || 33 * t.park_words <= t.park_cap; }

// Time-sliced launch (small_solve_sliced_kernel): ipw + 1 instances per wavefront, ipw of them advancing per round.  Such a
// wavefront lives longer than (ipw + 1) / ipw plain lifetimes — measured on cartpole N = 20 at the end of round 2: 1.62 (818 k vs
// 1 328 k cycles: write-outs inside the loop, 3 % for mixing QPs of instances one SQP iteration apart, and more register spill traffic
// than the plain kernel) — so it pays only when it saves enough rounds of wavefronts on the chip's SIMDs: 4096 instances are 2 rounds
// of 3-instance wavefronts or 1 round of 4-instance ones (5.44 -> 6.36 M solves/s); 32768 are 11 vs 8 rounds (plain wins).
//
// That rule counts wavefronts, not work.  A time-sliced wavefront lasts for the SUM of its instances' iterations and, at one round,
// nothing evens the sums out between SIMDs; plain wavefronts last for the MAXIMUM over three neighbours of the packing order and the
// dispatcher hands the second round to whichever SIMD frees up first.  On batches of one difficulty the sliced launch wins (cartpole
// 4096 states of the benchmark box: 0.56 vs 0.60 ms); on replay samples along closed-loop swing-ups (SQP iterations 2..15) the plain
// one does (0.47 vs 0.65 ms, profiles/r03_replay_cold_solve.txt).  Which of the two a caller's batches are cannot be read off the
// flags, so in automatic mode a handle whose batch size passes the rule times the two shapes against each other on its own calls.
enum { TUNE_PERIOD = 64, TUNE_SLICED = 0, TUNE_PLAIN = 1 };

// one kind of call (cold or warm): last probe time of either shape (ms, -1 = none yet), calls so far (events: MpcrlSolver::Tuner)
struct TunerState {
    float ms[2] = {-1.f, -1.f};
    unsigned calls = 0;
};

// the shape the tuner currently prefers: plain only once both have been timed and the plain kernel was faster by more than 20 %.
// The margin is what whole steps asked for.  The probes time the solve kernel alone; around it the plain launch carries the
// packing-order kernel (16 us at 4096 instances) and, inside the TD3 loop's graphs, loses more than that: on the benchmark's early
// replay rows the plain kernel probes 13 % faster (0.54 vs 0.63 ms) and the closed-loop step is 2 % SLOWER with it (2.06 vs 2.02 ms);
// on later-training replay rows it probes 27 % faster and the whole solve call is 23 % faster (profiles/r03_replay_cold_solve.txt).
constexpr float TUNE_MARGIN = 0.80f;
inline int tuned_best(const TunerState &t) {
    return (t.ms[0] > 0.f && t.ms[1] > 0.f && t.ms[TUNE_PLAIN] < TUNE_MARGIN * t.ms[TUNE_SLICED]) ? TUNE_PLAIN : TUNE_SLICED;
}

// shape of call number `call` of a tuned handle: calls 1 and 2 of every TUNE_PERIOD are the timed probes (call 0 of a fresh handle
// pays module load and cold caches and is not timed)
inline int tuned_shape(const TunerState &t, bool *timed) {
    const unsigned ph = t.calls % TUNE_PERIOD;
    if (timed) *timed = ph == 1 || ph == 2;
    return ph == 1 ? TUNE_SLICED : (ph == 2 ? TUNE_PLAIN : tuned_best(t));
}

// PLAIN: small_solve_kernel<M, SHORT, BOX>; SLICED: small_solve_sliced_kernel<M, LDSPARK, WARM, SHORT, BOX>; LQ: lq_solve_kernel<lq_spl,
// lq_rl> (stages per lane, lanes of an instance's DPP row; runs the sensitivity pass itself); EXACT: small_solve_kernel<CartpoleDevExact>
// (test-only, MPCRL_EXACT_QP).  box: PLAIN and SLICED only; lds_park: SLICED only; grid, sens_grid: workgroups of one wavefront of the
// solve launch and of the small_sens_kernel<M, SHORT> launch behind it.
struct SmallPlan {
    enum Family { PLAIN, SLICED, LQ, EXACT } family;
    bool seg_short, box, lds_park, warm;
    int lq_spl, lq_rl;
    unsigned grid, sens_grid;   // sens_grid 0 = no separate sensitivity launch
    bool candidate, by_rule;    // a time-sliced launch is legal for these inputs; the wave-count rule favours it
};

// `shape` (TUNE_SLICED / TUNE_PLAIN: what the tuner says, choose_shape in mpcrl_api.hip) is consulted only in automatic mode
// (slice_mode == 0) for a candidate that passes the rule; candidate and by_rule do not depend on it.
inline SmallPlan plan_small(const SmallTraits &t, int N, long B, int n_simd, int flags, int slice_mode, bool box_rows, int linear_spl,
                            int shape) {
    const int lpi = N + 1, ipw = std::min(64 / lpi, t.max_ipw);
    const long blocks = (B + ipw - 1) / ipw;
    SmallPlan p = {};
    p.seg_short = seg_short(t, N), p.warm = !(flags & MPCRL_COLD), p.box = box_rows && t.box_rows;
    p.grid = (unsigned)blocks, p.sens_grid = (flags & (MPCRL_SENS_V | MPCRL_SENS_PI)) ? (unsigned)blocks : 0;
    if (t.box_rows && (flags & MPCRL_EXACT_QP)) {
        p.family = SmallPlan::EXACT, p.box = false;
        return p;
    }
    if (!t.has_soft) {
        const int ips = std::min(64 / lpi, t.max_ipw - 1), q = ips + 1;
        const long waves4 = (B + q - 1) / q, rounds3 = (blocks + n_simd - 1) / n_simd, rounds4 = (waves4 + n_simd - 1) / n_simd;
        p.candidate = ips >= 1 && 64 - ips * lpi >= 1 && !(flags & MPCRL_RTI);   // (a lane is left for the parked instance)
        p.by_rule = 162 * rounds4 <= 100 * rounds3;
        if (p.candidate && (slice_mode != 0 ? slice_mode > 0 : p.by_rule && shape == TUNE_SLICED)) {
            p.family = SmallPlan::SLICED, p.lds_park = sliced_parks_in_lds(t, N), p.grid = (unsigned)waves4;
            return p;
        }
    }
    if (t.lq) {
        // the linear-system model: several stages per lane, four (eight) instances per wavefront each in a DPP row (half row) of its own
        // (linear_kernel.hpp) unless switched off (MPCRL_LINEAR_SPL=1 at mpcrl_create: one stage per lane, small_solve_kernel) or the
        // horizon leaves it no advantage.  Three stages per lane while they fit a row (N <= 47); beyond that FOUR (N <= 63 = the longest
        // horizon mpcrl_create accepts: 16 lanes again).  Round 5 packed those horizons in segments of 17-22 lanes with __shfl
        // (lq_solve_kernel<3, 0>): 1.31-1.54 ms per 4096 solves at N = 48..63 against 0.99-1.20 of the one-stage kernels and 0.69-0.74 of
        // <4, 16> (profiles/r06_lq_long_horizons.txt) — gone.
        const int lpi3 = (N + 1 + 2) / 3, rl = lpi3 <= 8 ? 8 : 16, ipw3 = 64 / rl;   // lpi3 = lq_lanes_per_instance<3>(N)
        if (linear_spl != 1 && ipw3 > ipw && N + 1 <= 64) {
            p.family = SmallPlan::LQ, p.lq_spl = lpi3 > 16 ? 4 : 3, p.lq_rl = rl;
            p.grid = (unsigned)((B + ipw3 - 1) / ipw3), p.sens_grid = 0;
            return p;
        }
    }
    p.family = SmallPlan::PLAIN;
    return p;
}

}  // namespace mpcrl
