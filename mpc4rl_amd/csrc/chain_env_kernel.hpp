// chain_env_kernel.hpp — the chain of masses as a plant, and the roll-out step of its Q-learning loop (mpc4rl_amd/envs.py
// BatchedChainMassEnv, mpc4rl_amd/qlearning_chain.py), one lane per environment, all arithmetic fp64.
//   env_chain_step_kernel           the plant: the reference's chain ODE (rlmpc/mpc/chain_mass/ocp_utils.py:76-130) integrated as the
//                                   model integrates it (rk_steps RK4 steps of Ts / rk_steps, ocp_utils.py:42-56,132) at the
//                                   environment's OWN parameter vector, plus a per-step disturbance on the free masses' accelerations
//   qlearning_chain_collect_kernel  after the policy's solve: the three controls (optionally explored), the environment step, row t of
//                                   the episode table, the observation and the cold mask of the next solve
// The ODE is ChainDev<NMASS>::ode_p<double> of models_dev.hpp as it stands — what the solve kernel linearises — with w_std * wn added to
// the 3 M acceleration entries of its result (the ODE is additive in w, so this is w + noise inside it).  Both kernels step through
// chain_env_step, one device function: the same expressions, the same bits.
// Every state and stage array is indexed at compile time (fully unrolled loops), so the arrays live in registers: a runtime index would
// send them to scratch.  The one runtime loop, over the columns of Q, reads its column's state entry from memory instead.  Blocks of 64:
// one wavefront, up to 512 VGPRs per lane.
// The cost is l(s, a) = 1/2 (s - x_ss)' Q (s - x_ss) + 1/2 a' R a of the state BEFORE the step with the environment's own Q and R (the
// quantity the MPC's Q(s, a) models); the cartpole and linear-system environments report the cost of the NEW state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "models_dev.hpp"

namespace mpcrl {

// the plant's arguments (mpcrl_env_chain_step)
struct ChainEnvPar {
    const double *p;          // the parameter vector(s) in the OCP's layout (m, D, L, C, Q, R, w)
    int64_t p_stride;         // 0: one vector for all environments; NP: one row per environment
    const double *x_ss;       // [NX] the cost's reference state
    const double *wn;         // [.][3 M] standard-normal draws (NULL: no disturbance)
    double h, w_std;          // the RK4 step Ts / rk_steps; the disturbance's standard deviation
    int rk_steps;
};

// The same pointer as a value the compiler knows nothing about.  Each ODE evaluation reads its parameters through one of these, so the
// 10 (NMASS - 1) per-lane parameter loads are not kept in registers across the eight evaluations of a step: held, they take 120 VGPRs at
// NMASS 7 on top of the four state-sized stage arrays and the kernel spills to scratch.
MPCRL_DI const double *chain_env_reread(const double *p) {
    asm volatile("" : "+v"(p));
    return p;
}

// One environment's step.  xs: the state in memory (read once more by the cost's column loop), x: the same state in registers on entry,
// the new state on return; a: the applied controls; wn: this environment's 3 M draws (NULL: none).  Returns l(s, a).
template <int NMASS>
MPCRL_DI double chain_env_step(const double *p, const double *x_ss, double h, int rk_steps, const double *wn, double w_std, const double *xs,
                               const double (&a)[3], double (&x)[ChainDev<NMASS>::NX]) {
    using Mdl = ChainDev<NMASS>;
    constexpr int NX = Mdl::NX, NA = 3 * Mdl::M, ACC = 3 * (Mdl::M + 1);
    // ---- the cost of (s, a): e' Q e column by column (Q column-major: Q(i, j) = Q[i + NX j]), then a' R a
    double cost;
    {
        double e[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) e[i] = x[i] - x_ss[i];
        const double *Q = p + Mdl::OFF_Q, *R = p + Mdl::OFF_R;
        double q = 0.0;
#pragma unroll 1      // one column at a time: unrolled, its NX * NX loads are issued ahead and take the register file
        for (int j = 0; j < NX; ++j) {
            double c = 0.0;
#pragma unroll
            for (int i = 0; i < NX; ++i) c += e[i] * Q[i + NX * j];
            q += c * (xs[j] - x_ss[j]);
        }
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) r += (a[0] * R[3 * j] + a[1] * R[1 + 3 * j] + a[2] * R[2 + 3 * j]) * a[j];
        cost = 0.5 * (q + r);
    }
    // ---- rk_steps RK4 steps of h on ode_p + the disturbance (disc_map_p's scheme)
    double nz[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) nz[i] = wn ? w_std * wn[i] : 0.0;
#pragma unroll 1
    for (int s = 0; s < rk_steps; ++s) {
        double acc[NX], kk[NX], xt[NX];
        Mdl::template ode_p<double>(x, a, chain_env_reread(p), kk);
#pragma unroll
        for (int i = 0; i < NA; ++i) kk[ACC + i] = kk[ACC + i] + nz[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) acc[i] = kk[i], xt[i] = x[i] + (0.5 * h) * kk[i];
        Mdl::template ode_p<double>(xt, a, chain_env_reread(p), kk);
#pragma unroll
        for (int i = 0; i < NA; ++i) kk[ACC + i] = kk[ACC + i] + nz[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) acc[i] = acc[i] + 2.0 * kk[i], xt[i] = x[i] + (0.5 * h) * kk[i];
        Mdl::template ode_p<double>(xt, a, chain_env_reread(p), kk);
#pragma unroll
        for (int i = 0; i < NA; ++i) kk[ACC + i] = kk[ACC + i] + nz[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) acc[i] = acc[i] + 2.0 * kk[i], xt[i] = x[i] + h * kk[i];
        Mdl::template ode_p<double>(xt, a, chain_env_reread(p), kk);
#pragma unroll
        for (int i = 0; i < NA; ++i) kk[ACC + i] = kk[ACC + i] + nz[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = x[i] + (h / 6.0) * (acc[i] + kk[i]);
    }
    return cost;
}

// obs_f32 != 0: obs is float, else double (the state itself stays fp64); obs may be NULL
template <int NMASS>
__global__ void __launch_bounds__(64) env_chain_step_kernel(const ChainEnvPar e, int B, double *state, const double *action, void *obs, int obs_f32,
                                                            double *cost) {
    constexpr int NX = ChainDev<NMASS>::NX, NA = 3 * ChainDev<NMASS>::M;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    double *xs = state + (long)i * NX;
    double x[NX];
#pragma unroll
    for (int k = 0; k < NX; ++k) x[k] = xs[k];
    const double a[3] = {action[3L * i], action[3L * i + 1], action[3L * i + 2]};
    const double c = chain_env_step<NMASS>(e.p + (long)i * e.p_stride, e.x_ss, e.h, e.rk_steps, e.wn ? e.wn + (long)i * NA : nullptr, e.w_std, xs, a, x);
#pragma unroll
    for (int k = 0; k < NX; ++k) xs[k] = x[k];
    if (obs) {
        if (obs_f32) {
#pragma unroll
            for (int k = 0; k < NX; ++k) reinterpret_cast<float *>(obs)[(long)i * NX + k] = (float)x[k];
        } else {
#pragma unroll
            for (int k = 0; k < NX; ++k) reinterpret_cast<double *>(obs)[(long)i * NX + k] = x[k];
        }
    }
    cost[i] = c;
}

struct QlChainCollectArgs {
    ChainEnvPar env;          // env.wn: [T][E][3 M], row r read at step r
    int E, T;
    double *state;            // [E][NX] the environments' states
    const double *u0;         // [E][3] the policy's solve: controls
    const int *status;        // [E]
    const float *eps;         // [T][E][3] standard-normal draws, row r read at step r
    double lo[3], hi[3];      // lbu, ubu
    float sigma;
    double *obs;              // [E][NX] out: the observation of the next solve
    int32_t *row;             // [E] the table row this environment writes next (advanced by one per call)
    int32_t *cold;            // [E] out: 0 (the cold mask of the next solve; the caller sets it to 1 before an episode)
    double *S;                // [T][E][NX] s_t
    double *A;                // [T][E][3]  the applied action
    double *C;                // [T][E]     l(s_t, a_t)
};

template <int NMASS>
__global__ void __launch_bounds__(64) qlearning_chain_collect_kernel(const QlChainCollectArgs a) {
    constexpr int NX = ChainDev<NMASS>::NX, NA = 3 * ChainDev<NMASS>::M;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.E) return;
    const int r = a.row[i];
    if (r < 0 || r >= a.T) return;          // the table is full: nothing is written, nothing is stepped
    const long k = (long)r * a.E + i;
    double *xs = a.state + (long)i * NX;
    double x[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xs[j];
    const double u[3] = {a.u0[3L * i], a.u0[3L * i + 1], a.u0[3L * i + 2]};
    const int st = a.status[i];
    const bool good = (st == 0 || st == 2) && isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
    double act[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        act[j] = good ? u[j] : 0.0;
        if (a.sigma > 0.0f) {
#pragma clang fp contract(off)      // clip(a + (double)(sigma eps), lo, hi): the float product is rounded, then the fp64 sum
            const float n = a.sigma * a.eps[3 * k + j];
            act[j] = act[j] + (double)n;
            act[j] = act[j] < a.lo[j] ? a.lo[j] : (act[j] > a.hi[j] ? a.hi[j] : act[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) a.S[k * NX + j] = x[j];
    const double c = chain_env_step<NMASS>(a.env.p + (long)i * a.env.p_stride, a.env.x_ss, a.env.h, a.env.rk_steps,
                                           a.env.wn ? a.env.wn + k * NA : nullptr, a.env.w_std, xs, act, x);
#pragma unroll
    for (int j = 0; j < 3; ++j) a.A[3 * k + j] = act[j];
    a.C[k] = c;
#pragma unroll
    for (int j = 0; j < NX; ++j) xs[j] = x[j], a.obs[(long)i * NX + j] = x[j];
    a.row[i] = r + 1;
    a.cold[i] = 0;
}

}  // namespace mpcrl
