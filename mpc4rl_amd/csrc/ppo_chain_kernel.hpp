// ppo_chain_kernel.hpp — the roll-out step of PPO on the chain of masses (mpc4rl_amd/ppo.py), one lane per environment, all arithmetic
// fp64.  The policy is a diagonal Gaussian over the chain's three controls,
//     a ~ N(mu, diag(sigma^2)),   mu_j = 2 (u0*_j - lo_j) / (hi_j - lo_j) - 1,   sigma_j = exp(log_std_j)       (one log_std per control)
// and its log probability the sum over j = 0, 1, 2, in that order, of ppo_log_prob (ppo_kernel.hpp): the expressions of the one-control
// roll-out and of the surrogate, so a re-solve that returns the roll-out's u0 gives a ratio of exactly 1.
//   ppo_chain_collect_kernel<NMASS>  after the policy's solve: the sample and its log probability, row t of the roll-out tables, the
//                                    environment step, the truncation, the reset of the environments that ended, the observation and the
//                                    cold mask of the next solve
// The step is chain_env_step of chain_env_kernel.hpp as it stands — the bits of mpcrl_env_chain_step — on the PHYSICAL controls
// lo_j + 0.5 (clip(a_j, -1, 1) + 1) (hi_j - lo_j) (unscale_action: the plant takes no scaled action).  As there, every state and stage
// array is indexed at compile time and lives in registers, blocks are one wavefront, and the kernel uses no scratch at any chain size:
// what the lane can write before the step (the sample, its log probability, the observation's row) is written before it, so that only
// the state and the three applied controls are held across the step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chain_env_kernel.hpp"
#include "ppo_kernel.hpp"

namespace mpcrl {

struct PpoChainCollectArgs {
    ChainEnvPar env;          // env.wn: [E][3 M], this step's draws
    int E, T, t;
    double *state;            // [E][NX] the environments' states
    int64_t *steps;           // [E] steps since the last reset (the plant keeps no count)
    const double *u0;         // [E][3] the policy's solve: controls
    const int *status;        // [E]
    const float *eps;         // [E][3] standard-normal draws
    const double *value;      // [E] the critic at the observation just solved
    const double *log_std;    // [3]
    double lo[3], hi[3];      // lbu, ubu
    double reward_scale;
    int64_t episode_length;
    const double *x_reset;    // [NX] the state an episode starts from ...
    double vel_std;           // ... plus vel_std * rn on the 3 M velocity entries
    const double *rn;         // [E][3 M] standard-normal draws (NULL: vel_std == 0)
    double *OBS, *ACT, *LOGP, *VAL, *REW, *NEXT;      // [T][E] ([..][NX] for OBS, NEXT; [..][3] for ACT)
    uint8_t *TERM, *DONE, *OK;                        // [T][E]
    double *obs;              // [E][NX] out: the next solve's x0 (after resets)
    int32_t *ended;           // [E] out: 1 = the episode ended (the next solve starts that instance cold)
};

template <int NMASS>
__global__ void __launch_bounds__(64) ppo_chain_collect_kernel(const PpoChainCollectArgs a) {
    constexpr int NX = ChainDev<NMASS>::NX, NA = 3 * ChainDev<NMASS>::M;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.E) return;
    const long k = (long)a.t * a.E + i;
    double *xs = a.state + (long)i * NX;
    double x[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xs[j];
    // ---- the sample and its log probability (qlearning_chain_collect_kernel's `good`: all three controls are numbers)
    const double u[3] = {a.u0[3L * i], a.u0[3L * i + 1], a.u0[3L * i + 2]};
    const int st = a.status[i];
    const bool ok = (st == 0 || st == 2) && isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
    double applied[3], logp = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma clang fp contract(off)      // mu + sigma eps as the torch expression: product, sum; unscale_action the same way
        const double ls = a.log_std[j], sigma = exp(ls);
        const double mu = ppo_mean(u[j], ok, a.lo[j], a.hi[j]);
        double act = sigma * (double)a.eps[3L * i + j];
        act = mu + act;
        const double lp = ppo_log_prob(act, mu, sigma, ls);
        logp = j == 0 ? lp : logp + lp;
        a.ACT[3 * k + j] = act;      // the stored sample is unclipped; the plant sees the clip to [-1, 1], in physical units
        const double c = act < -1.0 ? -1.0 : (act > 1.0 ? 1.0 : act);
        applied[j] = a.lo[j] + 0.5 * (c + 1.0) * (a.hi[j] - a.lo[j]);
    }
    // ---- row t of the tables: what is known before the step
#pragma unroll
    for (int j = 0; j < NX; ++j) a.OBS[k * NX + j] = x[j];
    a.LOGP[k] = logp, a.VAL[k] = a.value[i], a.TERM[k] = 0, a.OK[k] = ok ? 1 : 0;
    // ---- the step
    const double cost = chain_env_step<NMASS>(a.env.p + (long)i * a.env.p_stride, a.env.x_ss, a.env.h, a.env.rk_steps,
                                              a.env.wn ? a.env.wn + (long)i * NA : nullptr, a.env.w_std, xs, applied, x);
    a.REW[k] = a.reward_scale * cost;
#pragma unroll
    for (int j = 0; j < NX; ++j) a.NEXT[k * NX + j] = x[j];      // before any reset: the bootstrap value is taken here
    // ---- the truncation (the plant never terminates) and the reset: x_reset, + vel_std rn on the velocities (BatchedChainMassEnv._fresh)
    const int64_t n = a.steps[i] + 1;
    const bool done = n >= a.episode_length;
    a.DONE[k] = done ? 1 : 0;
    if (done) {
#pragma unroll
        for (int j = 0; j < NX - NA; ++j) x[j] = a.x_reset[j];
#pragma unroll
        for (int j = 0; j < NA; ++j) {
#pragma clang fp contract(off)
            const double r = a.rn ? a.vel_std * a.rn[(long)i * NA + j] : 0.0;
            x[NX - NA + j] = a.rn ? a.x_reset[NX - NA + j] + r : a.x_reset[NX - NA + j];
        }
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) xs[j] = x[j], a.obs[(long)i * NX + j] = x[j];
    a.steps[i] = done ? 0 : n;
    a.ended[i] = done ? 1 : 0;
}

}  // namespace mpcrl
