// The linear system's learner loops around the solves, on the device: the roll-out step of the Q-learning example
// (rlmpc/examples/linear_system_mpc_qlearning.py:160-172; mpc4rl_amd/qlearning_linear.py) and of PPO (mpc4rl_amd/ppo.py), one lane per
// environment.
//   qlearning_linear_collect_kernel   after the policy's solve: the action (optionally explored), the environment step, row t of the
//                                     episode table, the observation and the cold mask of the next solve
//   ppo_linear_collect_kernel         after the policy's solve: the sample and its log probability, the environment step, row t of the
//                                     roll-out tables, the truncation at episode_length with the reset of those environments
// The environment step is linear_env_step of env_kernel.hpp (the same bits as mpcrl_env_linear_step); PPO's mean and log probability are
// the device functions of ppo_kernel.hpp, shared with the surrogate.  The environment never terminates: there is no liveness in the
// Q-learning table, and PPO's TERM is all zero (an episode ends by truncation only, so GAE bootstraps through every end).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "env_kernel.hpp"
#include "ppo_kernel.hpp"

namespace mpcrl {

struct QlLinearCollectArgs {
    LinearEnvPar par;
    int E, T;
    double *state;            // [E][2] the environments' states
    const double *u0;         // [E] the policy's solve: control
    const int *status;        // [E]
    const float *eps;         // [T][E] standard-normal draws, row r read at step r
    const double *u01;        // [T][E] uniform draws (the environment's noise), row r read at step r
    double lo, hi;            // lbu, ubu
    float sigma;
    double *obs;              // [E][2] out: the observation of the next solve
    int32_t *row;             // [E] the table row this environment writes next (advanced by one per call)
    int32_t *cold;            // [E] out: 0 (the cold mask of the next solve; the caller sets it to 1 before an episode)
    double *S;                // [T][E][2] s_t
    double *A;                // [T][E]    the applied action (unscaled: this plant's example uses no action scaling)
    double *C;                // [T][E]    the cost of the step
};

__global__ void __launch_bounds__(256) qlearning_linear_collect_kernel(const QlLinearCollectArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.E) return;
    const int r = a.row[i];
    if (r < 0 || r >= a.T) return;          // the table is full: nothing is written, nothing is stepped
    const long k = (long)r * a.E + i;
    const double2 s = reinterpret_cast<const double2 *>(a.state)[i];
    const double u = a.u0[i];
    const int st = a.status[i];
    const bool good = (st == 0 || st == 2) && isfinite(u);
    double act = good ? u : 0.0;
    if (a.sigma > 0.0f) {
#pragma clang fp contract(off)      // clip(a + (double)(sigma eps), lo, hi): the float product is rounded, then the fp64 sum
        const float n = a.sigma * a.eps[k];
        act = act + (double)n;
        act = act < a.lo ? a.lo : (act > a.hi ? a.hi : act);
    }
    const LinearStepOut o = linear_env_step(a.par, s.x, s.y, act, a.u01[k]);
    reinterpret_cast<double2 *>(a.S)[k] = s;
    a.A[k] = act, a.C[k] = o.cost;
    reinterpret_cast<double2 *>(a.state)[i] = make_double2(o.s0, o.s1);
    reinterpret_cast<double2 *>(a.obs)[i] = make_double2(o.s0, o.s1);
    a.row[i] = r + 1;
    a.cold[i] = 0;
}

struct PpoLinearCollectArgs {
    LinearEnvPar par;
    int E, T, t;
    double *state;            // [E][2] the environments' states
    int64_t *steps;           // [E] steps since the last reset (the learner's: the environment keeps no count)
    const double *u0;         // [E] the policy's solve: control
    const int *status;        // [E]
    const float *eps;         // [E] standard-normal draws
    const double *u01;        // [E] uniform draws (the environment's noise)
    const double *value;      // [E] the critic at the observation just solved
    const double *log_std;    // [1]
    double lo, hi, reward_scale;
    int64_t episode_length;   // an episode is truncated after this many steps
    double reset0, reset1;    // the state an episode starts from
    double *OBS, *ACT, *LOGP, *VAL, *REW, *NEXT;      // [T][E] ([..][2] for OBS, NEXT)
    uint8_t *TERM, *DONE, *OK;                        // [T][E]
    double *obs;              // [E][2] out: the next solve's x0 (after resets)
    int32_t *ended;           // [E] out: 1 = the episode ended (the next solve starts that instance cold)
};

__global__ void __launch_bounds__(256) ppo_linear_collect_kernel(const PpoLinearCollectArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.E) return;
    const double ls = a.log_std[0], sigma = exp(ls);
    const double u = a.u0[i];
    const bool ok = ppo_solve_ok(a.status[i], u);
    const double mu = ppo_mean(u, ok, a.lo, a.hi);
    double act;
    {
#pragma clang fp contract(off)      // mu + sigma eps as the torch expression: product, sum
        act = sigma * (double)a.eps[i];
        act = mu + act;
    }
    const double logp = ppo_log_prob(act, mu, sigma, ls);
    const double2 s = reinterpret_cast<const double2 *>(a.state)[i];
    // the stored sample is unclipped; the environment sees clip(a, -1, 1) (a NaN sample — log_std not finite — steps with NaN, as in torch)
    const double applied = act < -1.0 ? -1.0 : (act > 1.0 ? 1.0 : act);
    const LinearStepOut o = linear_env_step(a.par, s.x, s.y, applied, a.u01[i]);
    const int64_t n = a.steps[i] + 1;
    const bool done = n >= a.episode_length;
    const long k = (long)a.t * a.E + i;
    reinterpret_cast<double2 *>(a.OBS)[k] = s;
    reinterpret_cast<double2 *>(a.NEXT)[k] = make_double2(o.s0, o.s1);       // before any reset: the bootstrap value is taken here
    a.ACT[k] = act, a.LOGP[k] = logp, a.VAL[k] = a.value[i], a.REW[k] = a.reward_scale * o.cost;
    a.TERM[k] = 0, a.DONE[k] = done ? 1 : 0, a.OK[k] = ok ? 1 : 0;
    // the environment goes on, or starts again (BatchedLinearSystemEnv.reset)
    const double2 nxt = done ? make_double2(a.reset0, a.reset1) : make_double2(o.s0, o.s1);
    reinterpret_cast<double2 *>(a.state)[i] = nxt;
    reinterpret_cast<double2 *>(a.obs)[i] = nxt;
    a.steps[i] = done ? 0 : n;
    a.ended[i] = done ? 1 : 0;
}

}  // namespace mpcrl
