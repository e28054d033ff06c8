// The linear system's learner loops around the solves, on the device: the roll-out step of the Q-learning example
// (rlmpc/examples/linear_system_mpc_qlearning.py:160-172; mpc4rl_amd/qlearning_linear.py) and of PPO (mpc4rl_amd/ppo.py), one lane per
// environment.
//   qlearning_linear_collect_kernel   after the policy's solve: the action (optionally explored), the environment step, row t of the
//                                     episode table, the observation and the cold mask of the next solve
//   PpoLinearEnv                      the plant of ppo_collect_kernel (ppo_kernel.hpp): the environment step, the truncation at
//                                     episode_length with the reset of those environments
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

// PPO's plant (ppo_collect_kernel<PpoLinearEnv>): the environment never terminates, an episode is truncated after episode_length steps
// and starts again from a fixed state (BatchedLinearSystemEnv.reset)
struct PpoLinearEnv {
    static constexpr int PAIRS = 1;
    LinearEnvPar par;
    int64_t episode_length;
    double reset0, reset1;
    __device__ __forceinline__ void step(const double2 *s, double action, double u01, double2 *nxt, double &reward, bool &terminated) const {
        const LinearStepOut o = linear_env_step(par, s[0].x, s[0].y, action, u01);
        nxt[0] = make_double2(o.s0, o.s1), reward = o.cost, terminated = false;
    }
    __device__ __forceinline__ bool ended(bool, int64_t n) const { return n >= episode_length; }
    __device__ __forceinline__ void reset(double, double2 *s) const { s[0] = make_double2(reset0, reset1); }
};

}  // namespace mpcrl
