// Batched Q-learning of the cartpole MPC (round 7): the episode loop of scripts/cartpole_mpc_qlearning.py:200-263 around the solves, on
// the device (mpc4rl_amd/qlearning_cartpole.py).
//   qlearning_cartpole_collect_kernel  one roll-out step after the policy's solve, one lane per environment: the policy action with the
//                                      exploration of perturb_action (script lines 104-107), the environment step, row t of the episode
//                                      table and the liveness of the environment (the reference's `while not done`)
//   qlearning_td_grad_kernel           the TD errors of the learning sweep (script lines 255-257) and the message [sum lr td dQ/dp,
//                                      sum lr td, count] of their mean, summed in a fixed order (no floating-point atomics)
//   qlearning_apply_kernel             theta += message / max(1, count) on the learnable entries, after the collective
// The arithmetic of the action and of the environment step is the shared device functions of env_kernel.hpp (the same bits as
// mpcrl_policy_action + mpcrl_env_cartpole_step).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "env_kernel.hpp"
#include "batch_sum.hpp"

namespace mpcrl {

struct QlCollectArgs {
    CartpoleEnvPar par;
    int E, T;
    double *state;            // [E][4] the environments' states (fp64)
    int64_t *steps;           // [E]
    const double *u0;         // [E] the policy's solve: control
    const int *status;        // [E]
    const float *eps;         // [T][E] standard-normal draws, row t read at step t
    double lo, hi;            // lbu, ubu
    float sigma;
    double *obs;              // [E][4] or nullptr: out: the observation of the next solve
    uint8_t *alive;           // [E] in / out
    int32_t *row;             // [E] the table row this environment writes next (advanced by one per call)
    int32_t *cold;            // [E] or nullptr: out: 0 (the cold mask of the next solve; the caller sets it to 1 before an episode)
    double *S;                // [T][E][4] s_t
    double *A;                // [T][E]    the unscaled applied action
    double *C;                // [T][E]    the cost, x^2 + theta^2 of the new state
    uint8_t *live;            // [T][E]    1 = the row is a sample of the episode
};

__global__ void __launch_bounds__(256) qlearning_cartpole_collect_kernel(const QlCollectArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.E) return;
    const int r = a.row[i];
    if (r < 0 || r >= a.T) return;          // the table is full: nothing is written, nothing is stepped
    const double2 s01 = reinterpret_cast<const double2 *>(a.state)[2 * i], s23 = reinterpret_cast<const double2 *>(a.state)[2 * i + 1];
    double nx = s01.x, nxd = s01.y, nth = s23.x, nthd = s23.y, act = 0.0, cost = 0.0;
    const bool al = a.alive[i] != 0;
    if (al) {
        const int st = a.status[i];
        const double u = a.u0[i];
        const bool good = (st == 0 || st == 2) && isfinite(u);
        // scale_action, then clip(a + sigma eps, -1, 1) in float (mpcrl_policy_action with noise_clip = 0)
        const float f = policy_action_one(u, good, a.lo, a.hi, 1, a.eps + (long)r * a.E + i, a.sigma, 0.0f);
        const CartpoleStepOut o = cartpole_env_step(a.par, s01.x, s01.y, s23.x, s23.y, (double)f);
        const int64_t n = a.steps[i] + 1;
        const bool done = o.terminated || n >= a.par.max_episode_steps;
        {
#pragma clang fp contract(off)      // unscale_action as the torch / numpy expression: 0.5 (hi - lo) (a + 1) + lo, three roundings
            const double half = 0.5 * (a.hi - a.lo);
            act = half * ((double)f + 1.0) + a.lo;
        }
        cost = o.reward;
        nx = o.nx, nxd = o.nxd, nth = o.nth, nthd = o.nthd;
        reinterpret_cast<double2 *>(a.state)[2 * i] = make_double2(nx, nxd);
        reinterpret_cast<double2 *>(a.state)[2 * i + 1] = make_double2(nth, nthd);
        a.steps[i] = n;
        a.alive[i] = done ? 0 : 1;
    }
    // row r: s_t, and for an environment that has ended its (frozen) final state, action 0, cost 0, live 0
    const long k = (long)r * a.E + i;
    reinterpret_cast<double2 *>(a.S)[2 * k] = s01;
    reinterpret_cast<double2 *>(a.S)[2 * k + 1] = s23;
    a.A[k] = act, a.C[k] = cost, a.live[k] = al ? 1 : 0;
    if (a.obs) {
        reinterpret_cast<double2 *>(a.obs)[2 * i] = make_double2(nx, nxd);
        reinterpret_cast<double2 *>(a.obs)[2 * i + 1] = make_double2(nth, nthd);
    }
    a.row[i] = r + 1;
    if (a.cold) a.cold[i] = 0;
}

// The TD step of one episode.  Terms j = i E + e, i < T - 2 (sample rows i and i + 1 of environment e):
//     valid_j = live[i][e] && live[i+1][e] && live[i+2][e] && the Q and V solves of rows i and i + 1 returned status 0
// (live is a prefix per environment — what the collect kernel writes — so live[i+2] is i + 1 < L_e - 1: the reference's size - 1 samples
// and td[:-1] per environment);
//     td_j = (cost_j + gamma V_{j+E}) - Q_j;  w_j = valid_j ? lr td_j : 0  (selected: Q / V of a failed solve may be NaN)
//     msg = [sum_j w_j dQ/dp_j (n_p), sum_j w_j, sum_j valid_j]   (dQ/dp read as nan_to_num does; 0 x finite = 0)
// The sum is the fixed-order batch sum of batch_sum.hpp over blocks of TD_ROWS terms: the same inputs give the same bits.
constexpr int TD_ROWS = 128, TD_PMAX = 256;     // (TD_ROWS = the block size: one term per lane in the first phase)

struct QlTdArgs {
    const double *Q, *V;          // [T-1][E]
    const double *dQ;             // [T-1][E][n_p]
    const int *sq, *sv;           // [T-1][E]
    const double *cost;           // [T][E]
    const uint8_t *live;          // [T][E]
    int T, E, n_p;
    double gamma, lr;
    double *td;                   // [T-2][E]: td where valid, else 0
    uint8_t *valid;               // [T-2][E] or nullptr
    double *partial;              // [n_blocks][n_p + 2]
    unsigned int *ticket;         // [1], zero before the first launch (the kernel leaves it zero)
    double *msg;                  // [n_p + 2]
};

__global__ void __launch_bounds__(128) qlearning_td_grad_kernel(const QlTdArgs a) {
    __shared__ double w[TD_ROWS], okr[TD_ROWS];
    __shared__ double wsum, cnt;
    const long M = (long)(a.T - 2) * a.E;
    const long b0 = (long)blockIdx.x * TD_ROWS;
    const int P2 = a.n_p + 2;
    if (threadIdx.x < TD_ROWS) {
        const long j = b0 + threadIdx.x;
        double wj = 0.0, oj = 0.0;
        if (j < M) {
            const long E = a.E;
            const bool ok = a.live[j] && a.live[j + E] && a.live[j + 2 * E] && a.sq[j] == 0 && a.sv[j] == 0 && a.sq[j + E] == 0 && a.sv[j + E] == 0;
            double t;
            {
#pragma clang fp contract(off)      // cost + gamma V' - Q as the script writes it: product, sum, difference
                t = a.gamma * a.V[j + E];
                t = a.cost[j] + t;
                t = t - a.Q[j];
                wj = ok ? a.lr * t : 0.0;
            }
            a.td[j] = ok ? t : 0.0;
            if (a.valid) a.valid[j] = ok ? 1 : 0;
            oj = ok ? 1.0 : 0.0;
        }
        w[threadIdx.x] = wj, okr[threadIdx.x] = oj;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, n = 0.0;
        for (int r = 0; r < TD_ROWS; ++r) s += w[r], n += okr[r];
        wsum = s, cnt = n;
    }
    __syncthreads();
    const int nr = (int)(M - b0 < TD_ROWS ? M - b0 : TD_ROWS);
    double *row = a.partial + (long)blockIdx.x * P2;
    block_weighted_colsum<TD_ROWS>(w, a.dQ + b0 * a.n_p, nr, a.n_p, row);
    if (threadIdx.x == 0) row[a.n_p] = wsum, row[a.n_p + 1] = cnt;
    if (!last_workgroup(a.ticket)) return;
    sliced_final_sum<TD_PMAX, TD_ROWS>(a.partial, gridDim.x, P2, [&](int p, double s) { a.msg[p] = s; });
}

// After the collective: step = mask != 0 ? msg / max(1, count) : 0 (the mean of mean_update; a masked entry is selected out, never
// multiplied); theta += step.
__global__ void __launch_bounds__(256) qlearning_apply_kernel(const double *msg, int n_theta, const double *mask, double *theta, double *step_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_theta) return;
    const double c = msg[n_theta + 1] > 1.0 ? msg[n_theta + 1] : 1.0;
    const double st = (!mask || mask[i] != 0.0) ? msg[i] / c : 0.0;
    theta[i] = theta[i] + st;
    step_out[i] = st;
}

}  // namespace mpcrl
