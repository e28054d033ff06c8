// Batched PPO with the MPC as Gaussian actor (mpc4rl_amd/ppo.py; the roll-out step here is the one-control one, the chain's is in
// ppo_chain_kernel.hpp; the surrogate is written for 1 to 3 controls): what the reference's
// MPCActorCriticPolicy (rlmpc/ppo/policies.py:26-134) leaves as NotImplementedError, around the solves, on the device.  The policy is
// a ~ N(mu, sigma^2), mu = scale_action(u0*) of the solve, sigma = exp(log_std) with one learnable, state-independent log_std.
//   ppo_collect_kernel<Env>       one roll-out step after the policy's solve, one lane per environment: the sample and its log
//                                 probability, the environment step, row t of the roll-out tables, the reset of the environments that
//                                 ended, the observation and the cold mask of the next solve
//   ppo_gae_kernel                generalised advantage estimates, one lane per environment, serial over t = T-1 ... 0
//   ppo_adv_stats_kernel          count, sum and centred sum of squares of the advantages over the valid rows of a minibatch
//   ppo_surrogate_kernel          the clipped surrogate's terms and the message [-lr sum g_mu 2/(hi-lo) dpi/dp, -lr sum g_ls, count,
//                                 statistics], summed in a fixed order (no floating-point atomics)
//   ppo_log_std_apply_kernel      log_std += message / max(1, count), after the collective
// All PPO arithmetic is fp64.  The environment step is the shared device function of env_kernel.hpp (the same bits as
// mpcrl_env_cartpole_step); mean and log probability are the device functions below, shared by the roll-out and the surrogate, so a
// re-solve that returns the roll-out's u0 gives a ratio of exactly 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "env_kernel.hpp"
#include "batch_sum.hpp"

namespace mpcrl {

// the accept_status2 rule of mpcrl_policy_action: the solve converged or ran out of iterations, and u0 is a number
__device__ __forceinline__ bool ppo_solve_ok(int status, double u0) { return (status == 0 || status == 2) && isfinite(u0); }

// scale_action in fp64 (the fp64 part of policy_action_one); a rejected solve gives the zero action
__device__ __forceinline__ double ppo_mean(double u0, bool ok, double lo, double hi) {
#pragma clang fp contract(off)
    return ok ? 2.0 * ((u0 - lo) / (hi - lo)) - 1.0 : 0.0;
}

// log N(a; mu, sigma^2) with sigma = exp(log_std): -(a - mu)^2 / (2 sigma^2) - log_std - 1/2 log 2 pi
__device__ __forceinline__ double ppo_log_prob(double a, double mu, double sigma, double log_std) {
#pragma clang fp contract(off)
    const double d = a - mu;
    return -(d * d) / (2.0 * (sigma * sigma)) - log_std - 0.9189385332046727;
}

// What the roll-out step needs of a plant: PAIRS (the state as double2 pairs), the step from state s under the applied action (u01: the
// step's uniform draw), whether the episode ended after n steps, and the state the next episode starts from.
struct PpoCartpoleEnv {
    static constexpr int PAIRS = 2;
    CartpoleEnvPar par;
    __device__ __forceinline__ void step(const double2 *s, double action, double, double2 *nxt, double &reward, bool &terminated) const {
        const CartpoleStepOut o = cartpole_env_step(par, s[0].x, s[0].y, s[1].x, s[1].y, action);
        nxt[0] = make_double2(o.nx, o.nxd), nxt[1] = make_double2(o.nth, o.nthd), reward = o.reward, terminated = o.terminated;
    }
    __device__ __forceinline__ bool ended(bool terminated, int64_t n) const { return terminated || n >= par.max_episode_steps; }
    __device__ __forceinline__ void reset(double u01, double2 *s) const {      // (mpcrl_env_cartpole_reset)
        const CartpoleState r = cartpole_env_reset(u01);
        s[0] = r.s01, s[1] = r.s23;
    }
};

template <class Env>
struct PpoCollectArgs {
    Env env;
    int E, T, t;
    double *state;            // [E][nx] the environments' states
    int64_t *steps;           // [E] steps since the last reset
    const double *u0;         // [E] the policy's solve: control
    const int *status;        // [E]
    const float *eps;         // [E] standard-normal draws
    const double *u01;        // [E] uniform draws (the step's noise, the reset)
    const double *value;      // [E] the critic at the observation just solved
    const double *log_std;    // [1]
    double lo, hi, reward_scale;
    double *OBS, *ACT, *LOGP, *VAL, *REW, *NEXT;      // [T][E] ([..][nx] for OBS, NEXT)
    uint8_t *TERM, *DONE, *OK;                        // [T][E]
    double *obs;              // [E][nx] out: the next solve's x0 (after resets)
    int32_t *ended;           // [E] out: 1 = the episode ended (the next solve starts that instance cold)
};

template <class Env>
__global__ void __launch_bounds__(256) ppo_collect_kernel(const PpoCollectArgs<Env> a) {
    constexpr int W = Env::PAIRS;
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
    double2 s[W], nxt[W];
#pragma unroll
    for (int q = 0; q < W; ++q) s[q] = reinterpret_cast<const double2 *>(a.state)[W * i + q];
    // the stored sample is unclipped; the environment sees clip(a, -1, 1) (a NaN sample — log_std not finite — steps with NaN, as in torch)
    const double applied = act < -1.0 ? -1.0 : (act > 1.0 ? 1.0 : act);
    const double u01 = a.u01[i];
    double reward;
    bool terminated;
    a.env.step(s, applied, u01, nxt, reward, terminated);
    const int64_t n = a.steps[i] + 1;
    const bool done = a.env.ended(terminated, n);
    const long k = (long)a.t * a.E + i;
#pragma unroll
    for (int q = 0; q < W; ++q) {
        reinterpret_cast<double2 *>(a.OBS)[W * k + q] = s[q];
        reinterpret_cast<double2 *>(a.NEXT)[W * k + q] = nxt[q];       // before any reset: the bootstrap value is taken here
    }
    a.ACT[k] = act, a.LOGP[k] = logp, a.VAL[k] = a.value[i], a.REW[k] = a.reward_scale * reward;
    a.TERM[k] = terminated ? 1 : 0, a.DONE[k] = done ? 1 : 0, a.OK[k] = ok ? 1 : 0;
    // the environment goes on, or starts again
    if (done) a.env.reset(u01, nxt);
#pragma unroll
    for (int q = 0; q < W; ++q) {
        reinterpret_cast<double2 *>(a.state)[W * i + q] = nxt[q];
        reinterpret_cast<double2 *>(a.obs)[W * i + q] = nxt[q];
    }
    a.steps[i] = done ? 0 : n;
    a.ended[i] = done ? 1 : 0;
}

// stable_baselines3's RolloutBuffer.compute_returns_and_advantage with the time-limit bootstrap written as VNEXT on truncated rows:
//     delta_t = REW_t + gamma (1 - TERM_t) VNEXT_t - VAL_t;  adv_t = delta_t + gamma lambda (1 - DONE_t) adv_{t+1}, adv_T = 0;  ret_t = adv_t + VAL_t
// (every product and sum its own rounding, in the order of the torch statement ppo_gae)
__global__ void __launch_bounds__(256) ppo_gae_kernel(const double *REW, const double *VAL, const double *VNEXT, const uint8_t *TERM, const uint8_t *DONE,
                                                      int T, int E, double gamma, double lam, double *ADV, double *RET) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const double gl = gamma * lam;
    double adv = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        const long k = (long)t * E + e;
        const double v = VAL[k];
        const double nt = TERM[k] ? 0.0 : 1.0, nd = DONE[k] ? 0.0 : 1.0;
        const double delta = (REW[k] + (gamma * nt) * VNEXT[k]) - v;
        adv = delta + (gl * nd) * adv;
        ADV[k] = adv, RET[k] = adv + v;
    }
}

// The policy half of one minibatch update, for NU controls (1: the cartpole and the linear system; 3: the chain of masses, whose policy
// is the diagonal Gaussian of ppo_chain_kernel.hpp).  Rows b < M of the minibatch, j = idx[b] its row of the flattened [T E] tables:
//     valid_b = 0 <= j < n_rows, OK[j], the re-solve accepted (status 0 or 2, all NU u0_new finite), ACT (all NU), LOGP, ADV[j] finite
//     A_b     = normalize_adv and more than one valid row ? (ADV[j] - mean) / (std + 1e-8) : ADV[j]      (unbiased std, as torch.std)
//     logp_b  = sum_c log N(a_c; mu_c, sigma_c^2), c = 0 .. NU-1 in that order;   r_b = exp(logp_b - LOGP[j])
//     loss_b  = -min(r_b A_b, clip(r_b, 1 - eps, 1 + eps) A_b)
//     g_mu_c = -A r (a_c - mu_c) / sigma_c^2,  g_ls_c = -A r ((a_c - mu_c)^2 / sigma_c^2 - 1);  all 0 where the clipped branch is the minimum
// An invalid row is selected out (its u0_new / dpi_dp may be NaN); dpi_dp is read as nan_to_num does.  With NU = 1 these are the
// operations of the one-control kernel in its order.
constexpr int PPO_ROWS = 128, PPO_PMAX = 256, PPO_NS = 6, PPO_STAT_THREADS = 1024, PPO_NU_MAX = 3;
// message / partial columns after the n_p gradient entries: sum g_ls_0, count, sum loss, sum (r - 1) - log r, clipped rows, sum r;
// the message then carries the two advantage statistics: sum ADV and sum (ADV - mean)^2 over the valid rows.  With NU > 1 the sums of
// g_ls_c, c >= 1, follow: partial columns [n_p + PPO_NS + c - 1], message entries [n_p + PPO_MSG_EXTRA + c - 1] — the first
// n_p + PPO_MSG_EXTRA entries are the one-control layout, which mpcrl_qlearning_apply and the all-reduce read.
constexpr int PPO_MSG_EXTRA = 8;

struct PpoSurrogateArgs {
    const int64_t *idx;           // [M]
    int M, n_p;
    int64_t n_rows;               // rows of the flattened tables
    const double *ACT, *LOGP, *ADV;      // ACT [n_rows][NU]
    const uint8_t *OK;
    const double *u0_new;         // [M][NU]
    const int *status_new;        // [M]
    const double *dpi;            // [M][NU][n_p]
    const double *log_std;        // [NU]
    double lo[PPO_NU_MAX], hi[PPO_NU_MAX];
    double clip, ent_coef, lr;
    int normalize;
    double *partial;              // [n_blocks][n_p + PPO_NS + NU - 1]
    unsigned int *ticket;         // [1], zero before the first launch (the kernel leaves it zero)
    double *msg;                  // [n_p + PPO_MSG_EXTRA + NU - 1]
};

template <int NU>
__device__ __forceinline__ bool ppo_row_valid(const PpoSurrogateArgs &a, int b, long &j) {
    j = (long)a.idx[b];
    if (j < 0 || j >= a.n_rows) return false;
    bool ok = a.OK[j] != 0;
#pragma unroll
    for (int c = 0; c < NU; ++c) ok = ok && ppo_solve_ok(a.status_new[b], a.u0_new[(long)NU * b + c]) && isfinite(a.ACT[NU * j + c]);
    return ok && isfinite(a.LOGP[j]) && isfinite(a.ADV[j]);
}

// sum of v over the workgroup in a fixed order (a tree over the lanes' slots); every lane returns the total
__device__ __forceinline__ double ppo_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int m = PPO_STAT_THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// one workgroup: msg[n_p + 1] = valid rows, msg[n_p + 6] = sum ADV, msg[n_p + 7] = sum (ADV - mean)^2 over them (two passes)
template <int NU>
__global__ void __launch_bounds__(PPO_STAT_THREADS) ppo_adv_stats_kernel(const PpoSurrogateArgs a) {
    __shared__ double red[PPO_STAT_THREADS];
    double n = 0.0, s = 0.0;
    for (int b = threadIdx.x; b < a.M; b += PPO_STAT_THREADS) {
        long j;
        if (ppo_row_valid<NU>(a, b, j)) n += 1.0, s += a.ADV[j];
    }
    n = ppo_block_sum(n, red), s = ppo_block_sum(s, red);
    const double mean = s / (n > 1.0 ? n : 1.0);
    double q = 0.0;
    for (int b = threadIdx.x; b < a.M; b += PPO_STAT_THREADS) {
        long j;
        if (ppo_row_valid<NU>(a, b, j)) {
            const double d = a.ADV[j] - mean;
            q += d * d;
        }
    }
    q = ppo_block_sum(q, red);
    if (threadIdx.x == 0) a.msg[a.n_p + 1] = n, a.msg[a.n_p + 6] = s, a.msg[a.n_p + 7] = q;
}

// The sum is the fixed-order batch sum of batch_sum.hpp over blocks of PPO_ROWS rows — a row's NU sensitivity rows in the order of its
// controls: the same inputs give the same bits.
template <int NU>
__global__ void __launch_bounds__(PPO_ROWS) ppo_surrogate_kernel(const PpoSurrogateArgs a) {
    constexpr int NS = PPO_NS + NU - 1;
    __shared__ double w[PPO_ROWS * NU];          // [row][control]: block_weighted_colsum's weights of the block's PPO_ROWS x NU rows of dpi
    __shared__ double sc[NS][PPO_ROWS];
    const long b0 = (long)blockIdx.x * PPO_ROWS;
    const int P2 = a.n_p + NS;
    const double n_valid = a.msg[a.n_p + 1];
    double mean = 0.0, den = 1.0;
    if (a.normalize && n_valid > 1.0) {
        mean = a.msg[a.n_p + 6] / n_valid;
        den = sqrt(a.msg[a.n_p + 7] / (n_valid - 1.0)) + 1e-8;
    }
    {
        const long b = b0 + threadIdx.x;
        double wj[NU], v[NS];
#pragma unroll
        for (int c = 0; c < NU; ++c) wj[c] = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) v[q] = 0.0;
        long j;
        if (b < a.M && ppo_row_valid<NU>(a, (int)b, j)) {
            const double A = (a.ADV[j] - mean) / den;
            double d[NU], var[NU], logp = 0.0;
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                const double ls = a.log_std[c], sigma = exp(ls);
                var[c] = sigma * sigma;
                const double act = a.ACT[NU * j + c];
                const double mu = ppo_mean(a.u0_new[(long)NU * b + c], true, a.lo[c], a.hi[c]);
                const double lp = ppo_log_prob(act, mu, sigma, ls);
                logp = c == 0 ? lp : logp + lp;
                d[c] = act - mu;
            }
            const double logr = logp - a.LOGP[j];
            const double r = exp(logr);
            const double rc = r < 1.0 - a.clip ? 1.0 - a.clip : (r > 1.0 + a.clip ? 1.0 + a.clip : r);
            const double l1 = r * A, l2 = rc * A;
            const bool flat = (A > 0.0 && r > 1.0 + a.clip) || (A < 0.0 && r < 1.0 - a.clip);      // the clipped branch is the minimum
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                const double g_mu = flat ? 0.0 : -(A * r) * (d[c] / var[c]);
                const double g_ls = flat ? 0.0 : -(A * r) * (d[c] * d[c] / var[c] - 1.0);
                wj[c] = g_mu * (2.0 / (a.hi[c] - a.lo[c]));
                v[c == 0 ? 0 : PPO_NS + c - 1] = g_ls;
            }
            v[1] = 1.0, v[2] = -(l1 < l2 ? l1 : l2), v[3] = (r - 1.0) - logr, v[4] = fabs(r - 1.0) > a.clip ? 1.0 : 0.0, v[5] = r;
        }
#pragma unroll
        for (int c = 0; c < NU; ++c) w[NU * threadIdx.x + c] = wj[c];
#pragma unroll
        for (int q = 0; q < NS; ++q) sc[q][threadIdx.x] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double s = 0.0;
        for (int r = 0; r < PPO_ROWS; ++r) s += sc[threadIdx.x][r];
        a.partial[(long)blockIdx.x * P2 + a.n_p + threadIdx.x] = s;
    }
    const int nr = (int)(a.M - b0 < PPO_ROWS ? a.M - b0 : PPO_ROWS);
    block_weighted_colsum<PPO_ROWS>(w, a.dpi + b0 * NU * a.n_p, nr * NU, a.n_p, a.partial + (long)blockIdx.x * P2);
    if (!last_workgroup(a.ticket)) return;
    const int nb = gridDim.x;
    sliced_final_sum<PPO_PMAX, PPO_ROWS>(a.partial, nb, P2, [&](int p, double s) {
        // the step of theta and of log_std: -lr x the sums (the entropy bonus adds -ent_coef to every valid row's g_ls)
        if (p < a.n_p) s = -a.lr * s;
        if (p == a.n_p || p >= a.n_p + PPO_NS) s = -a.lr * (s - a.ent_coef * n_valid);
        a.msg[p < a.n_p + PPO_NS ? p : p + (PPO_MSG_EXTRA - PPO_NS)] = s;
    });
    // the workspace is left all zero
    for (long e = threadIdx.x; e < (long)nb * P2; e += PPO_ROWS) a.partial[e] = 0.0;
}

// After the collective: log_std[0] += msg[n_p] / max(1, msg[n_p + 1]) — the masked mean mpcrl_qlearning_apply takes for theta — and
// log_std[c] += msg[n_p + PPO_MSG_EXTRA + c - 1] / max(1, msg[n_p + 1]) for the controls c >= 1
__global__ void ppo_log_std_apply_kernel(const double *msg, int n_p, int nu, double *log_std) {
    const int c = threadIdx.x;
    if (blockIdx.x == 0 && c < nu) {
        const double cnt = msg[n_p + 1] > 1.0 ? msg[n_p + 1] : 1.0;
        log_std[c] = log_std[c] + msg[c == 0 ? n_p : n_p + PPO_MSG_EXTRA + c - 1] / cnt;
    }
}

}  // namespace mpcrl
