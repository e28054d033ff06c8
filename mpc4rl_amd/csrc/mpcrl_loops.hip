// mpcrl_loops.hip — the handle-less half of the C ABI of libmpcrl_hip.so (include/mpcrl.h): the library kernels of the RL loops
// (reduction, environments, replay, TD3 / Q-learning / policy-gradient / PPO / value / critic steps) and the probe of the dynamics
// jets.  Each export checks its arguments and launches on the device that owns its memory (ON_DEVICE_OF); the arithmetic is in the
// headers below.  A unit of its own: an edit to a loop kernel does not recompile the solve kernels of mpcrl_api.hip (csrc/Makefile).
#include "mpcrl_host.hpp"

#include <algorithm>
#include <cmath>

#include "reduce_kernel.hpp"
#include "env_kernel.hpp"
#include "critic_kernel.hpp"
#include "replay_kernel.hpp"
#include "td3_kernel.hpp"
#include "qlearning_kernel.hpp"
#include "qlearning_gn_kernel.hpp"
#include "cdpg_kernel.hpp"
#include "ppo_kernel.hpp"
#include "ppo_chain_kernel.hpp"
#include "value_kernel.hpp"
#include "linear_loop_kernel.hpp"
#include "chain_env_kernel.hpp"
#include "jet_probe_kernel.hpp"

using namespace mpcrl;

namespace {

// the 9 doubles of mpcrl_env_cartpole_step's `par` (host memory)
CartpoleEnvPar cartpole_env_par(const double *par) {
    CartpoleEnvPar p;
    p.gravity = par[0], p.masscart = par[1], p.masspole = par[2], p.length = par[3], p.force_mag = par[4], p.tau = par[5];
    p.x_threshold = par[6], p.theta_threshold = par[7], p.max_episode_steps = (long)par[8];
    return p;
}

// the 12 doubles of mpcrl_env_linear_step's `par` (host memory)
LinearEnvPar linear_env_par(const double *par) {
    LinearEnvPar p;
    for (int i = 0; i < 4; ++i) p.A[i] = par[i];
    p.B[0] = par[4], p.B[1] = par[5], p.lb_noise = par[6], p.ub_noise = par[7];
    p.low[0] = par[8], p.low[1] = par[9], p.high[0] = par[10], p.high[1] = par[11];
    return p;
}

// The plant arguments of mpcrl_env_chain_step / mpcrl_qlearning_chain_collect, checked: false = MPCRL_E_ARG.  wn may be NULL only without
// a disturbance.
bool chain_env_par(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, const double *wn, double w_std,
                   ChainEnvPar &e) {
    if (n_mass < 3 || n_mass > 7 || rk_steps < 1 || !(Ts > 0.0) || !p || !x_ss || !(w_std == w_std) || (w_std != 0.0 && !wn)) return false;
    const int64_t nl = n_mass - 1, m = n_mass - 2, nx = (2 * m + 1) * 3, n_p = 10 * nl + nx * nx + 9 + 3 * m;      // ChainDev<n_mass>::NP
    if (p_stride != 0 && p_stride != n_p) return false;
    e.p = p, e.p_stride = p_stride, e.x_ss = x_ss, e.wn = w_std != 0.0 ? wn : nullptr, e.h = Ts / rk_steps, e.w_std = w_std, e.rk_steps = rk_steps;
    return true;
}
// one instantiation per chain size (the host switches on n_mass)
#define CHAIN_ENV_SWITCH(n_mass, LAUNCH) \
    switch (n_mass) {                    \
        case 3: LAUNCH(3); break;        \
        case 4: LAUNCH(4); break;        \
        case 5: LAUNCH(5); break;        \
        case 6: LAUNCH(6); break;        \
        default: LAUNCH(7); break;       \
    }

// the launch of mpcrl_ppo_cartpole_collect / mpcrl_ppo_linear_collect, after their argument checks
template <class Env>
int launch_ppo_collect(const Env &env, int E, int T, int t, double *state, int64_t *steps, const double *u0, const int32_t *status, const float *eps,
                       const double *u01, const double *value, const double *log_std, double lo, double hi, double reward_scale, double *OBS,
                       double *ACT, double *LOGP, double *VAL, double *REW, double *NEXT, uint8_t *TERM, uint8_t *DONE, uint8_t *OK, double *obs,
                       int32_t *ended, void *stream) {
    ON_DEVICE_OF(OBS);
    PpoCollectArgs<Env> a;
    a.env = env;
    a.E = E, a.T = T, a.t = t, a.state = state, a.steps = steps, a.u0 = u0, a.status = (const int *)status, a.eps = eps, a.u01 = u01, a.value = value;
    a.log_std = log_std, a.lo = lo, a.hi = hi, a.reward_scale = reward_scale, a.OBS = OBS, a.ACT = ACT, a.LOGP = LOGP, a.VAL = VAL, a.REW = REW;
    a.NEXT = NEXT, a.TERM = TERM, a.DONE = DONE, a.OK = OK, a.obs = obs, a.ended = ended;
    hipLaunchKernelGGL(ppo_collect_kernel<Env>, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int mpcrl_weighted_grad_sum(const double *grad, int64_t ld, const double *weight, int rows, int n, double *out, void *stream) {
    if (!grad || !out || rows < 0 || n < 1 || ld < n) return MPCRL_E_ARG;
    ON_DEVICE_OF(out);
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipMemsetAsync(out, 0, (size_t)(n + 2) * sizeof(double), st));
    if (rows == 0) return 0;
    if (n <= REDUCE_MAXN_ROWPAR) {
        const int blocks = std::min(256, (rows + 255) / 256);
        hipLaunchKernelGGL(grad_reduce_rows_kernel, dim3(blocks), dim3(256), 0, st, grad, (long)ld, weight, rows, n, out);
    } else {
        const int ysplit = std::max(1, std::min(64, rows / 64));
        hipLaunchKernelGGL(grad_reduce_cols_kernel, dim3((n + 255) / 256, ysplit), dim3(256), 0, st, grad, (long)ld, weight, rows, n, out);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_env_cartpole_step(const double *par, int B, double *state, int64_t *steps, const double *action, void *obs, int obs_f32,
                            double *reward, uint8_t *terminated, uint8_t *truncated, void *stream) {
    if (!par || B < 0 || !state || !steps || !action || !reward || !terminated || !truncated) return MPCRL_E_ARG;
    if (B == 0) return 0;
    ON_DEVICE_OF(state);
    const CartpoleEnvPar p = cartpole_env_par(par);
    if (obs_f32)
        hipLaunchKernelGGL(env_cartpole_step_kernel<float>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, B, state, steps, action,
                           (float *)obs, reward, terminated, truncated);
    else
        hipLaunchKernelGGL(env_cartpole_step_kernel<double>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, B, state, steps, action,
                           (double *)obs, reward, terminated, truncated);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_policy_action(const double *u0, const int32_t *status, const float *noise, const double *lo, const double *hi, int B, int nu, int scale,
                        double sigma, double noise_clip, int accept_status2, float *action, uint8_t *ok, void *stream) {
    if (!u0 || !status || !lo || !hi || !action || B < 0 || nu < 1) return MPCRL_E_ARG;
    if (B == 0) return 0;
    ON_DEVICE_OF(action);
    hipLaunchKernelGGL(policy_action_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, u0, (const int *)status, noise, lo, hi, B, nu, scale,
                       (float)sigma, (float)noise_clip, accept_status2, action, ok);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_replay_sample(const float *table, int row_len, int nx, int E, int cap, int steps, const int64_t *idx, int B, const int64_t *pos_t,
                        int exclude_pos, const uint8_t *iter_ok, float *rows, double *obs64, double *nxt64, int64_t *row_s, int32_t *cold_s,
                        int64_t *row_n, int32_t *cold_n, void *stream) {
    if (!table || !idx || !rows || !obs64 || !nxt64 || B < 1 || nx < 1 || row_len < 2 * nx + 2 || E < 1 || cap < 1 || steps < 1 || steps > cap) return MPCRL_E_ARG;
    if (iter_ok && (!pos_t || !row_s || !cold_s || !row_n || !cold_n)) return MPCRL_E_ARG;
    if (exclude_pos && (!pos_t || steps != cap || cap < 2)) return MPCRL_E_ARG;
    ON_DEVICE_OF(rows);
    ReplaySampleArgs a;
    a.table = table, a.row_len = row_len, a.nx = nx, a.B = B, a.E = E, a.cap = cap, a.steps = steps, a.idx = idx, a.pos_t = pos_t, a.exclude = exclude_pos, a.iter_ok = iter_ok;
    a.rows = rows, a.obs64 = obs64, a.nxt64 = nxt64, a.row_s = row_s, a.row_n = row_n, a.cold_s = cold_s, a.cold_n = cold_n;
    hipLaunchKernelGGL(replay_sample_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_td3_cartpole_collect(const double *par, int E, double *state, int64_t *steps, const double *u0, const int32_t *status, const float *eps,
                               const double *u01, double lo, double hi, int scale, double sigma, double *obs, int32_t *ended, float *table, int cap,
                               double reward_scale, int64_t *pos, uint8_t *iter_ok, int64_t *iter_rows, double *stats, void *workspace, void *stream) {
    if (!par || E < 1 || !state || !steps || !u0 || !status || !eps || !u01 || !obs || !ended || !table || cap < 1 || !pos || !stats || !workspace)
        return MPCRL_E_ARG;
    ON_DEVICE_OF(state);
    Td3CollectArgs a;
    a.par = cartpole_env_par(par);
    a.E = E, a.state = state, a.steps = steps, a.u0 = u0, a.status = (const int *)status, a.eps = eps, a.u01 = u01, a.lo = lo, a.hi = hi, a.scale = scale;
    a.sigma = (float)sigma, a.obs = obs, a.ended = ended, a.table = table, a.cap = cap, a.reward_scale = reward_scale, a.pos = pos, a.iter_ok = iter_ok;
    a.iter_rows = iter_rows, a.stats = stats;
    set_ticket_workspace(a, workspace);
    hipLaunchKernelGGL(td3_cartpole_collect_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_td3_policy_post(const double *msg, int n_theta, double lr, const double *mask, double tau, double *theta, double *theta_target,
                          double *step_out, const float *crit, float *crit_target, int n_crit, void *stream) {
    if (!msg || n_theta < 1 || !mask || !theta || !theta_target || !step_out || n_crit < 0 || (n_crit > 0 && (!crit || !crit_target))) return MPCRL_E_ARG;
    ON_DEVICE_OF(theta);
    const int n = n_theta > n_crit ? n_theta : n_crit;
    hipLaunchKernelGGL(td3_policy_post_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, msg, n_theta, lr, mask, tau, theta, theta_target,
                       step_out, crit, crit_target, n_crit);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_qlearning_cartpole_collect(const double *par, int E, int T, double *state, int64_t *steps, const double *u0, const int32_t *status,
                                     const float *eps, double lo, double hi, double sigma, double *obs, uint8_t *alive, int32_t *row, int32_t *cold,
                                     double *S, double *A, double *C, uint8_t *live, void *stream) {
    if (!par || E < 1 || T < 1 || !state || !steps || !u0 || !status || !eps || !alive || !row || !S || !A || !C || !live || !(hi > lo))
        return MPCRL_E_ARG;
    ON_DEVICE_OF(state);
    QlCollectArgs a;
    a.par = cartpole_env_par(par);
    a.E = E, a.T = T, a.state = state, a.steps = steps, a.u0 = u0, a.status = (const int *)status, a.eps = eps, a.lo = lo, a.hi = hi;
    a.sigma = (float)sigma, a.obs = obs, a.alive = alive, a.row = row, a.cold = cold, a.S = S, a.A = A, a.C = C, a.live = live;
    hipLaunchKernelGGL(qlearning_cartpole_collect_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_qlearning_td_workspace_bytes(int T, int E, int n_p) {
    if (T < 2 || E < 1 || n_p < 1) return MPCRL_E_ARG;
    return ticket_workspace_bytes((int64_t)(T - 2) * E, TD_ROWS, n_p + 2);
}

int mpcrl_qlearning_td_grad(const double *Q, const double *V, const double *dQ_dp, const int32_t *status_q, const int32_t *status_v, const double *cost,
                            const uint8_t *live, int T, int E, int n_p, double gamma, double lr, void *workspace, double *td, uint8_t *valid, double *msg,
                            void *stream) {
    if (!msg || T < 2 || E < 1 || n_p < 1) return MPCRL_E_ARG;
    const int64_t M = (int64_t)(T - 2) * E;
    if (M > 0 && (!Q || !V || !dQ_dp || !status_q || !status_v || !cost || !live || !workspace || !td)) return MPCRL_E_ARG;
    ON_DEVICE_OF(msg);
    if (M == 0) {   // no term: an empty message
        HIP_OK(hipMemsetAsync(msg, 0, (size_t)(n_p + 2) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (ticket_blocks(M, TD_ROWS) > 0x7fffffff) return MPCRL_E_ARG;
    QlTdArgs a;
    a.Q = Q, a.V = V, a.dQ = dQ_dp, a.sq = (const int *)status_q, a.sv = (const int *)status_v, a.cost = cost, a.live = live;
    a.T = T, a.E = E, a.n_p = n_p, a.gamma = gamma, a.lr = lr, a.td = td, a.valid = valid;
    a.msg = msg;
    set_ticket_workspace(a, workspace);
    hipLaunchKernelGGL(qlearning_td_grad_kernel, dim3((unsigned)ticket_blocks(M, TD_ROWS)), dim3(TD_ROWS), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_qlearning_apply(const double *msg, int n_theta, const double *mask, double *theta, double *step_out, void *stream) {
    if (!msg || n_theta < 1 || !theta || !step_out) return MPCRL_E_ARG;
    ON_DEVICE_OF(theta);
    hipLaunchKernelGGL(qlearning_apply_kernel, dim3((n_theta + 255) / 256), dim3(256), 0, (hipStream_t)stream, msg, n_theta, mask, theta, step_out);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_qlearning_gn_workspace_bytes(int T, int E, int K) {
    if (T < 2 || E < 1 || K < 1 || K > GN_KMAX) return MPCRL_E_ARG;
    return ticket_workspace_bytes((int64_t)(T - 2) * E, TD_ROWS, gn_msg_len(K));
}

int mpcrl_qlearning_td_gn(const double *Q, const double *V, const double *dQ_dp, const int32_t *status_q, const int32_t *status_v, const double *cost,
                          const uint8_t *live, int T, int E, int n_p, double gamma, const int32_t *idx, int K, void *workspace, double *td,
                          uint8_t *valid, double *msg, void *stream) {
    if (!msg || T < 2 || E < 1 || n_p < 1 || K < 1 || K > GN_KMAX || K > n_p || !idx) return MPCRL_E_ARG;
    const int64_t M = (int64_t)(T - 2) * E;
    if (M > 0 && (!Q || !V || !dQ_dp || !status_q || !status_v || !cost || !live || !workspace || !td)) return MPCRL_E_ARG;
    ON_DEVICE_OF(msg);
    if (M == 0) {   // no term: an empty message
        HIP_OK(hipMemsetAsync(msg, 0, (size_t)gn_msg_len(K) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (ticket_blocks(M, TD_ROWS) > 0x7fffffff) return MPCRL_E_ARG;
    QlGnArgs a;
    a.Q = Q, a.V = V, a.dQ = dQ_dp, a.sq = (const int *)status_q, a.sv = (const int *)status_v, a.cost = cost, a.live = live;
    a.idx = (const int *)idx, a.T = T, a.E = E, a.n_p = n_p, a.K = K, a.gamma = gamma, a.td = td, a.valid = valid;
    a.msg = msg;
    set_ticket_workspace(a, workspace);
    const dim3 grid((unsigned)ticket_blocks(M, TD_ROWS)), block(TD_ROWS);
#define GN_LAUNCH(NC) hipLaunchKernelGGL(qlearning_td_gn_kernel<NC>, grid, block, 0, (hipStream_t)stream, a)
    switch (K / 16 + 1) {       // the column tiles of [G | b]: ceil((K + 1) / 16)
        case 1: GN_LAUNCH(1); break;
        case 2: GN_LAUNCH(2); break;
        case 3: GN_LAUNCH(3); break;
        case 4: GN_LAUNCH(4); break;
        default: GN_LAUNCH(5); break;
    }
#undef GN_LAUNCH
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_qlearning_gn_apply(const double *msg, int K, const int32_t *idx, int n_theta, double lr, double damping, double *theta, double *step_out,
                             int32_t *info, void *stream) {
    if (!msg || K < 1 || K > GN_KMAX || !idx || n_theta < K || !(lr == lr) || !(damping >= 0.0) || !theta || !step_out || !info) return MPCRL_E_ARG;
    ON_DEVICE_OF(theta);
    hipLaunchKernelGGL(qlearning_gn_apply_kernel, dim3(1), dim3(GN_APPLY_NT), 0, (hipStream_t)stream, msg, K, (const int *)idx, n_theta, lr, damping,
                       theta, step_out, (int *)info);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_qlearning_gn_apply_box(const double *msg, int K, const int32_t *idx, int n_theta, double lr, double damping, const double *lo, const double *hi,
                                 const double *scale, double radius, double *theta, double *step_out, uint8_t *active, int32_t *info, void *stream) {
    if (!msg || K < 1 || K > GN_KMAX || !idx || n_theta < K || !std::isfinite(lr) || !(std::isfinite(damping) && damping >= 0.0) || !lo || !hi ||
        !scale || !(radius > 0.0) || !theta || !step_out || !active || !info)
        return MPCRL_E_ARG;
    ON_DEVICE_OF(theta);
    hipLaunchKernelGGL(qlearning_gn_apply_box_kernel, dim3(1), dim3(GN_APPLY_NT), 0, (hipStream_t)stream, msg, K, (const int *)idx, n_theta, lr, damping,
                       lo, hi, scale, radius, theta, step_out, active, (int *)info);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_cdpg_record(const double *V, const double *u0, const double *du0_dp, const int32_t *status, const int32_t *row, const int32_t *idx, int E, int T,
                      int nu, int n_p, int K, double *Vt, double *U0, int32_t *St, double *Jt, void *stream) {
    if (K < 1 || K > GN_KMAX || nu < 1 || nu > CDPG_NU_MAX || T < 2 || E < 1 || n_p < 1 || !V || !u0 || !du0_dp || !status || !row || !idx || !Vt || !U0 ||
        !St || !Jt)
        return MPCRL_E_ARG;
    ON_DEVICE_OF(Jt);
    CdpgRecordArgs a;
    a.V = V, a.u0 = u0, a.du0 = du0_dp, a.status = (const int *)status, a.row = (const int *)row, a.idx = (const int *)idx;
    a.E = E, a.T = T, a.nu = nu, a.n_p = n_p, a.K = K, a.Vt = Vt, a.U0 = U0, a.St = (int *)St, a.Jt = Jt;
    const int64_t lanes = (int64_t)E * nu * K;
    hipLaunchKernelGGL(cdpg_record_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_cdpg_workspace_bytes(int T, int E, int K) {
    if (T < 2 || E < 1 || K < 1 || K > GN_KMAX) return MPCRL_E_ARG;
    return ticket_workspace_bytes((int64_t)(T - 2) * E, TD_ROWS, cdpg_msg_len(K));
}

int mpcrl_cdpg_terms(const double *Vt, const double *U0, const double *Jt, const int32_t *St, const double *act, const double *cost, const uint8_t *live,
                     int T, int E, int nu, int K, double gamma, void *workspace, double *delta, uint8_t *valid, double *msg, void *stream) {
    if (!msg || T < 2 || E < 1 || nu < 1 || nu > CDPG_NU_MAX || K < 1 || K > GN_KMAX) return MPCRL_E_ARG;
    const int64_t M = (int64_t)(T - 2) * E;
    if (M > 0 && (!Vt || !U0 || !Jt || !St || !act || !cost || !live || !workspace || !delta)) return MPCRL_E_ARG;
    ON_DEVICE_OF(msg);
    if (M == 0) {   // no term: an empty message
        HIP_OK(hipMemsetAsync(msg, 0, (size_t)cdpg_msg_len(K) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (ticket_blocks(M, TD_ROWS) > 0x7fffffff) return MPCRL_E_ARG;
    CdpgTermsArgs a;
    a.Vt = Vt, a.U0 = U0, a.Jt = Jt, a.St = (const int *)St, a.act = act, a.cost = cost, a.live = live;
    a.T = T, a.E = E, a.nu = nu, a.K = K, a.gamma = gamma, a.delta = delta, a.valid = valid;
    a.msg = msg;
    set_ticket_workspace(a, workspace);
    const dim3 grid((unsigned)ticket_blocks(M, TD_ROWS)), block(TD_ROWS);
#define CDPG_LAUNCH(NC) hipLaunchKernelGGL(cdpg_terms_kernel<NC>, grid, block, 0, (hipStream_t)stream, a)
    switch (K / 16 + 1) {       // the column tiles of [G | b]: ceil((K + 1) / 16)
        case 1: CDPG_LAUNCH(1); break;
        case 2: CDPG_LAUNCH(2); break;
        case 3: CDPG_LAUNCH(3); break;
        case 4: CDPG_LAUNCH(4); break;
        default: CDPG_LAUNCH(5); break;
    }
#undef CDPG_LAUNCH
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_cdpg_apply(const double *msg, int K, const int32_t *idx, int n_theta, double lr, double damping, int natural, const double *lo, const double *hi,
                     const double *scale, double radius, double *theta, double *step_out, double *w_out, uint8_t *active, int32_t *info, void *stream) {
    if (!msg || K < 1 || K > GN_KMAX || !idx || n_theta < K || !std::isfinite(lr) || !(std::isfinite(damping) && damping >= 0.0) || !(radius > 0.0) ||
        !theta || !step_out || !w_out || !active || !info)
        return MPCRL_E_ARG;
    ON_DEVICE_OF(theta);
    hipLaunchKernelGGL(cdpg_apply_kernel, dim3(1), dim3(GN_APPLY_NT), 0, (hipStream_t)stream, msg, K, (const int *)idx, n_theta, lr, damping, natural, lo,
                       hi, scale, radius, theta, step_out, w_out, active, (int *)info);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_ppo_cartpole_collect(const double *par, int E, int T, int t, double *state, int64_t *steps, const double *u0, const int32_t *status,
                               const float *eps, const double *u01, const double *value, const double *log_std, double lo, double hi,
                               double reward_scale, double *OBS, double *ACT, double *LOGP, double *VAL, double *REW, double *NEXT, uint8_t *TERM,
                               uint8_t *DONE, uint8_t *OK, double *obs, int32_t *ended, void *stream) {
    if (!par || E < 1 || T < 1 || t < 0 || t >= T || !state || !steps || !u0 || !status || !eps || !u01 || !value || !log_std || !(hi > lo) || !OBS ||
        !ACT || !LOGP || !VAL || !REW || !NEXT || !TERM || !DONE || !OK || !obs || !ended)
        return MPCRL_E_ARG;
    PpoCartpoleEnv env;
    env.par = cartpole_env_par(par);
    return launch_ppo_collect(env, E, T, t, state, steps, u0, status, eps, u01, value, log_std, lo, hi, reward_scale, OBS, ACT, LOGP, VAL, REW, NEXT,
                              TERM, DONE, OK, obs, ended, stream);
}

int mpcrl_ppo_gae(const double *REW, const double *VAL, const double *VNEXT, const uint8_t *TERM, const uint8_t *DONE, int T, int E, double gamma,
                  double gae_lambda, double *ADV, double *RET, void *stream) {
    if (!REW || !VAL || !VNEXT || !TERM || !DONE || !ADV || !RET || T < 1 || E < 1) return MPCRL_E_ARG;
    ON_DEVICE_OF(ADV);
    hipLaunchKernelGGL(ppo_gae_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, REW, VAL, VNEXT, TERM, DONE, T, E, gamma, gae_lambda, ADV,
                       RET);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_ppo_surrogate_workspace_bytes(int M, int n_p) {
    if (M < 1 || n_p < 1) return MPCRL_E_ARG;
    return ticket_workspace_bytes(M, PPO_ROWS, n_p + PPO_NS);
}

int64_t mpcrl_ppo_surrogate_workspace_bytes_nu(int M, int n_p, int nu) {
    if (M < 0 || n_p < 1 || nu < 1 || nu > PPO_NU_MAX) return MPCRL_E_ARG;
    return ticket_workspace_bytes(M, PPO_ROWS, n_p + PPO_NS + nu - 1);
}

// the two launches of mpcrl_ppo_surrogate_grad / mpcrl_ppo_surrogate_grad_nu, after their argument checks (lo, hi: nu host doubles)
static int launch_ppo_surrogate(const int64_t *idx, int M, int64_t n_rows, const double *ACT, const double *LOGP, const double *ADV, const uint8_t *OK,
                                const double *u0_new, const int32_t *status_new, const double *dpi_dp, int n_p, int nu, const double *log_std,
                                const double *lo, const double *hi, double clip_range, double ent_coef, double lr, int normalize_adv, void *workspace,
                                double *msg, void *stream) {
    ON_DEVICE_OF(msg);
    PpoSurrogateArgs a;
    a.idx = idx, a.M = M, a.n_p = n_p, a.n_rows = n_rows, a.ACT = ACT, a.LOGP = LOGP, a.ADV = ADV, a.OK = OK, a.u0_new = u0_new;
    a.status_new = (const int *)status_new, a.dpi = dpi_dp, a.log_std = log_std, a.clip = clip_range, a.ent_coef = ent_coef, a.lr = lr;
    for (int c = 0; c < PPO_NU_MAX; ++c) a.lo[c] = c < nu ? lo[c] : 0.0, a.hi[c] = c < nu ? hi[c] : 1.0;
    a.normalize = normalize_adv, a.msg = msg;
    set_ticket_workspace(a, workspace);
    const dim3 grid((unsigned)ticket_blocks(M, PPO_ROWS));
#define LAUNCH(NU)                                                                                                   \
    hipLaunchKernelGGL(ppo_adv_stats_kernel<NU>, dim3(1), dim3(PPO_STAT_THREADS), 0, (hipStream_t)stream, a); \
    hipLaunchKernelGGL(ppo_surrogate_kernel<NU>, grid, dim3(PPO_ROWS), 0, (hipStream_t)stream, a)
    switch (nu) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        default: LAUNCH(3); break;
    }
#undef LAUNCH
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_ppo_surrogate_grad(const int64_t *idx, int M, int64_t n_rows, const double *ACT, const double *LOGP, const double *ADV, const uint8_t *OK,
                             const double *u0_new, const int32_t *status_new, const double *dpi_dp, int n_p, const double *log_std, double lo, double hi,
                             double clip_range, double ent_coef, double lr, int normalize_adv, void *workspace, double *msg, void *stream) {
    if (!idx || M < 1 || n_rows < 1 || !ACT || !LOGP || !ADV || !OK || !u0_new || !status_new || !dpi_dp || n_p < 1 || !log_std || !(hi > lo) ||
        !(clip_range > 0.0) || !workspace || !msg)
        return MPCRL_E_ARG;
    return launch_ppo_surrogate(idx, M, n_rows, ACT, LOGP, ADV, OK, u0_new, status_new, dpi_dp, n_p, 1, log_std, &lo, &hi, clip_range, ent_coef, lr,
                                normalize_adv, workspace, msg, stream);
}

int mpcrl_ppo_surrogate_grad_nu(const int64_t *idx, int M, int64_t n_rows, const double *ACT, const double *LOGP, const double *ADV, const uint8_t *OK,
                                const double *u0_new, const int32_t *status_new, const double *dpi_dp, int n_p, int nu, const double *log_std,
                                const double *lo, const double *hi, double clip_range, double ent_coef, double lr, int normalize_adv, void *workspace,
                                double *msg, void *stream) {
    if (!idx || M < 0 || n_rows < 1 || !ACT || !LOGP || !ADV || !OK || !u0_new || !status_new || !dpi_dp || n_p < 1 || nu < 1 || nu > PPO_NU_MAX ||
        !log_std || !lo || !hi || !(clip_range > 0.0) || !workspace || !msg)
        return MPCRL_E_ARG;
    for (int c = 0; c < nu; ++c)
        if (!(hi[c] > lo[c])) return MPCRL_E_ARG;
    if (M == 0) return 0;
    return launch_ppo_surrogate(idx, M, n_rows, ACT, LOGP, ADV, OK, u0_new, status_new, dpi_dp, n_p, nu, log_std, lo, hi, clip_range, ent_coef, lr,
                                normalize_adv, workspace, msg, stream);
}

int mpcrl_ppo_log_std_apply(const double *msg, int n_p, double *log_std, void *stream) {
    return mpcrl_ppo_log_std_apply_nu(msg, n_p, 1, log_std, stream);
}

int mpcrl_ppo_log_std_apply_nu(const double *msg, int n_p, int nu, double *log_std, void *stream) {
    if (!msg || n_p < 1 || nu < 1 || nu > PPO_NU_MAX || !log_std) return MPCRL_E_ARG;
    ON_DEVICE_OF(log_std);
    hipLaunchKernelGGL(ppo_log_std_apply_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, msg, n_p, nu, log_std);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_value_forward(const double *obs, int64_t n, int nx, const float *params, double *values, void *stream) {
    if (!obs || !params || !values || n < 0 || nx < 1 || nx > VALUE_DMAX || (n + VALUE_S - 1) / VALUE_S > 0x7fffffffLL) return MPCRL_E_ARG;
    if (n == 0) return 0;
    ON_DEVICE_OF(values);
    hipLaunchKernelGGL(value_forward_kernel, dim3((unsigned)((n + VALUE_S - 1) / VALUE_S)), dim3(VALUE_NT), 0, (hipStream_t)stream, obs, (long)n, nx, params,
                       values);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_value_workspace_bytes(int M, int nx) {
    if (M < 1 || nx < 1 || nx > VALUE_DMAX) return MPCRL_E_ARG;
    return (((int64_t)M + VALUE_S - 1) / VALUE_S) * (value_n_params(nx) + 2) * (int64_t)sizeof(double);
}

int mpcrl_value_mse_grad(const double *OBS, const double *RET, const int64_t *idx, int M, int64_t n_rows, int nx, const float *params, double vf_coef,
                         double out_scale, void *workspace, double *out, void *stream) {
    if (!OBS || !RET || !idx || !params || !workspace || !out || M < 1 || n_rows < 0 || nx < 1 || nx > VALUE_DMAX) return MPCRL_E_ARG;
    ON_DEVICE_OF(out);
    ValueMseArgs a;
    a.OBS = OBS, a.RET = RET, a.idx = idx, a.M = M, a.nx = nx, a.n_rows = (long)n_rows, a.params = params, a.partial = (double *)workspace;
    const int n_blocks = (int)(((int64_t)M + VALUE_S - 1) / VALUE_S), n_params = value_n_params(nx);
    hipLaunchKernelGGL(value_mse_partial_kernel, dim3(n_blocks), dim3(VALUE_NT), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(value_mse_reduce_kernel, dim3((n_params + 1 + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const double *)workspace, n_blocks, nx,
                       vf_coef, out_scale, out);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_dpg_workspace_bytes(int B, int n_p) {
    if (B < 1 || n_p < 1) return MPCRL_E_ARG;
    return ticket_workspace_bytes(B, DPG_ROWS, n_p + 1);
}

int mpcrl_dpg_grad(const float *dq_da, const uint8_t *ok, const double *dpi_dp, int B, int nu, int n_p, const double *lo, const double *hi, int scale,
                   void *workspace, double *out, void *stream) {
    if (!dq_da || !dpi_dp || !workspace || !out || B < 1 || nu < 1 || nu > 8 || n_p < 1 || (scale && (!lo || !hi))) return MPCRL_E_ARG;
    ON_DEVICE_OF(out);
    DpgArgs a;
    a.dq_da = dq_da, a.ok = ok, a.dpi_dp = dpi_dp, a.B = B, a.nu = nu, a.n_p = n_p, a.scale = scale, a.lo = lo, a.hi = hi;
    a.out = out;
    set_ticket_workspace(a, workspace);
    hipLaunchKernelGGL(dpg_grad_kernel, dim3((unsigned)ticket_blocks(B, DPG_ROWS)), dim3(128), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t mpcrl_critic_workspace_bytes(int B, int nx, int nu, int n_critics) {
    if (B < 0 || nx < 1 || nu < 1 || nx + nu > CRITIC_DMAX || n_critics < 1 || n_critics > 2) return MPCRL_E_ARG;
    const int64_t n_blocks = (B + CRITIC_S - 1) / CRITIC_S, n_params = (int64_t)n_critics * (CRITIC_H * (nx + nu) + CRITIC_H * CRITIC_H + 3 * CRITIC_H + 1);
    return n_blocks * (n_params + 2) * (int64_t)sizeof(float);
}

int mpcrl_critic_td_grad(const float *rows, int row_stride, int B, int nx, int nu, const float *a_next, const uint8_t *ok_u, const float *params,
                         const float *params_target, int n_critics, double gamma, double out_scale, void *workspace, double *grad, float *loss_out,
                         uint8_t *ok_out, void *stream) {
    if (!rows || !a_next || !params || !params_target || !workspace || !grad || B < 1 || nx < 1 || nu < 1 || nx + nu > CRITIC_DMAX || n_critics < 1 ||
        n_critics > 2 || row_stride < 2 * nx + nu + 2)
        return MPCRL_E_ARG;
    ON_DEVICE_OF(grad);
    CriticArgs a;
    a.rows = rows, a.row_stride = row_stride, a.row_len = 2 * nx + nu + 2, a.B = B, a.nx = nx, a.nu = nu, a.n_critics = n_critics;
    a.a_next = a_next, a.ok_u = ok_u, a.params = params, a.params_target = params_target, a.gamma = (float)gamma;
    a.partial = (float *)workspace, a.ok_out = ok_out;
    const int n_blocks = (B + CRITIC_S - 1) / CRITIC_S, n_params = n_critics * (CRITIC_H * (nx + nu) + CRITIC_H * CRITIC_H + 3 * CRITIC_H + 1);
    if (nx + nu <= 16)
        hipLaunchKernelGGL(critic_td_partial_kernel<2>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(critic_td_partial_kernel<1>, dim3(n_blocks), dim3(128), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(critic_td_reduce_kernel, dim3((n_params + 1 + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const float *)workspace, n_blocks, n_params,
                       nx + nu, out_scale, grad, loss_out);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_critic_dq_da(const float *obs, int obs_stride, int B, int nx, int nu, const float *act, const uint8_t *ok, const float *params, float *dq_da,
                       uint8_t *ok_out, void *stream) {
    if (!obs || !act || !params || !dq_da || B < 1 || nx < 1 || nu < 1 || nx + nu > CRITIC_DMAX || obs_stride < nx) return MPCRL_E_ARG;
    ON_DEVICE_OF(dq_da);
    CriticDqdaArgs a;
    a.obs = obs, a.obs_stride = obs_stride, a.B = B, a.nx = nx, a.nu = nu, a.act = act, a.ok = ok, a.params = params, a.dq_da = dq_da, a.ok_out = ok_out;
    hipLaunchKernelGGL(critic_dqda_kernel, dim3((B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_env_linear_step(const double *par, int B, double *state, const double *action, const double *u01, void *obs, int obs_f32,
                          double *cost, void *stream) {
    if (!par || B < 0 || !state || !action || !u01 || !cost) return MPCRL_E_ARG;
    if (B == 0) return 0;
    ON_DEVICE_OF(state);
    const LinearEnvPar p = linear_env_par(par);
    if (obs_f32)
        hipLaunchKernelGGL(env_linear_step_kernel<float>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, B, state, action, u01, (float *)obs, cost);
    else
        hipLaunchKernelGGL(env_linear_step_kernel<double>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, B, state, action, u01, (double *)obs, cost);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_qlearning_linear_collect(const double *par, int E, int T, double *state, const double *u0, const int32_t *status, const float *eps,
                                   const double *u01, double lo, double hi, double sigma, double *obs, int32_t *row, int32_t *cold, double *S,
                                   double *A, double *C, void *stream) {
    if (!par || E < 0 || T < 1 || !state || !u0 || !status || !eps || !u01 || !obs || !row || !cold || !S || !A || !C || !(hi > lo)) return MPCRL_E_ARG;
    if (E == 0) return 0;
    ON_DEVICE_OF(state);
    QlLinearCollectArgs a;
    a.par = linear_env_par(par);
    a.E = E, a.T = T, a.state = state, a.u0 = u0, a.status = (const int *)status, a.eps = eps, a.u01 = u01, a.lo = lo, a.hi = hi;
    a.sigma = (float)sigma, a.obs = obs, a.row = row, a.cold = cold, a.S = S, a.A = A, a.C = C;
    hipLaunchKernelGGL(qlearning_linear_collect_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_ppo_linear_collect(const double *par, int E, int T, int t, double *state, int64_t *steps, const double *u0, const int32_t *status,
                             const float *eps, const double *u01, const double *value, const double *log_std, double lo, double hi,
                             double reward_scale, int64_t episode_length, const double *reset_state, double *OBS, double *ACT, double *LOGP,
                             double *VAL, double *REW, double *NEXT, uint8_t *TERM, uint8_t *DONE, uint8_t *OK, double *obs, int32_t *ended,
                             void *stream) {
    if (!par || E < 0 || T < 1 || t < 0 || t >= T || episode_length < 1 || !reset_state || !state || !steps || !u0 || !status || !eps || !u01 ||
        !value || !log_std || !(hi > lo) || !OBS || !ACT || !LOGP || !VAL || !REW || !NEXT || !TERM || !DONE || !OK || !obs || !ended)
        return MPCRL_E_ARG;
    if (E == 0) return 0;
    PpoLinearEnv env;
    env.par = linear_env_par(par), env.episode_length = episode_length, env.reset0 = reset_state[0], env.reset1 = reset_state[1];
    return launch_ppo_collect(env, E, T, t, state, steps, u0, status, eps, u01, value, log_std, lo, hi, reward_scale, OBS, ACT, LOGP, VAL, REW, NEXT,
                              TERM, DONE, OK, obs, ended, stream);
}

int mpcrl_env_chain_step(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, int B, double *state,
                         const double *action, const double *wn, double w_std, void *obs, int obs_f32, double *cost, void *stream) {
    ChainEnvPar e;
    if (!chain_env_par(n_mass, Ts, rk_steps, p, p_stride, x_ss, wn, w_std, e) || B < 0 || !state || !action || !cost) return MPCRL_E_ARG;
    if (B == 0) return 0;
    ON_DEVICE_OF(state);
#define LAUNCH(NM) \
    hipLaunchKernelGGL(env_chain_step_kernel<NM>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, e, B, state, action, obs, obs_f32, cost)
    CHAIN_ENV_SWITCH(n_mass, LAUNCH)
#undef LAUNCH
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_qlearning_chain_collect(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, double w_std, int E,
                                  int T, double *state, const double *u0, const int32_t *status, const float *eps, const double *wn,
                                  const double *lo, const double *hi, double sigma, double *obs, int32_t *row, int32_t *cold, double *S, double *A,
                                  double *C, void *stream) {
    QlChainCollectArgs a;
    if (!chain_env_par(n_mass, Ts, rk_steps, p, p_stride, x_ss, wn, w_std, a.env) || E < 0 || T < 1 || !state || !u0 || !status || !eps || !lo ||
        !hi || !obs || !row || !cold || !S || !A || !C || !(sigma >= 0.0) || !std::isfinite(sigma))
        return MPCRL_E_ARG;
    for (int j = 0; j < 3; ++j) {
        if (!(hi[j] > lo[j])) return MPCRL_E_ARG;
        a.lo[j] = lo[j], a.hi[j] = hi[j];
    }
    if (E == 0) return 0;
    ON_DEVICE_OF(state);
    a.E = E, a.T = T, a.state = state, a.u0 = u0, a.status = (const int *)status, a.eps = eps, a.sigma = (float)sigma;
    a.obs = obs, a.row = row, a.cold = cold, a.S = S, a.A = A, a.C = C;
#define LAUNCH(NM) hipLaunchKernelGGL(qlearning_chain_collect_kernel<NM>, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, a)
    CHAIN_ENV_SWITCH(n_mass, LAUNCH)
#undef LAUNCH
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_ppo_chain_collect(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, double w_std, int E, int T,
                            int t, double *state, int64_t *steps, const double *u0, const int32_t *status, const float *eps, const double *wn,
                            const double *value, const double *log_std, const double *lo, const double *hi, double reward_scale,
                            int64_t episode_length, const double *x_reset, double vel_std, const double *rn, double *OBS, double *ACT, double *LOGP,
                            double *VAL, double *REW, double *NEXT, uint8_t *TERM, uint8_t *DONE, uint8_t *OK, double *obs, int32_t *ended,
                            void *stream) {
    PpoChainCollectArgs a;
    if (!chain_env_par(n_mass, Ts, rk_steps, p, p_stride, x_ss, wn, w_std, a.env) || E < 0 || T < 1 || t < 0 || t >= T || episode_length < 1 ||
        !state || !steps || !u0 || !status || !eps || !value || !log_std || !lo || !hi || !x_reset || !(vel_std == vel_std) ||
        (vel_std != 0.0 && !rn) || !OBS || !ACT || !LOGP || !VAL || !REW || !NEXT || !TERM || !DONE || !OK || !obs || !ended)
        return MPCRL_E_ARG;
    for (int j = 0; j < 3; ++j) {
        if (!(hi[j] > lo[j])) return MPCRL_E_ARG;
        a.lo[j] = lo[j], a.hi[j] = hi[j];
    }
    if (E == 0) return 0;
    ON_DEVICE_OF(state);
    a.E = E, a.T = T, a.t = t, a.state = state, a.steps = steps, a.u0 = u0, a.status = (const int *)status, a.eps = eps, a.value = value;
    a.log_std = log_std, a.reward_scale = reward_scale, a.episode_length = episode_length, a.x_reset = x_reset, a.vel_std = vel_std;
    a.rn = vel_std != 0.0 ? rn : nullptr, a.OBS = OBS, a.ACT = ACT, a.LOGP = LOGP, a.VAL = VAL, a.REW = REW, a.NEXT = NEXT, a.TERM = TERM, a.DONE = DONE;
    a.OK = OK, a.obs = obs, a.ended = ended;
#define LAUNCH(NM) hipLaunchKernelGGL(ppo_chain_collect_kernel<NM>, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, a)
    CHAIN_ENV_SWITCH(n_mass, LAUNCH)
#undef LAUNCH
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_env_cartpole_reset(int B, double *state, int64_t *steps, const uint8_t *mask, const double *u01, void *obs, int obs_f32,
                             void *stream) {
    if (B < 0 || !state || !steps || !u01) return MPCRL_E_ARG;
    if (B == 0) return 0;
    ON_DEVICE_OF(state);
    if (obs_f32)
        hipLaunchKernelGGL(env_cartpole_reset_kernel<float>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, state, steps, mask, u01, (float *)obs);
    else
        hipLaunchKernelGGL(env_cartpole_reset_kernel<double>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, state, steps, mask, u01, (double *)obs);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_debug_model_jets(int model, int which, int n, double h, int rk_steps, const double *x, const double *u, const double *th,
                           const double *aux, double *out, void *stream) {
    if (n < 1 || which < 0 || which > 4 || !x || !out) return MPCRL_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (which == 4) {
        if (device_of(x) < 0 || device_of(x) != device_of(out)) return MPCRL_E_ARG;
        ON_DEVICE_OF(out);
        hipLaunchKernelGGL(jet_rcp_probe_kernel, grid, block, 0, st, n, x, out);
        HIP_OK(hipGetLastError());
        return 0;
    }
    const bool need_aux = which == 1 || which == 3;
    if (!u || !th || (need_aux && !aux)) return MPCRL_E_ARG;
    if (model != MPCRL_MODEL_CARTPOLE && model != MPCRL_MODEL_LINEAR) return MPCRL_E_ARG;   // the chain's derivatives do not go through the jets
    if (model == MPCRL_MODEL_CARTPOLE && (rk_steps < 1 || rk_steps > 4)) return MPCRL_E_ARG;
    for (const void *q : {(const void *)x, (const void *)u, (const void *)th, (const void *)(need_aux ? aux : x)})
        if (device_of(q) < 0 || device_of(q) != device_of(out)) return MPCRL_E_ARG;
    ON_DEVICE_OF(out);
#define MPCRL_JET_PROBE(MODEL, DEV, W) \
    if (model == MODEL && which == W) { \
        hipLaunchKernelGGL((jet_probe_kernel<DEV, W>), grid, block, 0, st, n, h, rk_steps, x, u, th, aux, out); \
        HIP_OK(hipGetLastError()); \
        return 0; \
    }
    MPCRL_JET_PROBE(MPCRL_MODEL_CARTPOLE, CartpoleDev, 0) MPCRL_JET_PROBE(MPCRL_MODEL_CARTPOLE, CartpoleDev, 1)
    MPCRL_JET_PROBE(MPCRL_MODEL_CARTPOLE, CartpoleDev, 2) MPCRL_JET_PROBE(MPCRL_MODEL_CARTPOLE, CartpoleDev, 3)
    MPCRL_JET_PROBE(MPCRL_MODEL_LINEAR, LinearDev, 0) MPCRL_JET_PROBE(MPCRL_MODEL_LINEAR, LinearDev, 1)
    MPCRL_JET_PROBE(MPCRL_MODEL_LINEAR, LinearDev, 2) MPCRL_JET_PROBE(MPCRL_MODEL_LINEAR, LinearDev, 3)
#undef MPCRL_JET_PROBE
    return MPCRL_E_ARG;
}

}  // extern "C"
