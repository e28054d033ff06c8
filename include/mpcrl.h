/* mpcrl.h — C ABI of the MI355X-native batched MPC-as-policy engine (libmpcrl_hip.so).
 *
 * This is the drop-in boundary for the hot path of MPC-Based-Reinforcement-Learning/mpc4rl:
 *
 *   reference interface replaced                               entry point here
 *   --------------------------------------------------------   ---------------------------------
 *   AcadosOcpSolver(ocp) + build_nlp(ocp)                      mpcrl_create
 *     rlmpc/mpc/cartpole/acados.py:192-203,
 *     rlmpc/mpc/linear_system/acados.py:20-22,126-129,
 *     rlmpc/mpc/chain_mass/acados.py:27-29,45
 *   ocp_solver.set(stage,"p",..) / cost_set(stage,"W"|"yref")  mpcrl_set_theta   (the cartpole cost block W_0, W, W_e,
 *     rlmpc/mpc/common/mpc.py:137-154,212-257                    yref_0, yref, yref_e of p is what the solve uses)
 *   ocp_solver.constraints_set(stage,"lbu"|"ubu"|"lbx"|"ubx")  mpcrl_set_bounds
 *     rlmpc/mpc/common/mpc.py:72-73,87-88
 *   float(nlp.L.val)  (MPC.get_L)                              mpcrl_get_lagrangian
 *     rlmpc/mpc/common/mpc.py:325-332
 *   shared_lib.ocp_nlp_cost_model_set(.., "scaling", gamma^k)  mpcrl_set_gamma
 *     rlmpc/mpc/common/mpc.py:259-285  (the reference's one raw C call)
 *   ocp_solver.reset(); set(stage,"x",x0)                      mpcrl_reset
 *     rlmpc/mpc/common/mpc.py:204-210
 *   set(0,"lbx"/"ubx",x0) [+ constraints_set(0,"lbu"/"ubu",u0)];   mpcrl_solve
 *   ocp_solver.solve(); get(0,"u"); get_cost(); update_nlp()
 *     rlmpc/mpc/common/mpc.py:27-50,52-96,177-202 and
 *     rlmpc/mpc/nlp.py:1341-1424 (dL_dp, dpi_dp)
 *   ocp_solver.get(stage, "x"|"u"|"pi"|"lam"|"t"|"sl"|"su")   mpcrl_get_iterate
 *   ocp_solver.set(stage, "x"|"u"|"pi", v) / load_iterate      mpcrl_set_iterate
 *     rlmpc/mpc/nlp.py:1354-1372, rlmpc/examples/chain_mass.py:119-120
 *   the one warm solver object SB3's replay loop reuses          mpcrl_get_iterate_rows / mpcrl_set_iterate_rows
 *     rlmpc/td3/policies.py:186-213                              (per-transition iterates of a replay buffer)
 *   perturb_action + env.step + replay_buffer.add of the        mpcrl_qlearning_cartpole_collect
 *   cartpole Q-learning roll-out
 *     scripts/cartpole_mpc_qlearning.py:104-107,223-234
 *   td_error, dp = LR td dQ_dp, np.mean(dp) of the learning   mpcrl_qlearning_td_grad / mpcrl_qlearning_td_workspace_bytes,
 *   sweep; mpc.set_p(p + mean)                                  mpcrl_qlearning_apply
 *     scripts/cartpole_mpc_qlearning.py:255-269
 *   (none: the reference steps p by LR td dQ_dp only)          mpcrl_qlearning_td_gn / mpcrl_qlearning_gn_workspace_bytes,
 *   the same sweep's Gauss-Newton (least-squares TD) step        mpcrl_qlearning_gn_apply, and inside bounds on the parameters
 *                                                                and a trust region: mpcrl_qlearning_gn_apply_box
 *   MPCActorCriticPolicy.forward / evaluate_actions /          mpcrl_ppo_cartpole_collect, mpcrl_ppo_gae,
 *   predict_values (NotImplementedError in the reference)       mpcrl_ppo_surrogate_grad / mpcrl_ppo_surrogate_workspace_bytes,
 *   and the PPO roll-out / update around them                   mpcrl_ppo_log_std_apply,
 *     rlmpc/ppo/policies.py:26-134                               mpcrl_value_forward, mpcrl_value_mse_grad / mpcrl_value_workspace_bytes
 *   mpc.get_action + env.step + replay_buffer.add of the       mpcrl_qlearning_linear_collect  (PPO on the same plant:
 *   linear system's Q-learning roll-out                          mpcrl_ppo_linear_collect)
 *     rlmpc/examples/linear_system_mpc_qlearning.py:160-172
 *   the chain of masses as a plant (f_expl + RK4, the model's     mpcrl_env_chain_step, and the roll-out step of its Q-learning
 *   own map at the plant's parameters, with a disturbance)       loop around it: mpcrl_qlearning_chain_collect
 *     rlmpc/mpc/chain_mass/ocp_utils.py:76-130
 *
 * Conventions
 *   - plain C, no torch types.  Every array argument of mpcrl_solve / *_iterate / mpcrl_reset /
 *     mpcrl_set_theta is a DEVICE pointer (HIP), double precision, row-major, owned by the caller.
 *   - the handle owns the warm-start iterate and all workspace; mpcrl_solve allocates nothing and is
 *     asynchronous on the given HIP stream.  A new handle holds the cold iterate (x = 0, u = 0, multipliers 0,
 *     slacks 1); mpcrl_reset(h, x0) restores it with x_k = x0.
 *   - return value: 0 ok, < 0 API misuse (MPCRL_E_*).  Per-instance solver status goes to status[B]
 *     with acados' numbering: 0 success, 1 NaN, 2 max-iter, 4 QP failure (reference: solve() returns
 *     int status, update/q_update raise on != 0, rlmpc/mpc/common/mpc.py:81-83,197-198).
 *   - one handle per (device, stream); handles are independent across GPUs; not re-entrant (stateful
 *     warm start, like the reference's solver object).
 *   - how a batch is laid out over wavefronts (packing order, plain or time-sliced launch of the small
 *     solve kernel; environment MPCRL_TIME_SLICE=0/1 read at mpcrl_create overrides the automatic choice)
 *     never changes a result bit.
 *   - linear-system model: environment MPCRL_LINEAR_SPL=1 at mpcrl_create keeps the one-stage-per-lane solve kernel instead
 *     of the three-stages-per-lane one.  Same iteration, sums associated differently: results equal to rounding EXCEPT where a
 *     stopping test is met within rounding — there the interior-point count can differ by one, an RTI call's status can differ,
 *     and the outputs agree to the QP tolerance only (see ABI 110 below).
 *   - linear-system model, warm calls: an instance whose WARM-started interior point runs out of iterations (it can jam against the
 *     rows a moved x0 activates) solves that QP once more from the cold interior point before status 4 is reported — the QP is convex,
 *     the cold start solves it; its iteration count then includes both attempts (> 60).  No signature or output layout changes.
 *   - cartpole: environment MPCRL_GENERIC_ROWS=1 at mpcrl_create keeps the generic solve kernels where the bounds would select the
 *     ones with the full-box bound pattern compiled in (mpcrl_query_box_rows); the two forms return the same bits.
 *   - cartpole: a wavefront holds min(floor(64 / (N + 1)), 4) instances — four is the number of 4x4 blocks of the
 *     matrix-core sweeps — so horizons below N = 15 use fewer of its lanes than a lane-per-stage packing could.
 */
#ifndef MPCRL_H
#define MPCRL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version = what mpcrl_version() of the library returns.  Bumped whenever the signature or the meaning of an exported function
 * changes; a binding must compare the two before its first call (mpc4rl_amd/_lib.py does).
 *   100  rounds 1-3
 *   110  round 4/5: mpcrl_query_time_sliced(h, flags, stream) gained `stream`; mpcrl_env_cartpole_step / _reset and
 *        mpcrl_env_linear_step gained `obs_f32` (obs became void*); mpcrl_set_exit_rule accepts the chain of masses;
 *        mpcrl_create refuses chain horizons whose trajectories do not fit the LDS of one workgroup (MPCRL_E_ARG).
 *        Behavioural change under 110 (round 5): the linear-system model's default solve kernel became lq_solve_kernel (three
 *        stages per lane; MPCRL_LINEAR_SPL=1 keeps the old one) — the SAME iteration with its sums associated differently, so a
 *        stopping test that is met within rounding can end an interior-point loop one iteration earlier or later (< 1 % of
 *        instances), or flip the status of an RTI call whose residual sits at the tolerance; outputs of such an instance then
 *        agree with the one-stage kernel and the oracle port to the QP tolerance (1e-4 ... 1e-3 on du0/dp), not to rounding
 *   120  round 6: mpcrl_solve flags MPCRL_NO_BND_STORE and MPCRL_EXACT_QP (test-only); mpcrl_get_iterate_rows / mpcrl_set_iterate_rows; mpcrl_policy_action
 *   130  round 6: mpcrl_critic_td_grad / mpcrl_critic_workspace_bytes / mpcrl_critic_dq_da (the TD3 learner's critic step); mpcrl_replay_sample; mpcrl_dpg_grad / mpcrl_dpg_workspace_bytes; mpcrl_td3_cartpole_collect; mpcrl_td3_policy_post; linear system: a
 *        failed WARM QP restarts cold (behaviour, see above)
 *   131  round 7: mpcrl_qlearning_cartpole_collect; mpcrl_qlearning_td_grad / mpcrl_qlearning_td_workspace_bytes; mpcrl_qlearning_apply
 *        (the batched Q-learning loop of the cartpole); nothing existing changed
 *   132  mpcrl_td3_policy_post: a masked entry (mask_i == 0) is selected out, step_i = 0, instead of multiplied by 0 — a NaN or +-inf
 *        message there no longer turns a frozen theta_i into NaN (behaviour; the signature is unchanged)
 *        additions under 132 (no existing export changed, so no bump): mpcrl_ppo_cartpole_collect; mpcrl_ppo_gae;
 *        mpcrl_ppo_surrogate_grad / mpcrl_ppo_surrogate_workspace_bytes; mpcrl_ppo_log_std_apply (batched PPO with the MPC as
 *        Gaussian actor, cartpole); round 8: mpcrl_value_forward; mpcrl_value_mse_grad / mpcrl_value_workspace_bytes (PPO's value
 *        function as library kernels); mpcrl_qlearning_linear_collect; mpcrl_ppo_linear_collect (the linear system's Q-learning and
 *        PPO roll-out steps); mpcrl_env_chain_step; mpcrl_qlearning_chain_collect (the chain of masses as a plant and its Q-learning
 *        roll-out step); mpcrl_ppo_chain_collect; mpcrl_ppo_surrogate_grad_nu / mpcrl_ppo_surrogate_workspace_bytes_nu;
 *        mpcrl_ppo_log_std_apply_nu (PPO on the chain of masses: a diagonal Gaussian over its three controls);
 *        mpcrl_qlearning_td_gn / mpcrl_qlearning_gn_workspace_bytes; mpcrl_qlearning_gn_apply (the Q-learners' Gauss-Newton step);
 *        mpcrl_qlearning_gn_apply_box (that step as a box QP: bounds on theta and a per-entry trust region);
 *        mpcrl_cdpg_record; mpcrl_cdpg_terms / mpcrl_cdpg_workspace_bytes; mpcrl_cdpg_apply (the deterministic policy gradient with a
 *        compatible linear critic, from the roll-out's own du0/dp); mpcrl_debug_seg_reduce (test probe of the small-model
 *        kernels' segmented reductions); mpcrl_query_box_rows (which form of the cartpole solve kernels the handle's bounds select);
 *        mpcrl_debug_model_jets (test probe of the dynamics jets: the discrete map and its derivatives, point by point);
 *        mpcrl_debug_launch_plan (test probe of the launch plan of the small-model solves: a pure host function);
 *        mpcrl_debug_get_order (test probe of the packing order: the permutation and the order kernel's remembered range) */
#define MPCRL_ABI_VERSION 132

enum { MPCRL_MODEL_CARTPOLE = 0, MPCRL_MODEL_LINEAR = 1, MPCRL_MODEL_CHAIN = 2 };
/* how the stage-cost scaling c_k is built (rlmpc/mpc/nlp.py:1044-1055 vs 1083-1091) */
enum { MPCRL_COST_NLS = 0, MPCRL_COST_EXTERNAL = 1 };
/* mpcrl_solve flags */
enum {
    MPCRL_SENS_V = 1,  /* dV/dp (or dQ/dp with u0_fixed)  = dL/dp   nlp.py:1211,1401 */
    MPCRL_SENS_PI = 2, /* du0* / dp                        nlp.py:1413-1424 */
    MPCRL_RTI = 4,     /* one SQP iteration from the stored iterate (build-side mode; the reference always runs full SQP) */
    MPCRL_COLD = 8,    /* ignore the stored iterate: x_k = x0, u = 0, multipliers 0 (MPC.reset, mpc.py:204-210) */
    MPCRL_COLD_DUAL = 16, /* start from the stored x, u, pi but ignore the stored bound multipliers / slacks (the interior point
                            starts from its default point).  Implied for the first solve after mpcrl_set_iterate(bnd = NULL):
                            the reference's `for stage: ocp_solver.set(stage, "x", x0)` initial guess (mpc.py:208-210) */
    MPCRL_NO_BND_STORE = 32, /* ABI 120.  Do not write the bound multipliers / slacks of the solution back into the handle's stored
                            iterate (ten planes of (N+1)(nx+nu) doubles per instance: 3.4 of the 4.7 KB a linear-system solve
                            writes).  x, u, pi are still stored; the planes keep what they held, the NEXT solve behaves as with
                            MPCRL_COLD_DUAL, and mpcrl_get_iterate's bnd describes the last solve that did store them
                            (mpcrl_get_lagrangian stays current).  For callers that start every solve cold (a replay batch, the benchmark) or only ever
                            warm-start the primal iterate.  Honoured by the linear-system solve kernel (lq_solve_kernel); the
                            other kernels ignore it (they store, which is always allowed) */
    MPCRL_EXACT_QP = 64  /* ABI 120, TEST-ONLY, full SQP only (not with MPCRL_RTI, not with MPCRL_LINEAR_SPL=1: MPCRL_E_ARG): every QP of
                            the SQP is solved to the tight interior-point tolerance from a cold interior-point start, fixed
                            fraction to the boundary, no predictor-only steps — what acados + HPIPM do with the reference's
                            options (config/cartpole.yaml:8-14, chain_mass/ocp_utils.py:308-312) and what the oracle's frozen
                            ORACLE_EXACT mode does.  Cartpole: the plain launch shape of a separate kernel instantiation; chain of
                            masses and the linear-system kernel: a wave-uniform switch at the SQP level.  tests/test_gpu_fullsize.py
                            holds the shipped (inexact-SQP) iteration to it at 1e-6 on the benchmark's inputs.  Several times
                            slower: never use it to time */
};
enum { MPCRL_E_ARG = -1, MPCRL_E_MODEL = -2, MPCRL_E_HIP = -3, MPCRL_E_NOMEM = -4 };

#define MPCRL_NO_BOUND 1e30 /* |bound| >= 1e29 means "absent" */

typedef struct {
    int32_t model;     /* MPCRL_MODEL_* */
    int32_t N;         /* horizon */
    int32_t nx, nu;    /* must match the model */
    int32_t np;        /* length of the full parameter vector p (reference order, nlp.py:969-989) */
    int32_t cost_kind; /* MPCRL_COST_* */
    double dT;         /* tf / N  (nlp.py:1163-1164) */
    double gamma;      /* discount factor */
    double h;          /* RK4 sub-step */
    int32_t rk_steps;  /* RK4 steps per shooting interval */
    double tol;        /* NLP residual tolerance (acados default 1e-6; chain 1e-5) */
    int32_t max_iter;  /* SQP iterations (nlp_solver_max_iter) */
    /* box bounds, HOST pointers, stage-vector order v = [u; x] */
    const double *lb0, *ub0; /* nu      : controls at stage 0 */
    const double *lb, *ub;   /* nu + nx : stages 1..N-1 */
    const double *lbe, *ube; /* nx      : stage N */
    const int32_t *soft;     /* nu + nx : 1 = L1-soft bound (idxsbx), may be NULL */
    const double *zl, *zu;   /* nu + nx : L1 weights of soft bounds, may be NULL */
    const double *consts;    /* model constants, HOST pointer (layout: DESIGN.md "model constants") */
    int32_t n_consts;
} MpcrlProblemSpec;

typedef struct MpcrlSolver *mpcrl_handle;

/* Creates a solver for `batch` independent OCP instances on HIP device `device`.  Copies the spec. */
int mpcrl_create(const MpcrlProblemSpec *spec, int batch, int device, mpcrl_handle *out);
int mpcrl_destroy(mpcrl_handle h);

/* theta: device pointer to np doubles (per_instance = 0, shared) or batch*np (per_instance = 1). */
int mpcrl_set_theta(mpcrl_handle h, const double *theta, int n_theta, int per_instance, void *stream);
int mpcrl_set_gamma(mpcrl_handle h, double gamma);
int mpcrl_set_options(mpcrl_handle h, double tol, int max_iter);

/* Opt-in divergence exit (not a reference behaviour: the reference runs full-step SQP without globalisation until
 * nlp_solver_max_iter, config/cartpole.yaml:12-14, rlmpc/mpc/common/mpc.py:42,81-83 — one instance at a time, where a diverging
 * solve costs only itself; in a batch the instances of a wavefront run in lock step and ONE diverging instance keeps its
 * wavefront iterating to max_iter).  Every `window` SQP iterations of an instance the best NLP residual seen so far must have
 * dropped below `factor` times its value at the previous check, else the instance ends with status 2 (as at max_iter) and its
 * lanes are free.  window = 0 (default): off.  1 <= window <= 255, 0 < factor <= 1.  Instances that converge with the rule on
 * return bit for bit what they return with it off.  All three model families (the chain of masses since ABI 110: there an instance
 * has a wavefront — a SIMD — to itself, and a diverging one holds it to max_iter). */
int mpcrl_set_exit_rule(mpcrl_handle h, int window, double factor);

/* Scheduling hint (no effect on results): perm[B] int32 on the device, a permutation of 0..B-1 — slot i of a launch works on
 * instance perm[i], so that instances expected to need similar iteration counts share a wavefront. NULL = identity. */
int mpcrl_set_order(mpcrl_handle h, const int32_t *perm, void *stream);
/* Builds that permutation on the device from the initial states themselves (x0: [B, nx] device): the batch ordered along the
 * coordinate of x0 with the largest spread.  One small kernel; batch <= 8192, else MPCRL_E_ARG (use mpcrl_set_order).  A no-op that
 * clears the order where every instance has a wavefront to itself (chain of masses; horizons of more than 31 stages). */
int mpcrl_auto_order(mpcrl_handle h, const double *x0, void *stream);
/* 1 if an mpcrl_solve with these flags would use the time-sliced launch (whose wavefronts take one instance from each quarter of the
 * batch: a packing order buys nothing there and the caller can skip building one), 0 if not, < 0 on misuse.  stream = the stream the
 * solve will be launched on: while it is being captured into a graph the answer is the shape such a launch takes (the one preferred
 * so far — nothing is timed inside a capture), not the shape of a probe call. */
int mpcrl_query_time_sliced(mpcrl_handle h, int flags, void *stream);
/* Launch shape of the cartpole / linear-system solve kernel for non-RTI solves (no effect on results: the two shapes return the same
 * bits).  mode 0 (default) = automatic: where the batch size makes the time-sliced shape a candidate (it saves a round of wavefronts
 * on the device's SIMDs) the handle times the two shapes against each other on the caller's own batches — calls 1 and 2 of every 64
 * are the probes, read back without waiting; cold calls and warm calls (stored iterates) are timed separately — and uses the plain
 * one where its kernel is more than 20 % faster: time-sliced on batches of one difficulty, plain on batches whose instances need very
 * different iteration counts (replay samples).  Inside a stream capture nothing is timed and the graph gets the shape preferred so
 * far.  mode 1 = time-sliced whenever legal, mode -1 = never (what the environment variable MPCRL_TIME_SLICE=1|0 sets at creation). */
int mpcrl_set_launch_mode(mpcrl_handle h, int mode);
/* The tuner's last probe times in ms (-1 = not measured yet) for cold (warm = 0) or warm (warm = 1) calls; returns 0 if it currently
 * prefers the time-sliced shape, 1 if the plain one, < 0 on misuse.  Never waits for the device. */
int mpcrl_get_launch_times(mpcrl_handle h, int warm, double *sliced_ms, double *plain_ms);

/* Box bounds after creation — ocp_solver.constraints_set(stage, "lbu"|"ubu"|"lbx"|"ubx", v) (rlmpc/mpc/common/mpc.py:72-73,87-88).
 * HOST pointers, stage-vector order v = [u; x]; |bound| >= 1e29 = absent.  which: U0 = controls of stage 0 (nu values),
 * STAGE = stages 1..N-1 (nu + nx; a coordinate created as a soft bound must keep both sides), TERMINAL = stage N (nx).
 * The pin lbu_0 = ubu_0 = u0 of Q(s,a) is the u0_fixed argument of mpcrl_solve (per instance), not this call. */
enum { MPCRL_BOUNDS_U0 = 0, MPCRL_BOUNDS_STAGE = 1, MPCRL_BOUNDS_TERMINAL = 2 };
int mpcrl_set_bounds(mpcrl_handle h, int which, const double *lb, const double *ub);
/* 1 if the handle's solves run the cartpole solve kernels that have the full-box bound pattern compiled in, 0 if the generic ones,
 * < 0 on misuse.  No effect on results: the two forms return the same bits.  The pattern: cartpole model, every bound of the interior
 * stages present (|b| < 1e29), the bounds of u_0 bitwise equal to the interior control bounds and the terminal bounds bitwise equal to
 * the interior state bounds — evaluated at mpcrl_create and again by every mpcrl_set_bounds.  Environment MPCRL_GENERIC_ROWS=1 read at
 * mpcrl_create keeps the generic kernels whatever the bounds are. */
int mpcrl_query_box_rows(mpcrl_handle h);

/* Cold iterate: x_k := x0 for all k (x0: [B, nx] device, or NULL: 0), u := 0, all multipliers 0, slacks 1; the next solve
 * starts cold (interior point from its default point). */
int mpcrl_reset(mpcrl_handle h, const double *x0, void *stream);

/* Per-instance MPCRL_COLD for the NEXT mpcrl_solve only: mask [B] int32 on the device, non-zero = that instance ignores its stored
 * iterate and starts from x_k = x0, u = 0, multipliers 0 (the reference's per-environment `mpc.reset(obs)` when an episode ends,
 * scripts/cartpole_mpc_as_td3_agent_closed_loop.py:62-64, for a batch in which only some environments ended).  NULL clears it. */
int mpcrl_set_cold_mask(mpcrl_handle h, const int32_t *mask, void *stream);

/* Solves all instances.
 *   x0        [B, nx]            initial states
 *   u0_fixed  [B, nu] or NULL    NULL: policy / V mode; else Q(s,a) mode (lbu_0 = ubu_0 = u0)
 *   u0_out    [B, nu]            u_0*
 *   V         [B]                optimal cost (V or Q)
 *   dV_dp     [B, np] or NULL    needs MPCRL_SENS_V
 *   dpi_dp    [B, nu, np] or NULL needs MPCRL_SENS_PI
 *   status    [B] int32          0 success, 1 NaN (a residual or the cost is not finite, e.g. a NaN in x0), 2 max-iter, 4 QP failure
 * The sensitivity rows are written in full by every call: zeros for the entries of p without a gradient, for instances whose
 * status is neither 0 nor 2, and for du0* / dp in Q mode; NaN where the exact-Hessian KKT matrix is not positive definite.
 *   iters     [B, 2] int32 or NULL   SQP iterations, total interior-point iterations
 */
int mpcrl_solve(mpcrl_handle h, const double *x0, const double *u0_fixed, int flags, double *u0_out, double *V,
                double *dV_dp, double *dpi_dp, int32_t *status, int32_t *iters, void *stream);

/* Iterate access (device arrays; any may be NULL).
 *   x [B, N+1, nx]; u [B, N, nu]; pi [B, N, nx] (pi[k] multiplies F(x_k,u_k) - x_{k+1}, nlp.py:827,1180)
 *   bnd [B, 10, N+1, nu+nx]: lam_l, lam_u, t_l, t_u, s_l, s_u, lam_sl, lam_su, t_sl, t_su
 *   res [B, 4]: stationarity, equality, inequality, complementarity residual of the last solve */
int mpcrl_get_iterate(mpcrl_handle h, double *x, double *u, double *pi, double *bnd, double *res, void *stream);
int mpcrl_set_iterate(mpcrl_handle h, const double *x, const double *u, const double *pi, const double *bnd, void *stream);
/* ABI 120.  The same moves with a ROW INDEX, for tables of iterates that hold more (or other) rows than the handle has instances —
 * a replay buffer that keeps, next to every transition, the iterate the roll-out policy's solve ended with (mpc4rl_amd/td3.py,
 * replay_iterates; the reference's SB3 loop keeps ONE solver and warm-starts every replay solve from the previous, unrelated sample:
 * rlmpc/td3/policies.py:186-213).  x [rows, (N+1) nx], u [rows, N nu], pi [rows, N nx], bnd [rows, 10 (N+1)(nu+nx)] device;
 * index [B] int64 device (NULL = identity).  get: table row index[i] := stored iterate of instance i (NULL arrays are skipped).
 * set: stored iterate of instance i := table row index[i]; bnd = NULL as in mpcrl_set_iterate (next solve: MPCRL_COLD_DUAL).
 * index[i] < 0: instance i is skipped (get: nothing written for it; set: it keeps its stored iterate — with bnd = NULL every
 * instance's bound planes are reset, skipped or not).  One launch each, no host synchronisation: capture-safe. */
int mpcrl_get_iterate_rows(mpcrl_handle h, double *x, double *u, double *pi, double *bnd, const int64_t *index, void *stream);
int mpcrl_set_iterate_rows(mpcrl_handle h, const double *x, const double *u, const double *pi, const double *bnd, const int64_t *index, void *stream);
/* L [B] device: the Lagrangian of the mirror NLP at the iterate the last solve returned, L = cost + pi'g + lam'h
 * (nlp.L, rlmpc/mpc/nlp.py:1180,1390; MPC.get_L, rlmpc/mpc/common/mpc.py:325-332). */
int mpcrl_get_lagrangian(mpcrl_handle h, double *L, void *stream);

/* K5, the local half of the one collective on the path: out[j] = sum_i weight[i] * grad[i*ld + j] (j < n), out[n] = sum_i weight[i],
 * out[n+1] = rows.  Replaces the per-sample Python accumulation of rlmpc/examples/linear_system_mpc_qlearning.py:203
 * (np.mean(np.vstack([LR * td[i] * dQ_dp[i, :] ...]))); the n+2 doubles are then all-reduced over the ranks (RCCL).
 * Device pointers; weight may be NULL (= 1).  No handle: the launch goes to the device that owns `out` (hipPointerGetAttributes),
 * whatever device is current in the calling thread, which is restored on return; MPCRL_E_ARG if `out` is not device memory. */
int mpcrl_weighted_grad_sum(const double *grad, int64_t ld, const double *weight, int rows, int n, double *out, void *stream);

/* K4, the batched cartpole swing-up environment (rlmpc/gym/continuous_cartpole/environment.py): B environments, one launch per call.
 *   par [9] HOST: gravity, masscart, masspole, length, force_mag, tau, x_threshold, theta_threshold, max_episode_steps
 *   state [B, 4], steps [B] int64: the environments (device, updated in place)
 * step  — action [B] in [-1, 1]: explicit Euler step (environment.py:105-134), obs [B, 4] (may be NULL) = new state, reward [B] =
 *         x^2 + theta^2 of the new state (:193-194), terminated [B] uint8 = the terminal box (:136-146), truncated [B] uint8 =
 *         steps >= max_episode_steps (gymnasium TimeLimit).
 * reset — environments with mask[i] != 0 (mask NULL: all) restart at (0, 0, (0.9 + 0.2 u01[i]) pi, 0) (:178-180), steps = 0;
 *         u01 [B] uniform [0, 1) numbers drawn by the caller; obs [B, 4] (may be NULL) = the state of EVERY environment after it.
 * obs_f32 != 0: obs is float (what the reference's gymnasium environments return, environment.py:166,186), else double; the state
 * is always double (the reference's numpy state).  No handle: the three environment calls launch on the device that owns `state`
 * (hipPointerGetAttributes), whatever device is current in the calling thread; device or managed memory (hipMalloc / hipMallocManaged),
 * MPCRL_E_ARG for anything else (host-registered or unknown pointers). */
int mpcrl_env_cartpole_step(const double *par, int B, double *state, int64_t *steps, const double *action, void *obs, int obs_f32,
                            double *reward, uint8_t *terminated, uint8_t *truncated, void *stream);
int mpcrl_env_cartpole_reset(int B, double *state, int64_t *steps, const uint8_t *mask, const double *u01, void *obs, int obs_f32,
                             void *stream);
/* The linear-system environment (rlmpc/gym/linear_system/environment.py:28-58), B environments in one launch:
 *   par [12] HOST: A (row-major 2x2), B (2), lb_noise, ub_noise, min_observation (2), max_observation (2)
 *   state [B, 2] (device, updated in place): s+ = A s + B a + [lb_noise + (ub_noise - lb_noise) u01, 0]; action [B]; u01 [B] uniform
 *   numbers of the caller; obs [B, 2] (may be NULL) = new state; cost [B] = 1/2 s's + 1/2 a'a + 100 per violated side of the box. */
int mpcrl_env_linear_step(const double *par, int B, double *state, const double *action, const double *u01, void *obs, int obs_f32,
                          double *cost, void *stream);

/* ABI 120.  The actor's output stage for a batch, one launch: what Actor.forward (rlmpc/td3/policies.py:186-213) and MPC.scale_action
 * (rlmpc/mpc/common/mpc.py:290-301) do per observation, plus TD3's exploration / target-policy noise.  All device pointers:
 *   u0 [B, nu] (mpcrl_solve's output), status [B]; noise [B, nu] float standard-normal draws of the caller or NULL; lo, hi [nu] = lbu, ubu;
 *   ok_i = status_i == 0 (accept_status2: or == 2) and u0_i finite;  a_i = ok_i ? 2 (u0_i - lo) / (hi - lo) - 1 : 0   (scale = 0: u0_i);
 *   noise given: a_i = clip(a_i + clip(sigma noise_i, +-noise_clip), -1, 1)   (noise_clip <= 0: the noise is not clipped);
 *   action [B, nu] float; ok [B] uint8, may be NULL.  Handle-less like the environment kernels (launched on the device that owns `action`). */
int mpcrl_policy_action(const double *u0, const int32_t *status, const float *noise, const double *lo, const double *hi, int B, int nu, int scale,
                        double sigma, double noise_clip, int accept_status2, float *action, uint8_t *ok, void *stream);

/* ABI 130.  The critic side of one TD3 update, two launches (critic_kernel.hpp): what stable_baselines3's TD3.train (the reference's
 * learner, pyproject.toml:10, around the critics of rlmpc/td3/policies.py:47-122) does between the target actor's action and the critic
 * optimiser's step.  Critics: n_critics (1 or 2) MLPs [obs | action] -> 64 -> 64 -> 1 with ReLU, float; `params` / `params_target` hold them
 * back to back in torch's parameter order, each W1 [64][nx + nu] | b1 [64] | W2 [64][64] | b2 [64] | W3 [64] | b3 [1] (row-major
 * [out][in], what nn.Linear.weight is).  All device pointers:
 *   rows [B][row_stride] float: obs (nx) | next obs (nx) | action (nu) | reward | done (the packed replay row), row_stride >= 2 nx + nu + 2;
 *   a_next [B][nu] float: the target policy's action at the next obs;  ok_u [B] uint8 or NULL: 0 = leave the transition out;
 *   ok_b   = ok_u[b] and the 2 nx + nu + 2 entries of the row and a_next[b] are finite;
 *   y_b    = reward + gamma (1 - done) min_c Q'_c(next obs, a_next);   e_cb = ok_b ? Q_c(obs, action) - y_b : 0;
 *   loss   = sum_c sum_b e_cb^2 / max(1, sum_b ok_b)   -> loss_out [1] float (may be NULL);
 *   grad   [n_params] DOUBLE = out_scale * d loss / d params, in the order of `params` (n_params = n_critics (64 (nx + nu) + 4289));
 *   ok_out [B] uint8 or NULL: ok_b.
 *   workspace: mpcrl_critic_workspace_bytes(B, nx, nu, n_critics) bytes of device memory owned by the caller.
 * The partial sums are reduced in a fixed order (no atomics): the same inputs give the same bits.  nx + nu <= 64, hidden width 64 only
 * (MPCRL_E_ARG otherwise).  Handle-less (launched on the device that owns `grad`). */
int64_t mpcrl_critic_workspace_bytes(int B, int nx, int nu, int n_critics);
int mpcrl_critic_td_grad(const float *rows, int row_stride, int B, int nx, int nu, const float *a_next, const uint8_t *ok_u, const float *params,
                         const float *params_target, int n_critics, double gamma, double out_scale, void *workspace, double *grad, float *loss_out,
                         uint8_t *ok_out, void *stream);

/* ABI 130.  dQ_1/da at (obs_b, act_b) for the deterministic policy gradient (autograd of ContinuousCritic.q1_forward,
 * rlmpc/td3/policies.py:68-76), one launch: obs [B][obs_stride] float (first nx entries), act [B][nu] float, ok [B] uint8 or NULL,
 * params: the FIRST critic in the layout above; dq_da [B][nu] float, 0 where ok[b] = 0 or an input is not finite; ok_out [B] uint8 or NULL:
 * 1 where the row was used. */
int mpcrl_critic_dq_da(const float *obs, int obs_stride, int B, int nx, int nu, const float *act, const uint8_t *ok, const float *params,
                       float *dq_da, uint8_t *ok_out, void *stream);

/* ABI 130.  A replay batch in one launch (replay_kernel.hpp): the sampled transitions gathered, their states widened for the two replay
 * solves, and — with iter_ok — the rows of the caller's iterate tables (mpcrl_set_iterate_rows) those solves start from.  Device pointers:
 *   table [cap * E][row_len] float: obs (nx) | next obs (nx) | action | reward | done (last entry), row = step * E + env;
 *   idx [B] int64: the sampled rows (the caller draws them);  pos_t [1] int64: the slot the roll-out writes next;  steps: slots written;
 *   rows [B][row_len] float = table[idx];  obs64 / nxt64 [B][nx] double;
 *   iter_ok [cap * E] uint8 or NULL (then the four outputs below are not written):
 *     row_s = idx;  row_n = the row of the NEXT step of the same environment if that slot is written and is not pos_t, done == 0 and
 *     the obs stored in that row equals this row's next obs entry for entry (float ==; a NaN never does), else idx.  The done column
 *     holds `terminated` only: an episode cut off at its time limit resets the environment with done == 0, and the comparison is what
 *     keeps its solve at next obs from starting at the reset state's iterate.  The next row is read only after the two slot tests
 *     passed (never slot pos_t, never an unwritten slot).
 *     cold_s / cold_n [B] int32 = 1 where iter_ok[row] == 0 (mpcrl_set_cold_mask takes them as they are).
 *   exclude_pos != 0 (a full table only): slot pos_t is being written while the batch is drawn (a roll-out running beside the update):
 *     idx [B] in [0, (cap - 1) E) then counts the rows of the other slots, slot (pos_t + 1 + idx / E) % cap. */
int mpcrl_replay_sample(const float *table, int row_len, int nx, int E, int cap, int steps, const int64_t *idx, int B, const int64_t *pos_t,
                        int exclude_pos, const uint8_t *iter_ok, float *rows, double *obs64, double *nxt64, int64_t *row_s, int32_t *cold_s,
                        int64_t *row_n, int32_t *cold_n, void *stream);

/* ABI 130.  The contraction of the deterministic policy gradient, one launch: out[p] = sum_b ok_b sum_u dq_da[b][u] chain_u dpi_dp[b][u][p]
 * (p < n_p), out[n_p] = sum_b ok_b, chain_u = 2 / (hi_u - lo_u) with scale != 0 (the derivative of MPC.scale_action,
 * rlmpc/mpc/common/mpc.py:290-301), else 1.  dq_da [B][nu] float (mpcrl_critic_dq_da), ok [B] uint8 or NULL, dpi_dp [B][nu][n_p] double
 * (mpcrl_solve's output; entries of rows that are left in are read as nan_to_num would), lo / hi [nu] double, out [n_p + 1] double.
 * workspace: mpcrl_dpg_workspace_bytes(B, n_p) bytes of device memory, ZERO before the first call (the call leaves its counter zero);
 * fixed summation order: the same inputs give the same bits.  nu <= 8. */
int64_t mpcrl_dpg_workspace_bytes(int B, int n_p);
int mpcrl_dpg_grad(const float *dq_da, const uint8_t *ok, const double *dpi_dp, int B, int nu, int n_p, const double *lo, const double *hi, int scale,
                   void *workspace, double *out, void *stream);

/* ABI 130.  The roll-out side of one TD3 step after the policy's solve, one launch (td3_kernel.hpp), cartpole environment, nu = 1: the
 * actor's output stage with exploration noise (mpcrl_policy_action with accept_status2), mpcrl_env_cartpole_step, the replay row
 * [obs | next obs | action | reward_scale * reward | terminated] (float, 11 entries) written at slot pos[0] of table [cap][E][11], the flag
 * of the stored iterate (iter_ok[pos][env] = solve converged and u0 finite; may be NULL), the statistics (stats[0..2] += sum of rewards,
 * converged solves, episodes ended), the reset of the environments that ended (mpcrl_env_cartpole_reset with u01), the next observation
 * obs [E][4] double (in: the observation of this solve) and ended [E] int32 (the cold mask of the next solve).  The last workgroup
 * advances pos[0] to (pos + 1) % cap; iter_rows [E] int64 (may be NULL) receives the rows of this step in the caller's iterate tables,
 * pos * E + env (what mpcrl_get_iterate_rows is then called with).
 * par: the nine doubles of mpcrl_env_cartpole_step.  workspace: 16 + 24 * ceil(E / 256) bytes, ZERO before the first call.  The
 * arithmetic is that of the three kernels it stands for (shared device functions): a loop switched to it reproduces its numbers. */
int mpcrl_td3_cartpole_collect(const double *par, int E, double *state, int64_t *steps, const double *u0, const int32_t *status, const float *eps,
                               const double *u01, double lo, double hi, int scale, double sigma, double *obs, int32_t *ended, float *table, int cap,
                               double reward_scale, int64_t *pos, uint8_t *iter_ok, int64_t *iter_rows, double *stats, void *workspace, void *stream);

/* ABI 130 (132: masked entries selected out).  The policy half of a TD3 update after the collective, one launch: msg [n_theta + 1] double
 * = the all-reduced theta-gradient sum and sample count;  step = mask != 0 ? lr * mask * msg / max(1, count) : 0 -> step_out (a masked
 * entry is selected out, never multiplied: a non-finite message there leaves theta alone);  theta += step;  theta_target =
 * (1 - tau) theta_target + tau theta;  crit_target = (1 - tau) crit_target + tau crit (float [n_crit], the flat critic parameters;
 * n_crit may be 0, crit / crit_target then NULL). */
int mpcrl_td3_policy_post(const double *msg, int n_theta, double lr, const double *mask, double tau, double *theta, double *theta_target,
                          double *step_out, const float *crit, float *crit_target, int n_crit, void *stream);

/* ABI 131.  One roll-out step of the batched cartpole Q-learning loop after the policy's solve, one launch (qlearning_kernel.hpp), one lane per
 * environment, nu = 1 — what scripts/cartpole_mpc_qlearning.py:223-234 does per step after mpc.get_action: for an environment that is
 * alive, a = clip(scale_action(u0) + sigma eps, -1, 1) in float (mpcrl_policy_action with accept_status2 and noise_clip 0: a failed solve
 * gives 0 before the noise), the environment step (mpcrl_env_cartpole_step), and its liveness: terminated, or truncated at
 * max_episode_steps, at this step = this row is recorded and the environment is dead from the next one on (it is not stepped again).
 * Row t = row[env] of the episode table, for every environment: S [T][E][4] = s_t (the state BEFORE the step — the reference stores
 * s_{t+1} there, obs = next_obs before replay_buffer.add, lines 229-231; the TD formula means s_t), A [T][E] = unscale_action(a) =
 * 0.5 (hi - lo) (a + 1) + lo, C [T][E] = x^2 + theta^2 of the new state, live [T][E] = 1; a dead environment's row holds its final state,
 * A = C = 0 and live = 0.  row [E] int32 advances by one (a row >= T is not written: the call is then a no-op for that environment);
 * alive [E] uint8 in / out; obs [E][4] double (may be NULL) = the state after the call (the next solve's x0); cold [E] int32 (may be NULL)
 * = 0.  state / steps as mpcrl_env_cartpole_step, par its nine doubles; eps [T][E] float, row t read at step t; lo < hi = lbu, ubu. */
int mpcrl_qlearning_cartpole_collect(const double *par, int E, int T, double *state, int64_t *steps, const double *u0, const int32_t *status,
                                     const float *eps, double lo, double hi, double sigma, double *obs, uint8_t *alive, int32_t *row, int32_t *cold,
                                     double *S, double *A, double *C, uint8_t *live, void *stream);

/* ABI 131.  The TD step of one episode of the cartpole Q-learning loop, one launch (qlearning_kernel.hpp): scripts/cartpole_mpc_qlearning.py
 * lines 255-269 for E environments.  Sample rows i < T - 1 of the learning sweep: Q, V [T-1][E], dQ_dp [T-1][E][n_p], status_q,
 * status_v [T-1][E] (the Q solve with u0 fixed and the V solve); cost, live [T][E] (the collect's table).  Terms j = i E + e, i < T - 2:
 *   valid_j = live[i][e], live[i+1][e], live[i+2][e] (live is a prefix per environment, so this is i + 1 < L_e - 1 with L_e the rows the
 *             environment recorded: the reference's size - 1 samples and td[:-1]) and the four solves of rows i, i + 1 returned 0;
 *   td_j    = (cost_j + gamma V[i+1][e]) - Q_j   -> td [T-2][E] (0 where not valid);  valid [T-2][E] uint8 (may be NULL);
 *   msg [n_p + 2] = [sum_j w_j dQ_dp_j, sum_j w_j, sum_j valid_j] with w_j = valid_j ? lr td_j : 0 — selected, never multiplied by a mask
 *             (Q / V of a failed solve may be NaN); dQ_dp read as nan_to_num does.  The layout of distributed.allreduce_weighted_grad.
 * workspace: mpcrl_qlearning_td_workspace_bytes(T, E, n_p) bytes of device memory, ZERO before the first call (the call leaves it zero).
 * Fixed summation order (no floating-point atomics): the same inputs give the same bits.  T >= 2 (T = 2: no term, msg = 0). */
int64_t mpcrl_qlearning_td_workspace_bytes(int T, int E, int n_p);
int mpcrl_qlearning_td_grad(const double *Q, const double *V, const double *dQ_dp, const int32_t *status_q, const int32_t *status_v, const double *cost,
                            const uint8_t *live, int T, int E, int n_p, double gamma, double lr, void *workspace, double *td, uint8_t *valid, double *msg,
                            void *stream);

/* ABI 131.  After the collective: step_i = mask_i != 0 ? msg_i / max(1, msg[n_theta + 1]) : 0 (mask [n_theta] double, NULL = all), the mean of
 * distributed.mean_update; theta += step; step_out [n_theta] = step (mpc.set_p(mpc.get_p() + np.mean(dp)), script lines 263-269). */
int mpcrl_qlearning_apply(const double *msg, int n_theta, const double *mask, double *theta, double *step_out, void *stream);

/* Added under ABI 132.  The Gauss-Newton (least-squares TD) form of the same step (qlearning_gn_kernel.hpp): over the K learned entries
 * idx of theta, Delta = lr (G/n + damping diag(G/n))^-1 (b/n) with G = sum_j g_j g_j', b = sum_j td_j g_j over the n valid terms and
 * g_j = dQ_dp_j[idx] — covariant under a rescaling of the parameters, so one lr in (0, 1] means the same on every model.
 *
 * mpcrl_qlearning_td_gn, one launch: the inputs, the terms j, valid_j and td_j of mpcrl_qlearning_td_grad (td and valid come out with the
 * same bits), without lr, plus idx [K] int32 on the DEVICE: strictly increasing columns of dQ_dp, 1 <= K <= 64 and K <= n_p (else
 * MPCRL_E_ARG; the entries cannot be checked on the host: one outside [0, n_p) reads as a zero column).  With g_j = nan_to_num(dQ_dp_j[idx])
 *   msg [K (K + 1) / 2 + K + 2] = [ G | b | sum_j valid_j td_j | sum_j valid_j ]
 *     G: the upper triangle packed row-major, G_ac (a <= c) at a K - a (a - 1) / 2 + (c - a):  G_ac = sum_j valid_j g_ja g_jc
 *     b: b_a = sum_j valid_j td_j g_ja at K (K + 1) / 2 + a
 * an invalid term selected out, never multiplied in.  The message is additive over environments and ranks: one all-reduce (sum).
 * workspace: mpcrl_qlearning_gn_workspace_bytes(T, E, K) bytes of device memory, ZERO before the first call (the call leaves it zero).
 * Fixed summation order (blocks of 128 terms in term order on the matrix cores, then the blocks in four slices; no floating-point
 * atomics): the same inputs give the same bits.  T >= 2 (T = 2: no term, msg = 0). */
int64_t mpcrl_qlearning_gn_workspace_bytes(int T, int E, int K);
int mpcrl_qlearning_td_gn(const double *Q, const double *V, const double *dQ_dp, const int32_t *status_q, const int32_t *status_v, const double *cost,
                          const uint8_t *live, int T, int E, int n_p, double gamma, const int32_t *idx, int K, void *workspace, double *td,
                          uint8_t *valid, double *msg, void *stream);

/* Added under ABI 132.  After the collective, one launch of one workgroup: n = max(1, count), Gb = G / n, bb = b / n, d_max = max_a Gb_aa.
 *   count == 0, d_max not finite or d_max == 0:  info = -1, theta untouched, step_out = 0;
 *   H = Gb + damping diag(Gb_aa > 0 ? Gb_aa : 1e-12 d_max)  (Marquardt's scaling: covariant under a diagonal rescaling of the parameters
 *   for any damping; the floor is for an entry no term is sensitive to, whose step is 0), fp64 Cholesky; pivot a not a finite number > 0:
 *   info = a + 1 (1-based), theta untouched, step_out = 0;
 *   else Delta = lr H^-1 bb, theta[idx[a]] += Delta_a, step_out [n_theta] = Delta at idx and 0 elsewhere, info = 0.
 * idx as above (device, [K], an entry outside [0, n_theta) is skipped); info [1] int32 on the device; damping >= 0; K <= n_theta. */
int mpcrl_qlearning_gn_apply(const double *msg, int K, const int32_t *idx, int n_theta, double lr, double damping, double *theta, double *step_out,
                             int32_t *info, void *stream);

/* Added under ABI 132.  The same step inside a box and a per-entry trust region, one launch of one workgroup.  msg, K, idx, n_theta, lr,
 * damping, H, bb and the codes -1 and a + 1 (1-based; H is factored whole first) as mpcrl_qlearning_gn_apply; lr and damping finite.
 *   Delta = argmin 1/2 D' H D - lr bb' D   subject to  l_a <= D_a <= u_a  for the K learned entries a, c = idx[a]:
 *   l_a = max(lo[c] - theta[c], -radius scale[c]),   u_a = min(hi[c] - theta[c], +radius scale[c])
 * lo, hi, scale [n_theta] doubles on the device, read at idx only; lo, hi may be -+inf, radius +inf (no trust region), scale > 0.  A
 * strictly convex box QP, solved exactly by a primal active-set method from clamp(0, l, u) (theta may start outside [lo, hi]: the step
 * moves it back), one fp64 Cholesky of the free block per iteration.  With no bound active this is mpcrl_qlearning_gn_apply's Delta.
 *   info [2] int32 on the device = {code, iterations}.  code 0: theta[c] = min(max(theta[c] + Delta_a, lo[c]), hi[c]), so lo <= theta <= hi
 *   holds exactly; step_out [n_theta] = Delta at idx (an entry on a bound: l_a or u_a bit for bit) and 0 elsewhere; active [K] uint8 on the
 *   device = 0 free, 1 at l_a, 2 at u_a.
 *   code -1 (no usable term), -2 (l_a > u_a for some a, or one of them NaN), -3 (the iteration cap, 8 K + 16: not reached by a problem
 *   the tests know), a + 1 (a pivot of entry a is no finite number > 0):  theta untouched, step_out = 0, active = 0.
 * Fixed order, no atomics: the same inputs give the same bits.  MPCRL_E_ARG: K outside 1..64, K > n_theta, a NULL pointer, lr or damping
 * not finite, damping < 0, radius not > 0 (NaN included). */
int mpcrl_qlearning_gn_apply_box(const double *msg, int K, const int32_t *idx, int n_theta, double lr, double damping, const double *lo, const double *hi,
                                 const double *scale, double radius, double *theta, double *step_out, uint8_t *active /* [K]: 0 free, 1 at l, 2 at u */,
                                 int32_t *info /* [2]: code, iterations */, void *stream);

/* Added under ABI 132.  The deterministic policy gradient with a compatible linear critic (cdpg_kernel.hpp; mpc4rl_amd/policy_gradient.py),
 * from the roll-out solves alone: pi(s_t) = u0, J_t = du0/dp on the K learned entries idx (1 <= K <= 64), V(s_t) the baseline, nu in
 * 1..3 controls.  Handle-less, asynchronous on `stream`, capture-safe; fixed order, no floating-point atomics: the same bits every time.
 * MPCRL_E_ARG on K outside 1..64, nu outside 1..3, T < 2, E < 1 and a NULL required pointer (nothing is written then).
 *
 * mpcrl_cdpg_record, one launch after a roll-out solve and BEFORE the plant's collect launch: for every environment e with
 * 0 <= row[e] < T (the row the collect is about to write; else nothing is written)
 *   Vt[row][e] = V[e], U0[row][e][:] = u0[e][:], St[row][e] = status[e], Jt[row][e][c][a] = du0_dp[e][c][idx[a]]   (exact copies)
 * V [E], u0 [E][nu], du0_dp [E][nu][n_p], status, row [E] int32, idx [K] int32, all on the device; an entry of idx outside [0, n_p)
 * reads as a zero column.  Vt [T][E], U0 [T][E][nu], St [T][E] int32, Jt [T][E][nu][K].
 *
 * mpcrl_cdpg_terms, one launch after the episode: terms j = i E + e, i < T - 2, valid when live[i], live[i+1], live[i+2] (the liveness
 * rule of mpcrl_qlearning_td_grad) and St[i] == 0 == St[i+1].  delta_j = (cost_j + gamma Vt_{j+E}) - Vt_j (three roundings, that order),
 * d_j = act_j - U0_j, psi_ja = sum_c nan_to_num(Jt_jca) d_jc (fp64, no contraction, c in order).  delta [T-2][E] (0 where invalid),
 * valid [T-2][E] uint8 (may be NULL) and
 *   msg [K (K + 1) + K + 2] = [ G | b | M | sum_j delta_j | count ]      over the valid terms, an invalid one selected out
 *     G_ac = sum_j psi_ja psi_jc,  M_ac = sum_j sum_c' J_jc'a J_jc'c:  upper triangles packed row-major as in mpcrl_qlearning_td_gn
 *     (G at 0, M at K (K + 1) / 2 + K);  b_a = sum_j delta_j psi_ja at K (K + 1) / 2 + a.
 * Additive over environments and ranks: one all-reduce (sum).  act [T][E][nu], cost [T][E], live [T][E] uint8: the episode tables.
 * workspace: mpcrl_cdpg_workspace_bytes(T, E, K) bytes of device memory, ZERO before the first call (the call leaves it zero).
 * T = 2: no term, msg = 0.
 *
 * mpcrl_cdpg_apply, after the collective, one launch of one workgroup: n, H = G/n + damping diag(..), the Cholesky solve and the codes -1
 * and a + 1 exactly as mpcrl_qlearning_gn_apply;  w = H^-1 (b/n);  Delta = -lr w (natural != 0) or -lr (M/n) w, then clipped entrywise
 * (a clip, not a QP) to [max(lo[c] - theta[c], -radius scale[c]), min(hi[c] - theta[c], +radius scale[c])], c = idx[a].  lo, hi, scale
 * [n_theta] on the device may each be NULL (-inf, +inf, 1); all NULL with radius = +inf: no clip.  An empty interval or a NaN bound:
 * info = -2.  On every code but 0 theta is untouched and step_out, w_out, active are 0.  Code 0: theta[c] = min(max(theta[c] + Delta_a,
 * lo[c]), hi[c]), step_out [n_theta] = Delta at idx (a clipped entry: its bound bit for bit) and 0 elsewhere, w_out [K] = w, active [K]
 * uint8 = 0 inside, 1 clipped to the lower end, 2 to the upper.  info [1] int32 on the device.  Also MPCRL_E_ARG: K > n_theta, lr or
 * damping not finite, damping < 0, radius not > 0. */
int mpcrl_cdpg_record(const double *V, const double *u0, const double *du0_dp, const int32_t *status, const int32_t *row, const int32_t *idx, int E, int T,
                      int nu, int n_p, int K, double *Vt, double *U0, int32_t *St, double *Jt, void *stream);
int64_t mpcrl_cdpg_workspace_bytes(int T, int E, int K);
int mpcrl_cdpg_terms(const double *Vt, const double *U0, const double *Jt, const int32_t *St, const double *act, const double *cost, const uint8_t *live,
                     int T, int E, int nu, int K, double gamma, void *workspace, double *delta, uint8_t *valid, double *msg, void *stream);
int mpcrl_cdpg_apply(const double *msg, int K, const int32_t *idx, int n_theta, double lr, double damping, int natural, const double *lo, const double *hi,
                     const double *scale, double radius, double *theta, double *step_out, double *w_out, uint8_t *active, int32_t *info, void *stream);

/* Added under ABI 132.  Batched PPO with the MPC as Gaussian actor (ppo_kernel.hpp; mpc4rl_amd/ppo.py), cartpole environment, nu = 1, all
 * arithmetic fp64: a ~ N(mu, sigma^2) with mu = scale_action(u0*) of the solve and sigma = exp(log_std[0]), log_std a DEVICE double the
 * learner steps.  Handle-less; every call launches on the device that owns its first output pointer, is asynchronous on `stream` and
 * capture-safe (no host synchronisation).
 *
 * One roll-out step after the policy's solve, one launch, one lane per environment.  par: the nine doubles of mpcrl_env_cartpole_step;
 * state / steps as there; u0, status [E]: the solve; eps [E] float standard-normal draws, u01 [E] uniform draws (resets), value [E] the
 * critic's V at the observation just solved; lo < hi = lbu, ubu; 0 <= t < T the row written.
 *   ok   = status in {0, 2} and u0 finite (mpcrl_policy_action's accept_status2 rule);   mu = ok ? 2 (u0 - lo) / (hi - lo) - 1 : 0;
 *   a    = mu + sigma eps (unclipped: this is what is stored);   logp = -(a - mu)^2 / (2 sigma^2) - log_std - 1/2 log 2 pi;
 *   the environment is stepped with clip(a, -1, 1) (the arithmetic of mpcrl_env_cartpole_step: the same bits).
 * Row t of the tables [T][E]: OBS ([..][4], the state before the step), ACT, LOGP, VAL = value, REW = reward_scale * reward, NEXT ([..][4],
 * the state after the step BEFORE any reset: the bootstrap value is taken there), TERM, DONE (uint8: terminated; terminated or
 * truncated), OK (uint8).  Environments that are done are then reset as mpcrl_env_cartpole_reset does with u01 (steps = 0);
 * obs [E][4] = the state after that (the next solve's x0), ended [E] int32 = DONE (the cold mask of the next solve). */
int mpcrl_ppo_cartpole_collect(const double *par, int E, int T, int t, double *state, int64_t *steps, const double *u0, const int32_t *status,
                               const float *eps, const double *u01, const double *value, const double *log_std, double lo, double hi,
                               double reward_scale, double *OBS, double *ACT, double *LOGP, double *VAL, double *REW, double *NEXT, uint8_t *TERM,
                               uint8_t *DONE, uint8_t *OK, double *obs, int32_t *ended, void *stream);

/* Added under ABI 132.  Generalised advantage estimates, one launch, one lane per environment, serial over t = T-1 ... 0; all [T][E]:
 *   delta_t = REW_t + gamma (1 - TERM_t) VNEXT_t - VAL_t;   ADV_t = delta_t + gamma lambda (1 - DONE_t) ADV_{t+1}, ADV_T = 0;   RET_t = ADV_t + VAL_t
 * VNEXT = the critic at NEXT.  stable_baselines3's RolloutBuffer.compute_returns_and_advantage with its time-limit bootstrap (gamma
 * V(terminal_obs) added to the reward of a truncated step) written as VNEXT on truncated rows: the same numbers. */
int mpcrl_ppo_gae(const double *REW, const double *VAL, const double *VNEXT, const uint8_t *TERM, const uint8_t *DONE, int T, int E, double gamma,
                  double gae_lambda, double *ADV, double *RET, void *stream);

/* Added under ABI 132.  The policy half of one PPO minibatch update, two launches (advantage statistics, then terms).  idx [M] int64: rows
 * of the flattened [n_rows = T E] tables ACT, LOGP, ADV, OK; from the minibatch's re-solve with MPCRL_SENS_PI: u0_new [M], status_new [M],
 * dpi_dp [M][1][n_p].  Per row b, j = idx[b]:
 *   valid_b = 0 <= j < n_rows, OK[j], status_new in {0, 2}, u0_new finite, ACT / LOGP / ADV [j] finite;
 *   A_b  = normalize_adv and more than one valid row ? (ADV[j] - mean) / (std + 1e-8) : ADV[j]   (over the valid rows, unbiased std as torch.std);
 *   mu_b, logp_b as in the roll-out from u0_new;   r_b = exp(logp_b - LOGP[j]);   loss_b = -min(r_b A_b, clip(r_b, 1 - eps, 1 + eps) A_b);
 *   g_mu = -A r (a - mu) / sigma^2,  g_ls = -A r ((a - mu)^2 / sigma^2 - 1), both 0 where the clipped branch is the minimum (A > 0 and
 *   r > 1 + eps, or A < 0 and r < 1 - eps).  An invalid row is selected out, never multiplied by 0; dpi_dp is read as nan_to_num does.
 * msg [n_p + 8]:  [0, n_p) = -lr sum_b g_mu,b 2 / (hi - lo) dpi_dp_b;  [n_p] = -lr (sum_b g_ls,b - ent_coef count) (the entropy bonus adds
 *   -ent_coef to the mean g_ls);  [n_p + 1] = count of valid rows — entries [0, n_p) with this count are the layout mpcrl_qlearning_apply and
 *   distributed.allreduce_weighted_grad use;  [n_p + 2 ...] = sums over the valid rows of loss_b, (r - 1) - log r (approximate KL),
 *   |r - 1| > eps (the clip fraction's count), r, ADV, (ADV - mean)^2.
 * workspace: mpcrl_ppo_surrogate_workspace_bytes(M, n_p) bytes of device memory, ZERO before the first call (the call leaves it zero).
 * Fixed summation order (no floating-point atomics): the same inputs give the same bits. */
int64_t mpcrl_ppo_surrogate_workspace_bytes(int M, int n_p);
int mpcrl_ppo_surrogate_grad(const int64_t *idx, int M, int64_t n_rows, const double *ACT, const double *LOGP, const double *ADV, const uint8_t *OK,
                             const double *u0_new, const int32_t *status_new, const double *dpi_dp, int n_p, const double *log_std, double lo, double hi,
                             double clip_range, double ent_coef, double lr, int normalize_adv, void *workspace, double *msg, void *stream);

/* Added under ABI 132.  After the collective (and next to mpcrl_qlearning_apply, which steps theta from the same message as a masked mean):
 * log_std[0] += msg[n_p] / max(1, msg[n_p + 1]). */
int mpcrl_ppo_log_std_apply(const double *msg, int n_p, double *log_std, void *stream);

/* Added under ABI 132.  PPO's value function (value_kernel.hpp): the MLP MPCActorCriticPolicy builds by default, nx -> 64 -> 64 -> 1 with
 * tanh, float; `params` holds it in torch's parameter order, W1 [64][nx] | b1 [64] | W2 [64][64] | b2 [64] | W3 [64] | b3 [1] (row-major
 * [out][in]: the per-net layout of mpcrl_critic_td_grad), n_params = 64 nx + 4289.  Inputs are PPO's double tables, rounded to float on
 * load; the network is evaluated in float, every sum over rows is accumulated in double in a fixed order.  All device pointers.
 *
 * values[b] = V(obs[b]) for n rows: obs [n][nx] double, values [n] double.  No masking: a non-finite row gives a non-finite value,
 * as the framework path does.  One launch (n = 0: none). */
int mpcrl_value_forward(const double *obs, int64_t n, int nx, const float *params, double *values, void *stream);

/* Added under ABI 132.  One minibatch of the value loss, two launches.  OBS [n_rows][nx] double, RET [n_rows] double (PPO's tables,
 * flattened), idx [M] int64.
 *   valid_b = 0 <= idx[b] < n_rows and the nx entries of OBS[idx[b]] and RET[idx[b]] are finite        (selected out, never multiplied by 0)
 *   e_b     = valid_b ? V(OBS[idx[b]]) - (float)RET[idx[b]] : 0
 *   loss    = vf_coef * sum_b e_b^2 / max(1, sum_b valid_b)                    -> out[n_params]
 *   count   = sum_b valid_b                                                     -> out[n_params + 1]
 *   grad    = out_scale * d loss / d params (double, order of `params`)         -> out[0 .. n_params)
 *   workspace: mpcrl_value_workspace_bytes(M, nx) bytes of device memory owned by the caller; it needs no initialisation, before or
 *   between calls (every entry read is written by the same call).
 * The partial sums are reduced in a fixed order (no atomics, no ticket): the same inputs give the same bits.  1 <= nx <= 16, hidden width
 * 64, tanh only; MPCRL_E_ARG otherwise, and for M < 1, a NULL pointer or a negative n_rows.  Handle-less (launched on the device that owns
 * `out`), capture-safe: no allocation, no host synchronisation. */
int64_t mpcrl_value_workspace_bytes(int M, int nx);
int mpcrl_value_mse_grad(const double *OBS, const double *RET, const int64_t *idx, int M, int64_t n_rows, int nx, const float *params,
                         double vf_coef, double out_scale, void *workspace, double *out, void *stream);

/* Added under ABI 132.  The linear system's learner loops around the solves (linear_loop_kernel.hpp; mpc4rl_amd/qlearning_linear.py,
 * mpc4rl_amd/ppo.py), nu = 1, one lane per environment, all arithmetic fp64.  par: the 12 HOST doubles of mpcrl_env_linear_step, state
 * [E][2] as there; the environment step is that call's arithmetic (a shared device function: the same bits).  Handle-less (launched on the
 * device that owns `state` / `OBS`), asynchronous on `stream`, capture-safe.  E = 0: nothing is launched.
 *
 * One roll-out step of the Q-learning loop after the policy's solve, one launch — rlmpc/examples/linear_system_mpc_qlearning.py:160-172
 * per step after mpc.get_action.  u0, status [E]: the solve; eps [T][E] float standard-normal draws and u01 [T][E] uniform draws (the
 * environment's noise), row r = row[env] of both read; lo < hi = lbu, ubu.
 *   a = status in {0, 2} and u0 finite ? u0 : 0;   sigma > 0: a = clip(a + (double)(float(sigma) eps), lo, hi)   (the float product is
 *   rounded first, then the fp64 sum and the clip; sigma = 0: a is u0 itself — the example explores nothing and scales no action);
 *   the environment is stepped with a and u01.
 * Row r of the episode table: S [T][E][2] = s_r (the state BEFORE the step), A [T][E] = a, C [T][E] = the step's cost.  state is updated in
 * place, obs [E][2] = the new state (the next solve's x0), cold [E] int32 = 0, row [E] int32 advances by one; an environment whose row is
 * outside [0, T) is left alone: nothing is written, nothing is stepped.  The environment never terminates: there is no liveness. */
int mpcrl_qlearning_linear_collect(const double *par, int E, int T, double *state, const double *u0, const int32_t *status, const float *eps,
                                   const double *u01, double lo, double hi, double sigma, double *obs, int32_t *row, int32_t *cold, double *S,
                                   double *A, double *C, void *stream);

/* Added under ABI 132.  One roll-out step of PPO on the linear system after the policy's solve, one launch: mpcrl_ppo_cartpole_collect with
 * this plant.  u0, status, eps [E], value, log_std, lo < hi, reward_scale, 0 <= t < T and the tables' row t as there (OBS, NEXT [T][E][2]);
 * u01 [E]: the environment's noise of this step.  mu, a, logp, OK as there; the environment is stepped with clip(a, -1, 1);
 * REW = reward_scale * cost; TERM = 0 (the plant never terminates); steps [E] int64 is the CALLER's count of steps since the last reset
 * (the environment keeps none): DONE = steps + 1 >= episode_length (>= 1), a truncation, so mpcrl_ppo_gae bootstraps through it from NEXT,
 * the state BEFORE the reset.  A done environment restarts at reset_state (2 HOST doubles, read at the call) with steps = 0; obs [E][2] =
 * the state after that, ended [E] int32 = DONE. */
int mpcrl_ppo_linear_collect(const double *par, int E, int T, int t, double *state, int64_t *steps, const double *u0, const int32_t *status,
                             const float *eps, const double *u01, const double *value, const double *log_std, double lo, double hi,
                             double reward_scale, int64_t episode_length, const double *reset_state, double *OBS, double *ACT, double *LOGP,
                             double *VAL, double *REW, double *NEXT, uint8_t *TERM, uint8_t *DONE, uint8_t *OK, double *obs, int32_t *ended,
                             void *stream);

/* Added under ABI 132.  The chain of masses as a plant (chain_env_kernel.hpp; mpc4rl_amd/envs.py BatchedChainMassEnv), B environments in
 * one launch, one lane per environment, all arithmetic fp64: the reference's chain ODE (rlmpc/mpc/chain_mass/ocp_utils.py:76-130)
 * integrated as the model integrates it, rk_steps RK4 steps of Ts / rk_steps (ocp_utils.py:42-56,132), at the environment's OWN parameters.
 * n_mass in 3..7, nx = 3 (2 (n_mass - 2) + 1), M = n_mass - 2 free masses.  p: DEVICE pointer in the OCP's layout (m, D, L, C, Q, R, w;
 * n_p doubles); p_stride = 0: one vector shared by all environments, p_stride = n_p: one row per environment.  x_ss [nx]: DEVICE pointer,
 * the cost's reference state.  state [B][nx] is updated in place; action [B][3] is used as given (the caller clips); wn [B][3 M]:
 * standard-normal draws of the caller, w_std * wn is added to the free masses' accelerations in every ODE evaluation of the step (the
 * ODE is additive in w: this is p's w + noise); wn may be NULL if and only if w_std == 0 (then it is not read).
 *   cost [B] = 1/2 (s - x_ss)' Q (s - x_ss) + 1/2 a' R a  of the state BEFORE the step with the environment's own Q and R: l(s, a), the
 *   quantity the MPC's Q(s, a) models (mpcrl_env_cartpole_step and mpcrl_env_linear_step report the cost of the NEW state).
 * obs [B][nx] (may be NULL) = the new state, float if obs_f32 != 0, else double.  MPCRL_E_ARG: n_mass outside 3..7, rk_steps < 1,
 * Ts <= 0, a p_stride other than 0 or n_p, B < 0, a NULL p, x_ss, state, action or cost, a NULL wn with w_std != 0.  B = 0: nothing is
 * launched.  Handle-less (launched on the device that owns `state`), asynchronous on `stream`, capture-safe. */
int mpcrl_env_chain_step(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, int B, double *state,
                         const double *action, const double *wn, double w_std, void *obs, int obs_f32, double *cost, void *stream);

/* Added under ABI 132.  One roll-out step of the chain's Q-learning loop after the policy's solve, one launch
 * (mpc4rl_amd/qlearning_chain.py): mpcrl_qlearning_linear_collect's shape with three controls.  n_mass ... x_ss, w_std: the plant as in
 * mpcrl_env_chain_step (the environment step is that call's device function: the same bits).  u0 [E][3], status [E]: the solve;
 * eps [T][E][3] float standard-normal draws and wn [T][E][3 M] (NULL iff w_std == 0), row r = row[env] of both read; lo, hi: 3 HOST
 * doubles each (lbu, ubu), lo_j < hi_j.
 *   good = status in {0, 2} and all three u0 finite;   a_j = good ? u0_j : 0;
 *   sigma > 0: a_j = clip(a_j + (double)(float(sigma) eps_j), lo_j, hi_j)   (the float product is rounded first, then the fp64 sum and the
 *   clip; sigma = 0: a is u0 itself, beyond the bounds too; sigma is held as a float, so a positive double that rounds to 0.0f is 0);
 *   the environment is stepped with a and row r of wn.
 * Row r of the episode table: S [T][E][nx] = s_r (the state BEFORE the step), A [T][E][3] = a, C [T][E] = l(s_r, a).  state is updated in
 * place, obs [E][nx] = the new state (the next solve's x0), cold [E] int32 = 0, row [E] int32 advances by one; an environment whose row is
 * outside [0, T) is left alone: nothing is written, nothing is stepped.  The plant never terminates: there is no liveness.
 * MPCRL_E_ARG: the plant's cases, E < 0, T < 1, a NULL pointer, lo_j >= hi_j, a negative or non-finite sigma.  E = 0: nothing is launched. */
int mpcrl_qlearning_chain_collect(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, double w_std, int E,
                                  int T, double *state, const double *u0, const int32_t *status, const float *eps, const double *wn,
                                  const double *lo, const double *hi, double sigma, double *obs, int32_t *row, int32_t *cold, double *S, double *A,
                                  double *C, void *stream);

/* Added under ABI 132.  One roll-out step of PPO on the chain of masses after the policy's solve, one launch (ppo_chain_kernel.hpp;
 * mpc4rl_amd/ppo.py): mpcrl_ppo_linear_collect's shape with the chain as the plant and a diagonal Gaussian over its three controls, one
 * lane per environment, all arithmetic fp64.  n_mass ... x_ss, w_std: the plant as in mpcrl_env_chain_step (the environment step is that
 * call's device function: the same bits); wn [E][3 M]: this step's disturbance draws (NULL iff w_std == 0).  u0 [E][3], status [E]: the
 * solve; eps [E][3] float standard-normal draws; value [E]; log_std [3]: DEVICE doubles, one per control; lo, hi: 3 HOST doubles each
 * (lbu, ubu), lo_j < hi_j; 0 <= t < T the row written.
 *   ok   = status in {0, 2} and all three u0 finite (mpcrl_qlearning_chain_collect's `good`);   mu_j = ok ? 2 (u0_j - lo_j) / (hi_j - lo_j) - 1 : 0;
 *   a_j  = mu_j + exp(log_std_j) eps_j (unclipped: this is what is stored);
 *   logp = sum_j [-(a_j - mu_j)^2 / (2 sigma_j^2) - log_std_j - 1/2 log 2 pi], j = 0, 1, 2 in that order;
 *   the plant is stepped with the PHYSICAL controls lo_j + 0.5 (clip(a_j, -1, 1) + 1) (hi_j - lo_j) (unscale_action) and wn.
 * Row t of the tables [T][E]: OBS ([..][nx], the state before the step), ACT ([..][3]), LOGP, VAL = value, REW = reward_scale * l(s, applied)
 * (mpcrl_env_chain_step's cost: of the state BEFORE the step), NEXT ([..][nx], the state after the step BEFORE any reset), TERM = 0 (the
 * plant never terminates), DONE = steps + 1 >= episode_length (>= 1; steps [E] int64 is the CALLER's count of steps since the last reset),
 * OK.  A done environment restarts at x_reset (nx DEVICE doubles: the OCP's x0) plus vel_std * rn on its 3 M velocity entries (the last
 * 3 M of the state) with steps = 0 — rn [E][3 M]: this step's standard-normal draws, NULL iff vel_std == 0 — which is what
 * BatchedChainMassEnv.reset draws.  obs [E][nx] = the state after that (the next solve's x0), ended [E] int32 = DONE.
 * MPCRL_E_ARG: the plant's cases, E < 0, T < 1, t outside [0, T), episode_length < 1, a NULL pointer, lo_j >= hi_j, a NaN vel_std.  E = 0:
 * nothing is launched.  Handle-less (launched on the device that owns `state`), asynchronous on `stream`, capture-safe. */
int mpcrl_ppo_chain_collect(int n_mass, double Ts, int rk_steps, const double *p, int64_t p_stride, const double *x_ss, double w_std, int E, int T,
                            int t, double *state, int64_t *steps, const double *u0, const int32_t *status, const float *eps, const double *wn,
                            const double *value, const double *log_std, const double *lo, const double *hi, double reward_scale,
                            int64_t episode_length, const double *x_reset, double vel_std, const double *rn, double *OBS, double *ACT, double *LOGP,
                            double *VAL, double *REW, double *NEXT, uint8_t *TERM, uint8_t *DONE, uint8_t *OK, double *obs, int32_t *ended,
                            void *stream);

/* Added under ABI 132.  mpcrl_ppo_surrogate_grad for a diagonal Gaussian over nu controls, 1 <= nu <= 3: ACT [n_rows][nu], u0_new [M][nu],
 * dpi_dp [M][nu][n_p], log_std [nu] DEVICE doubles, lo, hi: nu HOST doubles each, lo_c < hi_c.  A row is valid when all nu entries of
 * u0_new and of ACT are finite (and the rest as there); logp_b is the sum over c = 0 .. nu-1, in that order, of the one-control term;
 *   g_mu,c = -A r (a_c - mu_c) / sigma_c^2,  g_ls,c = -A r ((a_c - mu_c)^2 / sigma_c^2 - 1), all 0 where the clipped branch is the minimum.
 * msg [n_p + 8 + (nu - 1)]: [0, n_p) = -lr sum_b sum_c g_mu,bc 2 / (hi_c - lo_c) nan_to_num(dpi_dp[b][c][.]) — the rows b in order, the
 *   controls c in order inside a row; [n_p, n_p + 8) as in mpcrl_ppo_surrogate_grad with g_ls,0 at [n_p], so mpcrl_qlearning_apply and
 *   the all-reduce read the same layout;  [n_p + 8 + c - 1] = -lr (sum_b g_ls,bc - ent_coef count) for c = 1 .. nu-1.
 * nu = 1 runs the kernel mpcrl_ppo_surrogate_grad runs: the same bits.  workspace: mpcrl_ppo_surrogate_workspace_bytes_nu(M, n_p, nu) bytes,
 * ZERO before the first call (the call leaves it zero).  MPCRL_E_ARG: nu outside 1..3, M < 0 and the cases there.  M = 0: nothing is
 * launched (and the workspace is the 16 bytes of the ticket). */
int64_t mpcrl_ppo_surrogate_workspace_bytes_nu(int M, int n_p, int nu);
int mpcrl_ppo_surrogate_grad_nu(const int64_t *idx, int M, int64_t n_rows, const double *ACT, const double *LOGP, const double *ADV, const uint8_t *OK,
                                const double *u0_new, const int32_t *status_new, const double *dpi_dp, int n_p, int nu, const double *log_std,
                                const double *lo, const double *hi, double clip_range, double ent_coef, double lr, int normalize_adv, void *workspace,
                                double *msg, void *stream);

/* Added under ABI 132.  mpcrl_ppo_log_std_apply for nu entries (1 <= nu <= 3), c = max(1, msg[n_p + 1]):
 * log_std[0] += msg[n_p] / c;  log_std[j] += msg[n_p + 7 + j] / c for j = 1 .. nu-1 (the layout of mpcrl_ppo_surrogate_grad_nu). */
int mpcrl_ppo_log_std_apply_nu(const double *msg, int n_p, int nu, double *log_std, void *stream);

/* Added under ABI 132.  TEST PROBE of the segmented reductions of the cartpole / linear-system kernels (small_kernel.hpp, seg_reduce):
 * one launch of one wavefront.  in, out: device arrays [n_max + n_sum][64] double, the max-values first; lane l of a value belongs
 * to instance slot l / lpi, stage l % lpi, 1 <= lpi <= 64.  Every value is reduced over the lanes of each slot (fmax for the
 * max-values, + for the sum-values, the kernels' tree and operand order) and out holds what each of the 64 lanes ends up with.
 * which: 0 = a reference copy of the tree with every move a __shfl_down / __shfl (it exists in the probe only), 1 = the helpers as
 * the cartpole kernels instantiate them, 2 = as the linear system's.  (n_max, n_sum) is one of (0,1) (1,0) (1,1) (2,2) (1,2) (4,1),
 * the shapes the kernels reduce; anything else: MPCRL_E_ARG. */
int mpcrl_debug_seg_reduce(const double *in, int lpi, int n_max, int n_sum, int which, double *out, void *stream);

/* Added under ABI 132.  TEST PROBE of the dynamics jets of the cartpole / linear-system kernels (jet_probe_kernel.hpp): the discrete map
 * of the model (RK4^rk_steps with step h; the linear system's map is discrete, h and rk_steps are not read) evaluated at n >= 1
 * points, one lane each, with the jets seeded as the kernels seed them.  x [n][nx], u [n][nu], th [n][NTD] (the parameters the
 * dynamics depend on: M, m, l / A column-major, B, b), out [n][row]: device arrays of doubles on one device.  With NW = nu + nx,
 * NLD = 3 directions (cartpole: u, theta, theta_dot; linear system: u, x_0, x_1), NH = NLD (NLD + 1) / 2 (packed lower triangle,
 * (i, j) at i (i + 1) / 2 + j) one row of out is
 *   which 0  Jet1<NLD>, the solve's linearisation:      F[nx], BA[nx][NW] (columns in stage-vector order v = [u; x], all of them)
 *   which 1  JetH<NLD>, the sensitivity pass's:         F, BA, H[nx][NH], hdd[NH] = sum_m aux[m] H[m];    aux = nu [n][nx]
 *   which 2  Jet1<NTD>, dF/dtheta:                      F, Fth[nx][NTD]
 *   which 3  Jet2<NTD>, the mixed second-order pass:    F, e[nx] = dF/dv y, g[nx][NTD] = dF/dtheta, m[nx][NTD] = d2F/dtheta dv y;  aux = y [n][NW]
 *   which 4  out[i] = 1 / x[i] as the jets compute it (jet_rcp), n doubles; model, h, rk_steps, u, th, aux are not read.
 * MPCRL_E_ARG: a null or non-device pointer among those the form reads, n < 1, which outside 0..4, rk_steps outside 1..4 for the
 * cartpole, MPCRL_MODEL_CHAIN (its derivatives do not go through the jets). */
int mpcrl_debug_model_jets(int model, int which, int n, double h, int rk_steps, const double *x, const double *u, const double *th,
                           const double *aux, double *out, void *stream);

/* Added under ABI 132.  TEST PROBE of the launch plan of the cartpole / linear-system solves (csrc/launch_plan.hpp, plan_small): the
 * pure function mpcrl_solve and mpcrl_query_time_sliced decide with, for inputs given as numbers.  No handle, no device, no launch.
 * model: MPCRL_MODEL_CARTPOLE or _LINEAR; N: horizon, 2 .. 63; B >= 1: batch; n_simd >= 1: SIMDs of the device; flags: of mpcrl_solve,
 * COLD already resolved; slice_mode: -1, 0, 1 as mpcrl_set_launch_mode; box_rows: what mpcrl_query_box_rows says; linear_spl: 3, or 1
 * for MPCRL_LINEAR_SPL=1; shape: what the tuner says, 0 = time-sliced, 1 = plain (read only where slice_mode == 0 and out[9], out[10]
 * are both 1).  Anything else: MPCRL_E_ARG.  out:
 *   [0] family: 0 plain (small_solve_kernel), 1 time-sliced (small_solve_sliced_kernel), 2 lq_solve_kernel, 3 the exact-QP instantiation
 *   [1] SHORT form of the segmented reductions   [2] BOX form (families 0, 1)   [3] parked instance in LDS (family 1)   [4] warm
 *   [5], [6] stages per lane and row lanes of lq_solve_kernel (family 2, else 0)
 *   [7] workgroups of the solve launch   [8] workgroups of the separate sensitivity launch, 0 = none
 *   [9] a time-sliced launch is legal   [10] the wave-count rule favours it   [11] 0 (reserved) */
int mpcrl_debug_launch_plan(int model, int N, int B, int n_simd, int flags, int slice_mode, int box_rows, int linear_spl, int shape,
                            int32_t out[12]);

/* Added under ABI 132.  TEST PROBE of the packing order (mpcrl_set_order, mpcrl_auto_order; csrc/order_kernel.hpp): what the next
 * mpcrl_solve of the handle would read.  Returns 1 if that solve would use a packing order, 0 if the identity, < 0 on misuse (a null
 * handle).  perm_out (device, [B] int32, may be NULL): filled with the handle's permutation when the return value is 1, left alone
 * otherwise.  state_out (device, [3] double, may be NULL): {spread, minimum, coordinate} of the batch mpcrl_auto_order last ordered
 * from scratch, {-1, 0, 0} before the first such call.  Both copies are asynchronous on `stream`; nothing in the handle changes. */
int mpcrl_debug_get_order(mpcrl_handle h, int32_t *perm_out, double *state_out, void *stream);

/* Bytes of device memory held by the handle; library version (MPCRL_ABI_VERSION of the header it was built from). */
int64_t mpcrl_workspace_bytes(mpcrl_handle h);
int mpcrl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCRL_H */
