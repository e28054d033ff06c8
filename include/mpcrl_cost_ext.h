/* mpcrl_cost_ext.h — derivatives of a cartpole solve with respect to its tracking cost (W_0, W, W_e, yref_0, yref, yref_e: entries
 * 3 .. 82 of the parameter vector p, which mpcrl_set_theta feeds to the solve): the backward pass of a differentiable MPC whose
 * weights and reference are learned, next to x0, the dynamics parameters and the box bounds.
 *
 * Versioned on its own (MPCRL_COST_EXT_VERSION, mpcrl_cost_ext_version()).  Handles, error codes, layouts and the rules for streams
 * and devices are those of mpcrl.h.
 *
 * dV/dp, du0* / dp (mpcrl_solve) and g_theta (mpcrl_traj_vjp, mpcrl_bound_vjp) keep their zero cost block: that is the convention of
 * the reference's mirror, whose NONLINEAR_LS cost is not parameterised.  The gradients here are a separate output that treats EVERY
 * entry of the cost block as an independent variable.
 *
 * Unscaled stage cost l = 1/2 r' W r, r = y - yref, y = [x; u] on stages 0 .. N-1 and y = x on stage N; stage 0 uses (W_0, yref_0),
 * stages 1 .. N-1 use (W, yref), stage N uses (W_e, yref_e).  The solve uses H = 1/2 (W + W'), and c_k is the cost scale of stage k
 * (MPCRL_COST_NLS: dT, and 1 on stage N).  A cost parameter enters the KKT residual only through grad_v l_k = H r, which is linear in
 * (W, yref).  With y = K^-1 [G; 0] the ONE adjoint solve of mpcrl_traj_vjp for a cotangent G = (gX, gU), y_k its primal part on stage
 * k in y order, and the sums over the stages of the block:
 *     dV / dW[a, b]  =  sum_k c_k 1/2 r_a r_b                      G' dw* / dW[a, b]  = -sum_k c_k 1/2 (y_a r_b + y_b r_a)
 *     dV / dyref[a]  = -sum_k c_k (H r)_a                          G' dw* / dyref[a]  = +sum_k c_k (H y)_a
 * (V is the Lagrangian at the KKT point; the same expressions hold at the stored iterate of a solve with u_0 pinned, for Q).  Where
 * the cartpole pass extrapolates over the stiffness cap, 2 y(W) - y(W / 2), the contraction takes the merged y: it is linear in y.
 *
 * Layout.  dV_dcost and g_cost are [B, np], np = 83, in the layout of p, each field column-major: W_0 (5x5) at 3, W (5x5) at 28,
 * W_e (4x4) at 53, yref_0 (5) at 69, yref (5) at 74, yref_e (4) at 79.  Entries 0 .. 2, the dynamics block, are exactly 0, so the
 * caller adds g_theta + g_cost.  The entries W[a, b] and W[b, a] hold the same bits.
 */
#ifndef MPCRL_COST_EXT_H
#define MPCRL_COST_EXT_H

#include "mpcrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_COST_EXT_VERSION 1
int mpcrl_cost_ext_version(void);

/* After an mpcrl_solve on a cartpole handle, with or without u_0 pinned (then: dQ / dcost), from the iterate it stored:
 *   dV_dcost [B, np]     formulas and layout above
 * flags must be 0.  Every row is written in full: the values for an instance that holds a solved iterate (the rule of
 * mpcrl_state_sens), zeros otherwise.  MPCRL_E_ARG: flags other than 0, dV_dcost NULL, a handle without a stored iterate of a solve.
 * MPCRL_E_MODEL on the linear system (its weights are in `consts`) and the chain (its Q, R are in dV/dp).  One launch.  No
 * allocation, no host synchronisation, no atomics; asynchronous on `stream`, safe to capture.  The stored iterate, the outputs of
 * the solve and the workspace are left as they were. */
int mpcrl_cost_value_grad(mpcrl_handle h, int flags, double *dV_dcost, void *stream);

/* mpcrl_bound_vjp (mpcrl_bound_ext.h) with one more output, on a cartpole handle: V mode, flags must be 0.
 *   g_x0 [B, nx], g_theta [B, np], g_lb, g_ub [B, N+1, nu+nx]    as mpcrl_bound_vjp writes them, bit for bit, whether or not g_cost
 *                                                                 is requested
 *   g_cost [B, np]                                                sum_k gX[k]' dx_k* / dcost + gU[k]' du_k* / dcost, layout above
 * Any of the five may be NULL, not all of them.  gX [B, N+1, nx] or NULL, gU [B, N, nu] or NULL (NULL = zeros; both NULL:
 * MPCRL_E_ARG).  The refusals, the zero rows (no solved iterate) and the NaN rows (KKT matrix not positive definite; entries 0 .. 2
 * of g_cost stay 0) are those of mpcrl_traj_vjp; MPCRL_E_MODEL on the linear system and the chain.  ONE launch and ONE adjoint solve
 * serve all five outputs.  No allocation, no host synchronisation, no atomics; asynchronous on `stream`, safe to capture.  The
 * outputs of the solve, the stored iterate and the Lagrangian are left as they were; the results do not depend on the handle's
 * packing order. */
int mpcrl_cost_vjp(mpcrl_handle h, int flags, const double *gX, const double *gU,
                   double *g_x0, double *g_theta, double *g_lb, double *g_ub, double *g_cost, void *stream);

#ifdef __cplusplus
}
#endif
#endif
