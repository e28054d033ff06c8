/* mpcrl_chain_traj_jvp_ext.h — Jacobian-vector product of the whole planned trajectory of a chain-of-masses solve: the forward mode of
 * a differentiable MPC whose outputs are X* = x_0 .. x_N and U* = u_0 .. u_{N-1}, on the model mpcrl_traj_jvp (mpcrl_traj_jvp_ext.h)
 * refuses.  Columns d(X*, U*) / dtheta_j for Gauss-Newton identification of m, D, L, C from multi-step predictions, or linearised
 * covariance propagation of an uncertain x0 or theta through the plan: a handful of directions where the VJP (mpcrl_chain_traj_ext.h)
 * would take (N + 1) nx + N nu cotangents.
 *
 * Versioned on its own (MPCRL_CHAIN_TRAJ_JVP_EXT_VERSION, mpcrl_chain_traj_jvp_ext_version()).  Handles, error codes, layouts and the
 * rules for streams and devices are those of mpcrl.h.
 *
 * The mathematics is that of mpcrl_traj_jvp_ext.h on the matrix of mpcrl_chain_traj_ext.h: with w = (U, X) and R the residual of the
 * exact-Hessian barrier KKT system the chain's du0* / dp pass factors (lam / t capped as there),
 *     dw = -(dR/dz)^-1 (dR/dtheta dtheta + dR/dx0 dx0)   restricted to w
 * — one PRIMAL Riccati solve per (instance, direction) whatever the horizon, on the transposed right-hand side of the VJP's
 * contraction: <G, dw> of this call equals g_x0 . dx0 + g_theta . dtheta of mpcrl_chain_traj_vjp on the same workspace.  x_0 is
 * eliminated: dX[.., 0, :] is dx0 itself, and dx0 enters R through Hex_0[u, x] and A_0.
 *
 * Out of scope: one factorisation shared by the directions of an instance, directions riding the 16 columns of the matrix cores,
 * Q mode, directions in the bounds, the tangent of the multipliers, forward-mode hooks on the autograd layer.
 */
#ifndef MPCRL_CHAIN_TRAJ_JVP_EXT_H
#define MPCRL_CHAIN_TRAJ_JVP_EXT_H

#include "mpcrl_ext.h"   /* MPCRL_STATE_Q_MODE */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_CHAIN_TRAJ_JVP_EXT_VERSION 1
int mpcrl_chain_traj_jvp_ext_version(void);

/* After an mpcrl_solve on this chain handle, from the workspace of that solve:
 *   status  [B]                  what that mpcrl_solve wrote (the handle does not keep it; the chain kernels read it).  Required.
 *   ndir                         directions per instance, >= 1
 *   dx0 [B, ndir, nx] or NULL, dtheta [B, ndir, np] or NULL      the directions (NULL = zeros; both NULL: MPCRL_E_ARG).  EVERY entry
 *                                of dtheta is read: m, D, L, C, Q, R, w.
 *   dX [B, ndir, N+1, nx] or NULL, dU [B, ndir, N, nu] or NULL   the tangents of the plan (both NULL: MPCRL_E_ARG); dX[.., 0, :] = dx0
 *                                (zeros when dx0 is NULL)
 * Every requested row is written in full by every call: the values for status 0 or 2, zeros for any other status, NaN where the
 * exact-Hessian KKT matrix is not positive definite (as dpi_dp).  flags must be 0: MPCRL_STATE_Q_MODE (u_0 pinned) is not offered and
 * answers MPCRL_E_ARG, as do unknown flags; with flags = 0 after a Q-mode solve the call treats u_0 as free at the pinned value, as
 * mpcrl_chain_traj_vjp does.  MPCRL_E_MODEL on a cartpole or linear-system handle; MPCRL_E_ARG for ndir < 1, a NULL status, or when
 * the workspace no longer describes the handle's last solve: it does from an mpcrl_solve that returned 0 until the next
 * mpcrl_set_iterate, mpcrl_set_iterate_rows, mpcrl_reset, mpcrl_set_theta, mpcrl_set_bounds or mpcrl_set_gamma.
 * Two launches per direction (right-hand side from the point tables, Riccati solve; one without dtheta), two more in front when that
 * solve did not run MPCRL_SENS_PI in V mode (second-order point pass, exact Hessians): the count does not depend on the horizon.  The
 * directions of an instance run in sequence on its workspace; a result does not depend on ndir or on the place of its direction.
 * No allocation, no host synchronisation, no atomics; asynchronous on `stream`, safe to capture.  The outputs of the solve, the
 * stored iterate and the Lagrangian are left as they were, and so are what mpcrl_chain_policy_state_sens and mpcrl_chain_traj_vjp
 * read and what a following warm mpcrl_solve starts from. */
int mpcrl_chain_traj_jvp(mpcrl_handle h, int flags, const int32_t *status, int ndir, const double *dx0, const double *dtheta,
                         double *dX, double *dU, void *stream);

#ifdef __cplusplus
}
#endif
#endif
