/* mpcrl_chain_traj_ext.h — vector-Jacobian product of the whole planned trajectory of a chain-of-masses solve: the backward pass of a
 * differentiable MPC whose loss reads X* = x_0 .. x_N and U* = u_0 .. u_{N-1}, on the model mpcrl_traj_vjp (mpcrl_traj_ext.h) refuses.
 *
 * Versioned on its own (MPCRL_CHAIN_TRAJ_EXT_VERSION, mpcrl_chain_traj_ext_version()).  Handles, error codes, layouts and the rules for
 * streams and devices are those of mpcrl.h.
 *
 * The mathematics is that of mpcrl_traj_ext.h: with w = (U, X) and R the residual of the exact-Hessian barrier KKT system the chain's
 * du0* / dp pass factors (lam / t capped as there),
 *     G' dw* / dtheta = -y' dR/dtheta,   G' dw* / dx0 = -y' dR/dx0 + gX[0],   y = (dR/dz)^-1 [G; 0]
 * for a cotangent G = (gX, gU): one adjoint Riccati solve per instance whatever the horizon, where du0* / dp-style passes would take
 * (N + 1) nx + N nu of them.  x_0 is eliminated: gX[0] enters through the identity term alone, and x0 enters R where
 * mpcrl_chain_policy_state_sens (mpcrl_chain_ext.h) contracts it, Hex_0[u, x] and A_0.
 */
#ifndef MPCRL_CHAIN_TRAJ_EXT_H
#define MPCRL_CHAIN_TRAJ_EXT_H

#include "mpcrl_ext.h"   /* MPCRL_STATE_Q_MODE */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_CHAIN_TRAJ_EXT_VERSION 1
int mpcrl_chain_traj_ext_version(void);

/* After an mpcrl_solve on this chain handle, from the workspace of that solve:
 *   status  [B]                  what that mpcrl_solve wrote (the handle does not keep it; the chain kernels read it).  Required.
 *   gX [B, N+1, nx] or NULL, gU [B, N, nu] or NULL      the cotangents (NULL = zeros; both NULL: MPCRL_E_ARG)
 *   g_x0    [B, nx]  or NULL     sum_k gX[k]' dx_k* / dx0 + gU[k]' du_k* / dx0
 *   g_theta [B, np]  or NULL     the same with respect to theta                     (both NULL: MPCRL_E_ARG)
 * Every requested row is written in full by every call: the values for status 0 or 2, zeros for any other status, NaN where the
 * exact-Hessian KKT matrix is not positive definite (as dpi_dp).  flags must be 0: MPCRL_STATE_Q_MODE (u_0 pinned) is not offered and
 * answers MPCRL_E_ARG, as do unknown flags; with flags = 0 after a Q-mode solve the call treats u_0 as free at the pinned value, as
 * mpcrl_chain_policy_state_sens does.  MPCRL_E_MODEL on a cartpole or linear-system handle; MPCRL_E_ARG for a NULL status, or when
 * the workspace no longer describes the handle's last solve: it does from an mpcrl_solve that returned 0 until the next
 * mpcrl_set_iterate, mpcrl_set_iterate_rows, mpcrl_reset, mpcrl_set_theta, mpcrl_set_bounds or mpcrl_set_gamma.
 * Three launches when that solve ran MPCRL_SENS_PI in V mode (adjoint solve, mixed term, outputs; two without g_theta), two more
 * otherwise (second-order point pass, exact Hessians).  No allocation, no host synchronisation, no atomics; asynchronous on `stream`,
 * safe to capture.  The outputs of the solve, the stored iterate and the Lagrangian are left as they were, and so is what
 * mpcrl_chain_policy_state_sens reads: a call of it before and after this one returns the same bits. */
int mpcrl_chain_traj_vjp(mpcrl_handle h, int flags, const int32_t *status, const double *gX, const double *gU,
                         double *g_x0, double *g_theta, void *stream);

#ifdef __cplusplus
}
#endif
#endif
