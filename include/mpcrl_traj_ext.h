/* mpcrl_traj_ext.h — vector-Jacobian product of the whole planned trajectory of a solve: the backward pass of a differentiable MPC
 * whose loss reads X* = x_0 .. x_N and U* = u_0 .. u_{N-1}, not u_0 alone.
 *
 * Versioned on its own (MPCRL_TRAJ_EXT_VERSION, mpcrl_traj_ext_version()).  Handles, error codes, layouts and the rules for streams
 * and devices are those of mpcrl.h.
 *
 * With w = (U, X) the primal part of the KKT point and R the residual of the exact-Hessian barrier KKT system the du0* / dp pass
 * factors, dw* / dtheta = -(dR/dz)^-1 dR/dtheta restricted to w, and the same with x0.  The matrix is symmetric, so for a cotangent
 * G = (gX, gU) on the trajectory
 *     G' dw* / dtheta = -y' dR/dtheta,   G' dw* / dx0 = -y' dR/dx0 + gX[0],   y = (dR/dz)^-1 [G; 0]
 * (x_0 = x0 is the identity): one adjoint solve per instance whatever the horizon, with the stiffness cap of du0* / dp (the same
 * factorisation), contracted as du0* / dp and du0* / dx0 contract the solution of the right-hand side e_{u_0}.
 */
#ifndef MPCRL_TRAJ_EXT_H
#define MPCRL_TRAJ_EXT_H

#include "mpcrl_ext.h"   /* MPCRL_STATE_Q_MODE */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_TRAJ_EXT_VERSION 1
int mpcrl_traj_ext_version(void);

/* After an mpcrl_solve in V mode on this handle, from the iterate it stored:
 *   g_x0    [B, nx]  or NULL   sum_k G_X[k]' dx_k* / dx0 + G_U[k]' du_k* / dx0
 *   g_theta [B, np]  or NULL   the same with respect to theta (zeros where the model's sensitivity pass has none)
 * gX [B, N+1, nx] or NULL, gU [B, N, nu] or NULL (NULL = zeros; both NULL: MPCRL_E_ARG).
 * Every requested row is written in full by every call: the values for an instance that holds a solved iterate (the rule of
 * mpcrl_state_sens: stored residuals, x, u, pi and dynamics parameters all finite), zeros otherwise, NaN where the exact-Hessian KKT
 * matrix is not positive definite.  flags must be 0: MPCRL_STATE_Q_MODE (u_0 pinned) is not offered and answers MPCRL_E_ARG, as do
 * unknown flags, two NULL outputs, a handle without a stored iterate of a solve and stored bound planes that are placeholders (after
 * MPCRL_NO_BND_STORE or mpcrl_set_iterate without bnd).  MPCRL_E_MODEL on a chain handle.
 * One launch.  No allocation, no host synchronisation, no atomics; asynchronous on `stream`, safe to capture.  The outputs of the
 * solve, the stored iterate and the Lagrangian are left as they were; the results do not depend on the handle's packing order. */
int mpcrl_traj_vjp(mpcrl_handle h, int flags, const double *gX, const double *gU,
                   double *g_x0, double *g_theta, void *stream);

#ifdef __cplusplus
}
#endif
#endif
