/* mpcrl_traj_jvp_ext.h — Jacobian-vector product of the whole planned trajectory of a solve: the forward mode of a differentiable
 * MPC.  How X* = x_0 .. x_N and U* = u_0 .. u_{N-1} move when x0 and theta move along a direction; with unit directions, the full
 * Jacobian d(X*, U*) / d(x0, theta) in nx + n_diff directions instead of one mpcrl_traj_vjp per entry of the trajectory.
 *
 * Versioned on its own (MPCRL_TRAJ_JVP_EXT_VERSION, mpcrl_traj_jvp_ext_version()).  Handles, error codes, layouts and the rules for
 * streams and devices are those of mpcrl.h.
 *
 * With w = (U, X) the primal part of the KKT point and R the residual of the exact-Hessian barrier KKT system the du0* / dp pass
 * factors (mpcrl_traj_ext.h: the same matrix, the same stiffness cap, on the cartpole the same extrapolation over it),
 *     dw = -(dR/dz)^-1 (dR/dtheta dtheta + dR/dx0 dx0)   restricted to w,
 * one solve per direction whatever the horizon, with x_0 = x0 eliminated: dX[0] = dx0.  <G, dw> = <g_x0, dx0> + <g_theta, dtheta>
 * with (g_x0, g_theta) of mpcrl_traj_vjp for the cotangent G holds to rounding.
 *
 * Of dtheta only the entries the sensitivity pass differentiates are read (cartpole: m, M, l, entries 0 .. 2; linear system: all
 * 12), the entries g_theta of mpcrl_traj_vjp is non-zero at.  The rest — the cartpole's cost block, entries 3 .. 82 — is ignored.
 *
 * Out of scope: the chain of masses (mpcrl_chain_traj_jvp_ext.h has a call of its own), MPCRL_STATE_Q_MODE (u_0 pinned), directions
 * in the box bounds or in the cartpole's cost block, and the tangent of the multipliers.
 */
#ifndef MPCRL_TRAJ_JVP_EXT_H
#define MPCRL_TRAJ_JVP_EXT_H

#include "mpcrl_ext.h"   /* MPCRL_STATE_Q_MODE */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_TRAJ_JVP_EXT_VERSION 1
int mpcrl_traj_jvp_ext_version(void);

/* After an mpcrl_solve in V mode on this handle, from the iterate it stored, for ndir >= 1 directions per instance:
 *   dX [B, ndir, N+1, nx] or NULL   dx_k* / dx0 dx0 + dx_k* / dtheta dtheta   (row k = 0 is dx0 itself)
 *   dU [B, ndir, N, nu]   or NULL   du_k* / dx0 dx0 + du_k* / dtheta dtheta
 * dx0 [B, ndir, nx] or NULL, dtheta [B, ndir, np] or NULL (NULL = zeros; both NULL: MPCRL_E_ARG); both outputs NULL: MPCRL_E_ARG.
 * Every requested row is written in full by every call: the values for an instance that holds a solved iterate (the rule of
 * mpcrl_state_sens), zeros otherwise, NaN where the exact-Hessian KKT matrix is not positive definite.  flags must be 0:
 * MPCRL_STATE_Q_MODE is not offered and answers MPCRL_E_ARG, as do unknown flags, ndir < 1, a handle without a stored iterate of a
 * solve and stored bound planes that are placeholders (after MPCRL_NO_BND_STORE or mpcrl_set_iterate without bnd).  MPCRL_E_MODEL on
 * a chain handle.
 * One launch: every (instance, direction) pair linearises and factors for itself.  No allocation, no host synchronisation, no
 * atomics; asynchronous on `stream`, safe to capture.  The outputs of the solve, the stored iterate and the Lagrangian are left as
 * they were; the results do not depend on the handle's packing order, nor on ndir or the place of a direction among the others. */
int mpcrl_traj_jvp(mpcrl_handle h, int flags, int ndir, const double *dx0, const double *dtheta,
                   double *dX, double *dU, void *stream);

#ifdef __cplusplus
}
#endif
#endif
