/* mpcrl_bound_ext.h — derivatives of a solve with respect to its box bounds (mpcrl_set_bounds): the backward pass of a differentiable
 * MPC whose constraint data are learned (constraint back-offs), next to x0 and theta.
 *
 * Versioned on its own (MPCRL_BOUND_EXT_VERSION, mpcrl_bound_ext_version()).  Handles, error codes, layouts and the rules for streams
 * and devices are those of mpcrl.h.
 *
 * With z = [w; pi; lam; t], w = (U, X), and R = [grad_w L; g; h + t; lam t - tau] the residual of the barrier KKT system the du0* / dp
 * pass factors, a bound b of side sgn (-1 lower, +1 upper) on coordinate i of the stage vector v_k = [u_k; x_k] enters R only through
 * its own row h + t, h = sgn (v_k[i] - b) [- slack]:  dR/db = -sgn in that row and nothing elsewhere.  Eliminating (lam, t) of that row
 * leaves the right-hand side (lam / t) e_{v_k[i]} on the reduced, symmetric system K of mpcrl_traj_vjp, for either side.  So for a
 * cotangent G = (gX, gU) on the trajectory and y = K^-1 [G; 0] — the ONE adjoint solve of mpcrl_traj_vjp, y_v its primal part —
 *     G' dw* / dlb[k, i] = (lam_l / t_l)[k, i] y_v[k, i]        dV / dlb[k, i] =  lam_l[k, i]
 *     G' dw* / dub[k, i] = (lam_u / t_u)[k, i] y_v[k, i]        dV / dub[k, i] = -lam_u[k, i]
 * (V is the Lagrangian at the KKT point).  An active lower bound gives du_k / dlb_k = 1.  The weight lam / t is the one the solve of
 * y used (capped at the stiffness cap of du0* / dp; on the cartpole each of the two solves of the extrapolation is contracted with its
 * own capped weight and the products are extrapolated).  Soft rows are treated as the du0* / dp pass treats them: their slacks are
 * constants (quirk q1 of the reference's mirror), and dV / dlb = lam_l holds there as well.
 *
 * Layout.  Every bound gradient is [B, N+1, nu+nx] in stage-vector order v = [u; x], the layout of one plane of mpcrl_get_iterate's
 * bnd: one entry per stage and coordinate.  The handle shares a bound over stages (mpcrl_set_bounds: MPCRL_BOUNDS_U0 = the controls
 * of stage 0, MPCRL_BOUNDS_STAGE = stages 1 .. N-1, MPCRL_BOUNDS_TERMINAL = the states of stage N); the caller sums the entries of
 * the stages of a group.  An entry is exactly 0 where no bound row exists: an absent bound (|b| >= 1e29), the state part of stage 0
 * (x_0 = x0: its gradient is g_x0), the control part of stage N, and in Q mode the control part of stage 0 (u_0 is pinned: dQ/du0).
 */
#ifndef MPCRL_BOUND_EXT_H
#define MPCRL_BOUND_EXT_H

#include "mpcrl_ext.h"   /* MPCRL_STATE_Q_MODE */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_BOUND_EXT_VERSION 1
int mpcrl_bound_ext_version(void);

/* After an mpcrl_solve on this handle (every model), from the bound planes it stored:
 *   dV_dlb [B, N+1, nu+nx] or NULL    lam_l   (with MPCRL_STATE_Q_MODE, after a solve with u_0 pinned: dQ / dlb)
 *   dV_dub [B, N+1, nu+nx] or NULL   -lam_u
 * flags: 0 or MPCRL_STATE_Q_MODE (the control part of stage 0 is then zero).  Every requested row is written in full: the values for
 * an instance that holds a solved iterate (the rule of mpcrl_state_sens), zeros otherwise and where no bound row exists.  MPCRL_E_ARG:
 * unknown flags, both outputs NULL, a handle without a stored iterate of a solve, stored bound planes that are placeholders (after
 * MPCRL_NO_BND_STORE or mpcrl_set_iterate without bnd).  One launch, a lane per entry.  No allocation, no host synchronisation, no
 * atomics; asynchronous on `stream`, safe to capture. */
int mpcrl_bound_value_grad(mpcrl_handle h, int flags, double *dV_dlb, double *dV_dub, void *stream);

/* mpcrl_traj_vjp (mpcrl_traj_ext.h) with the bound outputs: cartpole and linear system, V mode, flags must be 0.
 *   g_x0 [B, nx], g_theta [B, np]     as mpcrl_traj_vjp writes them, bit for bit, whether or not the bound outputs are requested
 *   g_lb, g_ub [B, N+1, nu+nx]        sum_k gX[k]' dx_k* / db + gU[k]' du_k* / db per bound row, layout above
 * Any of the four may be NULL, not all of them.  gX [B, N+1, nx] or NULL, gU [B, N, nu] or NULL (NULL = zeros; both NULL:
 * MPCRL_E_ARG).  The refusals, the zero rows (no solved iterate) and the NaN rows (KKT matrix not positive definite) are those of
 * mpcrl_traj_vjp; MPCRL_E_MODEL on a chain handle.  ONE launch and ONE adjoint solve serve all four outputs.  No allocation, no host
 * synchronisation, no atomics; asynchronous on `stream`, safe to capture.  The outputs of the solve, the stored iterate and the
 * Lagrangian are left as they were; the results do not depend on the handle's packing order. */
int mpcrl_bound_vjp(mpcrl_handle h, int flags, const double *gX, const double *gU,
                    double *g_x0, double *g_theta, double *g_lb, double *g_ub, void *stream);

/* mpcrl_chain_traj_vjp (mpcrl_chain_traj_ext.h) with the bound outputs, on a chain handle (MPCRL_E_MODEL on the other two models):
 * its `status` argument (rows with a status other than 0 / 2 are zero), its workspace-freshness rule (MPCRL_E_ARG after a setter that
 * changed the handle's state since the solve) and its refusals.  Any of the four outputs may be NULL, not all of them.  One launch
 * more than mpcrl_chain_traj_vjp when a bound output is requested, none more otherwise; g_x0 and g_theta are the bits of
 * mpcrl_chain_traj_vjp, and what mpcrl_chain_policy_state_sens and mpcrl_chain_traj_vjp return is unchanged by the call. */
int mpcrl_chain_bound_vjp(mpcrl_handle h, int flags, const int32_t *status, const double *gX, const double *gU,
                          double *g_x0, double *g_theta, double *g_lb, double *g_ub, void *stream);

#ifdef __cplusplus
}
#endif
#endif
