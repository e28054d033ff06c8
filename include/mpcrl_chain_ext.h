/* mpcrl_chain_ext.h — du0* / dx0 of the chain of masses, the state sensitivity mpcrl_state_sens (mpcrl_ext.h) does not give there.
 *
 * Versioned on its own (MPCRL_CHAIN_EXT_VERSION, mpcrl_chain_ext_version()).  Handles, error codes, layouts and the rules for streams
 * and devices are those of mpcrl.h.
 *
 * The du0* / dp pass of a chain solve factors the exact-Hessian barrier KKT system at the final iterate and leaves, in the handle's
 * per-instance workspace, the adjoint solutions (y_u, y_nu) of the nu right-hand sides e_iu, the exact stage Hessians and the
 * linearisation [B A]_k.  With x_0 eliminated, x0 enters that system in two places — the control rows of stage 0 through
 * Hex_0[u, x] and dynamics row 0 through A_0 — so
 *     du0* / dx0 [iu][j] = -( sum_c y_u[iu][stage 0, c] Hex_0[u_c, x_j]  +  sum_r y_nu[iu][row 0, r] A_0[r, j] )
 * with the stiffness cap of du0* / dp (the same factorisation).
 */
#ifndef MPCRL_CHAIN_EXT_H
#define MPCRL_CHAIN_EXT_H

#include "mpcrl_ext.h"   /* MPCRL_STATE_Q_MODE */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_CHAIN_EXT_VERSION 1
int mpcrl_chain_ext_version(void);

/* After an mpcrl_solve on this chain handle.  flags: 0, or MPCRL_STATE_Q_MODE when that solve had u0_fixed.  As in mpcrl_state_sens the
 * handle does not remember the mode of its last solve: flags must say it.  With flags = 0 after a Q-mode solve the call answers with
 * the V-mode Jacobian of the Q-mode iterate (u_0 treated as free at the pinned value) and no error.
 *   status  [B]          what that mpcrl_solve wrote (the handle does not keep it; the chain kernels read it).  Required.
 *   dpi_dx0 [B, nu, nx]  du0* / dx0.  Required.
 * Every row is written in full by every call: the values for status 0 or 2, zeros for any other status, NaN where the exact-Hessian
 * KKT matrix is not positive definite (as dpi_dp); with MPCRL_STATE_Q_MODE one memset to zero (u_0 is data), as in mpcrl_state_sens.
 * MPCRL_E_MODEL on a cartpole or linear-system handle; MPCRL_E_ARG for a NULL pointer, unknown flags, or when the workspace no longer
 * describes the handle's last solve: it does from an mpcrl_solve that returned 0 until the next mpcrl_set_iterate,
 * mpcrl_set_iterate_rows, mpcrl_reset, mpcrl_set_theta, mpcrl_set_bounds or mpcrl_set_gamma.
 * One launch when that solve ran MPCRL_SENS_PI in V mode (the adjoint solutions are there), four otherwise (second-order point pass,
 * exact Hessians, adjoint Riccati solve, contraction).  No allocation, no host synchronisation; asynchronous on `stream`, safe to
 * capture.  The outputs of the solve, the stored iterate and the Lagrangian are left as they were. */
int mpcrl_chain_policy_state_sens(mpcrl_handle h, int flags, const int32_t *status, double *dpi_dx0, void *stream);

#ifdef __cplusplus
}
#endif
#endif
