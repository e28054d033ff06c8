/* mpcrl_ext.h — extensions of libmpcrl_hip.so that have no counterpart in the reference's MPC surface.
 *
 * include/mpcrl.h is the C ABI of what the reference's `MPC` class offers and is versioned by MPCRL_ABI_VERSION; what goes beyond
 * that surface is declared here and versioned on its own (MPCRL_EXT_VERSION, mpcrl_ext_version()).  Handles, error codes, layouts
 * and the rules for streams and devices are those of mpcrl.h.
 *
 * State sensitivities of a solve.  With l0(x, u) = c_0 l_0(x, u, theta) + pi_1' F(x, u, theta), pi_1 the multiplier of
 * F(x_0, u_0) - x_1 at the stored iterate:
 *     dV/dx0   = grad_x l0(x0, u_0)          (minus the multiplier of x_0 = x0; the same expression gives dQ/dx0 in Q mode)
 *     dQ/du0   = grad_u l0(x0, u0)           (Q mode: the multiplier of the pin lbu_0 = ubu_0 = u0; no bound term enters)
 *     du0* / dx0                             (V mode: rows u_0 of -(dR/dz)^-1 dR/dx0 of the exact-Hessian barrier KKT system — the
 *                                             system the du0* / dp pass solves, same stiffness cap, another right-hand side)
 * Here du0* / dx0 exists for the cartpole and the linear system; the chain of masses has dV/dx0, dQ/dx0 and dQ/du0 from this call and
 * its du0* / dx0 from mpcrl_chain_policy_state_sens (mpcrl_chain_ext.h).
 */
#ifndef MPCRL_EXT_H
#define MPCRL_EXT_H

#include "mpcrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_EXT_VERSION 1
int mpcrl_ext_version(void);

enum { MPCRL_STATE_Q_MODE = 1 };   /* the last solve had u0_fixed: u_0 is data, not a variable */

/* After an mpcrl_solve on this handle, from the iterate it stored (x_0 = x0 and, in Q mode, u_0 = the pin):
 *   dV_dx0  [B, nx]      or NULL   dV/dx0 (V mode) or dQ/dx0 (Q mode)
 *   dQ_du0  [B, nu]      or NULL   Q mode only (else MPCRL_E_ARG)
 *   dpi_dx0 [B, nu, nx]  or NULL   du0* / dx0; written as zeros in Q mode (as dpi_dp is); MPCRL_E_MODEL on a chain handle
 * Every requested row is written in full by every call: the values for an instance that holds a solved iterate, zeros otherwise,
 * NaN in dpi_dx0 where the exact-Hessian KKT matrix is not positive definite.  The handle keeps the iterate and its residuals, not
 * the status word mpcrl_solve wrote into the caller's array: an instance counts as not solved (status 1) when a stored residual,
 * an entry of its stored x, u, pi or a dynamics parameter is not finite.  A caller that wants the rows of status-4 instances
 * zeroed as well selects them out with the status array it holds (MPCBatch.state_sens does).
 * MPCRL_E_ARG without a stored iterate of a solve, or when the stored bound planes are placeholders (after MPCRL_NO_BND_STORE or
 * mpcrl_set_iterate without bnd).  No allocation, no host synchronisation; asynchronous on `stream`, safe to capture. */
int mpcrl_state_sens(mpcrl_handle h, int flags, double *dV_dx0, double *dQ_du0, double *dpi_dx0, void *stream);

#ifdef __cplusplus
}
#endif
#endif
