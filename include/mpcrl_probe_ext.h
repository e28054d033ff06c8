/* mpcrl_probe_ext.h — TEST PROBES of single phases of the solve kernels, beside mpcrl_debug_seg_reduce of mpcrl.h: each runs one phase
 * of a kernel in one wavefront on a caller's data, in the form the library ships and in a reference copy of an earlier form that exists
 * in the probe's translation unit only (csrc/mpcrl_probe.hip).  Nothing of the library calls them.
 *
 * Versioned on its own (MPCRL_PROBE_EXT_VERSION, mpcrl_probe_ext_version()).  Error codes and the rules for streams and devices are
 * those of mpcrl.h.
 */
#ifndef MPCRL_PROBE_EXT_H
#define MPCRL_PROBE_EXT_H

#include "mpcrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_PROBE_EXT_VERSION 1
int mpcrl_probe_ext_version(void);

/* doubles per stage slot of the matrix-layout sweeps of the cartpole kernels (small_kernel.hpp, SmallSolver::MSLOT) */
#define MPCRL_PROBE_MX_SLOT 66
#define MPCRL_PROBE_MX_PIN 1      /* flags: Q-mode, u_0 pinned (the step of stage 0 leaves K_0 = 0, kff_0 = 0, 1/R_0 = 0, P_0 = Q) */
#define MPCRL_PROBE_MX_WANT_P 2   /* flags: the instantiation that also leaves p_k in the slots */

/* The matrix-core factor sweep of the cartpole kernels (SmallSolver::mx_factor), one launch of one wavefront at horizon N (1 <= N <= 63):
 * min(64 / (N + 1), 4) instances, lane l = stage l % (N + 1) of instance l / (N + 1).
 *   slots_in  [64][MPCRL_PROBE_MX_SLOT]  what the stage lanes publish before a sweep, in the slot layout of small_kernel.hpp: (A, Hxx + D_x)
 *             pairs at 2 (4 r + c); (B[r], Hxu[r]) at 32 + 4 r; (bb[r], g_x[r]) at 34 + 4 r; ([Huu + D_u | g_u | . | .][c], Hxu[c]) at
 *             48 + 2 c.  Entry 48 + 2 * 3 is the probe's: it writes there what the publish of the chosen form writes (which 0: 0.0,
 *             which 1: g_u again), whatever the caller put.
 *   slots_out [64][MPCRL_PROBE_MX_SLOT]  the slots after the sweep: P_k over the second members of the first 16 pairs, p_k[r] at 33 + 4 r
 *             (MPCRL_PROBE_MX_WANT_P), d_k[r] at 35 + 4 r, q_k[r] at 48 + 2 r, K at 56, (1/R, kff, beta) at 60
 *   ok_out    [4]  the flag of each of the four blocks: 1.0 = every pivot positive, 0.0 = one was not (NaN included); -1.0 for a block
 *             without an instance (its lanes shadow block 0 and store nowhere)
 * which: 0 = the sweep as it was before the column-3 copy of p_k, the lane-mask pivot flag and the peeled stage-0 step (a copy that
 * exists in the probe only, with the publish layout of that time), 1 = SmallSolver::mx_factor as the kernels run it.  Anything else,
 * unknown flags, N out of range or a NULL array: MPCRL_E_ARG.  Asynchronous on `stream`. */
int mpcrl_debug_mx_factor(const double *slots_in, int N, int flags, int which, double *slots_out, double *ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
