/* mpcrl_probe_chain_ext.h — TEST PROBE of the affine chains of the cartpole kernels' vector sweeps, beside the factor-sweep probe of
 * mpcrl_probe_ext.h and of the same kind: one phase of a kernel in one wavefront on a caller's data, in the form the library ships and
 * in a reference copy of an earlier form that exists in the probe's translation unit only (csrc/mpcrl_probe.hip).  Nothing of the
 * library calls it.  A header and a version of its own, as every group of exports added beside mpcrl.h has: the
 * table of mpcrl_probe_ext.h stays what its users bound.
 *
 * Versioned on its own (MPCRL_PROBE_CHAIN_EXT_VERSION, mpcrl_probe_chain_ext_version()).  The slot constant MPCRL_PROBE_MX_SLOT, error
 * codes and the rules for streams and devices are those of mpcrl_probe_ext.h and mpcrl.h.
 */
#ifndef MPCRL_PROBE_CHAIN_EXT_H
#define MPCRL_PROBE_CHAIN_EXT_H

#include "mpcrl_probe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCRL_PROBE_CHAIN_EXT_VERSION 1
int mpcrl_probe_chain_ext_version(void);

/* One affine chain of the vector sweeps of the cartpole kernels (SmallSolver::mx_chain) on the closed-loop matrices Acl_k = A_k - B_k K_k,
 * one launch of one wavefront at horizon N (1 <= N <= 63): min(64 / (N + 1), 4) instances, lane l = stage l % (N + 1) of instance
 * l / (N + 1).
 *   slots_in  [64][MPCRL_PROBE_MX_SLOT]  the slots as they stand after a factor sweep and the stage lanes' phase before the chain: A(r,c)
 *             at 2 (4 r + c), B[r] at 32 + 4 r, K[r] at 56 + r, and the chain's additive term at 35 + 4 r: d_k[r] of stages 0 .. N-1
 *             (forward), c_k[r] of stages 0 .. N (backward; c_N is the chain's start p_N)
 *   slots_out [64][MPCRL_PROBE_MX_SLOT]  the slots after the chain.  forward = 1: Dx_{k+1} = Acl_k Dx_k + d_k from Dx_0 = 0, Dx_k[r] at
 *             49 + 2 r of stages 1 .. N.  forward = 0: p_k = Acl_k' p_{k+1} + c_k from p_N = c_N, p_k[r] at 33 + 4 r of stages 0 .. N.
 *             Every other word, and every slot of a lane without a stage, is as it came in.
 * which: 0 = the chain as it was when every operand fetch clamped its stage (a copy that exists in the probe only, with the slot layout it
 * read; the chains have kept that layout, so both forms take the same slots), 1 = SmallSolver::mx_chain as the kernels run it: the
 * last turns of the operand ring peeled, addresses of the loop walking by constants.  Anything else, forward outside {0, 1}, N out of
 * range or a NULL array: MPCRL_E_ARG.  Asynchronous on `stream`. */
int mpcrl_debug_mx_chain(const double *slots_in, int N, int forward, int which, double *slots_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
