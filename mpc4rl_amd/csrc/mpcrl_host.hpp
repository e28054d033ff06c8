// mpcrl_host.hpp — what the translation units of libmpcrl_hip.so share on the host side: the handle, the error macro, the device
// guards, the workspace layout of the kernels that hand off to their last workgroup, and the table through which mpcrl_api.hip
// reaches the chain-of-masses kernels.  The library is built from one translation unit per chain size (chain_inst.hip,
// -DMPCRL_CHAIN_NMASS=3..7) next to mpcrl_api.hip (the handle's C ABI, cartpole / linear-system solve kernels) and mpcrl_loops.hip
// (the handle-less library kernels of the RL loops), so that they compile in parallel and an edit recompiles its own unit only
// (csrc/Makefile); every unit carries its own device code, nothing is linked on the device side.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/mpcrl.h"
#include "chain_common.hpp"

using mpcrl::LargeArgs;
using mpcrl::LargeSpec;
using mpcrl::SmallSpec;

struct MpcrlSolver {
    int model, B, device, nx, nu, np, N;
    SmallSpec small;
    LargeSpec large;
    bool is_large = false;
    int n_mass = 0;
    double *ws = nullptr, *consts_dev = nullptr;
    int *perm = nullptr, *cold_mask = nullptr;
    bool have_perm = false, have_cold_mask = false;
    double *order_state = nullptr;   // order_kernel.hpp: {spread, minimum, coordinate} of the last from-scratch packing order
    unsigned order_calls = 0;
    size_t ws_stride = 0;
    double *theta = nullptr;   // [np] or [B, np]
    int theta_stride = 0;
    double *X = nullptr, *U = nullptr, *PI = nullptr, *BND = nullptr, *RES = nullptr, *LAG = nullptr;
    int64_t bytes = 0;
    int n_simd = 1024;          // SIMDs of the device (one resident wavefront each for the small solve kernel)
    int slice_mode = 0;         // mpcrl_set_launch_mode / MPCRL_TIME_SLICE: 0 = automatic, 1 = whenever legal, -1 = never
    int linear_spl = 3;         // linear-system model: stages per lane of the solve kernel (3: linear_kernel.hpp; 1: small_solve_kernel)
    bool generic_rows = false;  // MPCRL_GENERIC_ROWS=1 at mpcrl_create: never the BOX instantiations of the cartpole solve kernels
    bool box_rows = false;      // the bounds are the full-box pattern those instantiations compile in (box_rows_spec; mpcrl_set_bounds keeps it current)
    // automatic mode: the two launch shapes of the small solve kernel are timed against each other on the caller's own batches
    // (choose_shape in mpcrl_api.hip; times and call count: launch_plan.hpp): [0] = time-sliced, [1] = plain
    struct Tuner : mpcrl::TunerState {
        hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
        bool pending[2] = {false, false};
    } tune[2];                  // [0] cold calls, [1] warm calls (different work per instance: timed separately)
    int planned = -1;           // what mpcrl_query_time_sliced promised for the next solve (-1: nothing promised)
    bool have_iterate = false;
    bool dual_cold = false;   // the stored bound multipliers are placeholders (set_iterate without bnd): next solve = MPCRL_COLD_DUAL
    // chain (include/mpcrl_chain_ext.h): the workspace still describes the last solve (its linearisation, multipliers and bound rows
    // at the stored iterate) / and also holds that solve's exact Hessians and adjoint solutions (V mode with MPCRL_SENS_PI)
    bool chain_ws_current = false, chain_adjoint_current = false;
};

#define HIP_OK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "mpcrl: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MPCRL_E_HIP;                                                               \
        }                                                                                     \
    } while (0)

// One chain size as mpcrl_api.hip sees it (defined by chain_inst.hip, one per -DMPCRL_CHAIN_NMASS)
struct MpcrlChainEntry {
    int n_mass;
    long np;                                                        // length of the parameter vector (ChainDev<n>::NP)
    size_t (*ws_doubles)(int N);                                    // per-instance workspace (LargeLayout)
    bool (*fits)(int N);                                            // every dynamic-LDS request of the kernels fits one workgroup
    int (*launch)(MpcrlSolver *h, LargeArgs a, hipStream_t st);     // init + SQP (+ sensitivity) launches of one mpcrl_solve
    int (*debug_phases)(unsigned long long *out16, int reset);      // -DMPCRL_PROFILE_PHASES builds: the unit's phase ticks (else null)
    // du0*/dx0 of the last solve (mpcrl_chain_policy_state_sens): the contraction alone, or the adjoint pipeline in front of it
    int (*policy_state_sens)(MpcrlSolver *h, const int32_t *status, double *dpi_dx0, bool adjoint_current, hipStream_t st);
    // trajectory VJP of the last solve (mpcrl_chain_traj_vjp): the adjoint solve for the cotangent and its contractions, the
    // second-order point pass and the exact Hessians in front of them unless that solve left them; g_lb / g_ub (mpcrl_chain_bound_vjp,
    // null for mpcrl_chain_traj_vjp): the bound rows contracted with the same solution, one launch more
    int (*traj_vjp)(MpcrlSolver *h, const int32_t *status, const double *gX, const double *gU, double *g_x0, double *g_theta,
                    double *g_lb, double *g_ub, bool adjoint_current, hipStream_t st);
    // trajectory JVP of the last solve (mpcrl_chain_traj_jvp): per direction the right-hand side and one primal Riccati solve, the
    // second-order point pass and the exact Hessians in front of them unless that solve left them
    int (*traj_jvp)(MpcrlSolver *h, const int32_t *status, int ndir, const double *dx0, const double *dtheta, double *dX, double *dU,
                    bool adjoint_current, hipStream_t st);
};
const MpcrlChainEntry *mpcrl_chain_entry_3(), *mpcrl_chain_entry_4(), *mpcrl_chain_entry_5(), *mpcrl_chain_entry_6(), *mpcrl_chain_entry_7();
// n_mass (3 .. 7, a free integer in the reference: rlmpc/mpc/chain_mass/ocp_utils.py:344-350) -> the translation unit of that chain size
// (the one table: mpcrl_api.hip and mpcrl_state.hip both go through it)
inline const MpcrlChainEntry *chain_entry(int n_mass) {
    switch (n_mass) {
        case 3: return mpcrl_chain_entry_3();
        case 4: return mpcrl_chain_entry_4();
        case 5: return mpcrl_chain_entry_5();
        case 6: return mpcrl_chain_entry_6();
        case 7: return mpcrl_chain_entry_7();
        default: return nullptr;
    }
}

// switches to the handle's device for the duration of a call and restores the caller's device afterwards
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
#define ON_DEVICE(dev)            \
    DeviceGuard guard_((dev));    \
    if (!guard_.ok) return MPCRL_E_HIP

// the handle-less library kernels (reduction, environments) launch on the device that OWNS the memory they are given, whatever device
// is current in the calling thread; -1 if the pointer is not device memory
inline int device_of(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    // device memory, or managed memory (its home device); host-registered / unregistered pointers are refused
    return (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) ? at.device : -1;
}
#define ON_DEVICE_OF(ptr)                       \
    const int dev_of_ = device_of((ptr));       \
    if (dev_of_ < 0) return MPCRL_E_ARG;        \
    ON_DEVICE(dev_of_)

// The workspace of a kernel that hands off to its last workgroup (batch_sum.hpp): the ticket, then one row of `cols` doubles per
// workgroup, a workgroup taking `rows_per_block` of the `rows` terms.
inline int64_t ticket_blocks(int64_t rows, int rows_per_block) { return (rows + rows_per_block - 1) / rows_per_block; }
inline int64_t ticket_workspace_bytes(int64_t rows, int rows_per_block, int cols) {
    return 16 + ticket_blocks(rows, rows_per_block) * cols * (int64_t)sizeof(double);
}
template <class Args>
void set_ticket_workspace(Args &a, void *workspace) {
    a.ticket = (unsigned int *)workspace, a.partial = (double *)((char *)workspace + 16);
}
