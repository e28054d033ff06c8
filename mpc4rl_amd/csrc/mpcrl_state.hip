// mpcrl_state.hip — include/mpcrl_ext.h: state sensitivities of a solve (dV/dx0, dQ/du0, du0*/dx0) from the iterate the handle
// stores; include/mpcrl_chain_ext.h and include/mpcrl_chain_traj_ext.h: du0*/dx0 and the trajectory VJP of the chain, from the workspace
// of its last solve (kernels and launches: chain_sens.hpp, chain_inst.hip); include/mpcrl_bound_ext.h: the derivatives with respect to
// the box bounds (bound_vjp_kernel.hpp, and the chain's launcher with its bound outputs); include/mpcrl_cost_ext.h: the derivatives with
// respect to the cartpole's tracking cost (cost_vjp_kernel.hpp); include/mpcrl_traj_jvp_ext.h: the trajectory JVP (traj_jvp_kernel.hpp);
// include/mpcrl_chain_traj_jvp_ext.h: the chain's (chain_sens.hpp, chain_inst.hip).  The kernels are state_sens_kernel.hpp; this unit instantiates them for the cartpole, the linear system and every chain
// size, and launches them.  Nothing here allocates or waits: two launches (or one and a memset) on the caller's stream.
#include "mpcrl_host.hpp"

#include "../../include/mpcrl_chain_ext.h"
#include "../../include/mpcrl_chain_traj_ext.h"
#include "../../include/mpcrl_bound_ext.h"
#include "../../include/mpcrl_cost_ext.h"
#include "../../include/mpcrl_traj_ext.h"
#include "../../include/mpcrl_traj_jvp_ext.h"
#include "../../include/mpcrl_chain_traj_jvp_ext.h"
#include "state_sens_kernel.hpp"
#include "traj_vjp_kernel.hpp"
#include "bound_vjp_kernel.hpp"
#include "cost_vjp_kernel.hpp"
#include "traj_jvp_kernel.hpp"

using namespace mpcrl;

namespace {

template <class M>
int launch_stage0(const MpcrlSolver *h, Stage0Args a, hipStream_t st) {
    hipLaunchKernelGGL(stage0_grad_kernel<M>, dim3((unsigned)h->B), dim3(64), 0, st, a);
    HIP_OK(hipGetLastError());
    return 0;
}

// The launch of the lane-layout kernels (du0*/dx0, the trajectory / bound / cost VJPs over B instances, the trajectory JVP over
// B * R items): min(64 / (N + 1), max_ipw) items per wavefront, and at most 32 lanes per instance take the reductions without the
// level at distance 32, as launch_small picks.  P names the kernel template: LANE_KERNEL(K) declares K_p for the kernel K<M, SHORT>.
#define LANE_KERNEL(K)                                 \
    struct K##_p {                                     \
        template <class M, bool SHORT>                 \
        static constexpr auto kernel() {               \
            return K<M, SHORT>;                        \
        }                                              \
    }
LANE_KERNEL(small_state_sens_kernel);
LANE_KERNEL(small_traj_vjp_kernel);
LANE_KERNEL(small_bound_vjp_kernel);
LANE_KERNEL(small_cost_vjp_kernel);
LANE_KERNEL(small_traj_jvp_kernel);
#undef LANE_KERNEL
template <class P, class M, class Args>
int launch_lanes(const MpcrlSolver *h, long items, const Args &a, hipStream_t st) {
    constexpr SmallTraits T = small_traits<M>();
    const int ipw = std::min(64 / (h->N + 1), T.max_ipw);
    const dim3 grid((unsigned)((items + ipw - 1) / ipw)), wave(64);
    if constexpr (!T.seg_skip) {
        if (seg_short(T, h->N)) {
            hipLaunchKernelGGL((P::template kernel<M, true>()), grid, wave, 0, st, h->small, a);
            HIP_OK(hipGetLastError());
            return 0;
        }
    }
    hipLaunchKernelGGL((P::template kernel<M, false>()), grid, wave, 0, st, h->small, a);
    HIP_OK(hipGetLastError());
    return 0;
}
template <class P, class Args>   // ... for the handle's small model
int launch_lanes_model(const MpcrlSolver *h, long items, const Args &a, hipStream_t st) {
    return h->model == MPCRL_MODEL_LINEAR ? launch_lanes<P, LinearDev>(h, items, a, st) : launch_lanes<P, CartpoleDev>(h, items, a, st);
}
// the iterate the handle stores, as the derivative kernels read it
IterateArgs iterate_args(const MpcrlSolver *h) {
    return IterateArgs{h->B, h->theta_stride, h->have_perm ? h->perm : nullptr, h->theta, h->X, h->U, h->PI, h->BND, h->RES};
}

template <class M>
int launch_bound_value(const MpcrlSolver *h, const BoundValueArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(bound_value_grad_kernel<M>, dim3((unsigned)h->B), dim3(64), 0, st, a);
    HIP_OK(hipGetLastError());
    return 0;
}

// which bound rows the handle's OCP has, per group of mpcrl_set_bounds (the rule of SmallSolver::init_bounds / ChainSolver::lbv)
template <class Spec>
void bound_rows_of(const Spec &sp, int nu, int nx, bool qmode, unsigned char (&rows)[3][BOUND_MAXNW]) {
    for (int i = 0; i < nu + nx; ++i) {
        rows[0][i] = (i < nu && !qmode) ? (sp.lb0[i] > -MPCRL_NO_BOUND * 0.1 ? 1 : 0) | (sp.ub0[i] < MPCRL_NO_BOUND * 0.1 ? 2 : 0) : 0;
        rows[1][i] = (sp.lb[i] > -MPCRL_NO_BOUND * 0.1 ? 1 : 0) | (sp.ub[i] < MPCRL_NO_BOUND * 0.1 ? 2 : 0);
        rows[2][i] = i >= nu ? (sp.lbe[i - nu] > -MPCRL_NO_BOUND * 0.1 ? 1 : 0) | (sp.ube[i - nu] < MPCRL_NO_BOUND * 0.1 ? 2 : 0) : 0;
    }
}

}  // namespace

extern "C" {

int mpcrl_ext_version(void) { return MPCRL_EXT_VERSION; }

int mpcrl_state_sens(mpcrl_handle h, int flags, double *dV_dx0, double *dQ_du0, double *dpi_dx0, void *stream) {
    if (!h || (flags & ~MPCRL_STATE_Q_MODE)) return MPCRL_E_ARG;
    const bool qmode = (flags & MPCRL_STATE_Q_MODE) != 0;
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    if (dQ_du0 && !qmode) return MPCRL_E_ARG;
    if (dpi_dx0 && h->is_large) return MPCRL_E_MODEL;
    ON_DEVICE(h->device);
    const hipStream_t st = (hipStream_t)stream;
    if (dV_dx0 || dQ_du0) {
        Stage0Args a;
        a.B = h->B, a.N = h->N, a.theta_stride = h->theta_stride, a.theta = h->theta;
        a.rk_steps = h->is_large ? h->large.rk_steps : h->small.rk_steps;
        a.h = h->is_large ? h->large.h : h->small.h;
        a.c0 = h->is_large ? h->large.dT : h->small.dT;   // c_0 = dT for both cost kinds
        a.X = h->X, a.U = h->U, a.PI = h->PI, a.RES = h->RES, a.consts = h->is_large ? h->consts_dev : nullptr;
        a.dV = dV_dx0, a.dQ = dQ_du0;
        int rc = MPCRL_E_MODEL;
        if (h->model == MPCRL_MODEL_CARTPOLE) rc = launch_stage0<CartpoleDev>(h, a, st);
        else if (h->model == MPCRL_MODEL_LINEAR) rc = launch_stage0<LinearDev>(h, a, st);
        else
            switch (h->n_mass) {
                case 3: rc = launch_stage0<ChainDev<3>>(h, a, st); break;
                case 4: rc = launch_stage0<ChainDev<4>>(h, a, st); break;
                case 5: rc = launch_stage0<ChainDev<5>>(h, a, st); break;
                case 6: rc = launch_stage0<ChainDev<6>>(h, a, st); break;
                case 7: rc = launch_stage0<ChainDev<7>>(h, a, st); break;
            }
        if (rc) return rc;
    }
    if (dpi_dx0) {
        if (qmode)   // u_0 is data: du0/dx0 = 0, as du0/dp is
            HIP_OK(hipMemsetAsync(dpi_dx0, 0, (size_t)h->B * h->nu * h->nx * sizeof(double), st));
        else {
            const StateSensArgs a{iterate_args(h), dpi_dx0};
            const int rc = launch_lanes_model<small_state_sens_kernel_p>(h, h->B, a, st);
            if (rc) return rc;
        }
    }
    return 0;
}

int mpcrl_traj_ext_version(void) { return MPCRL_TRAJ_EXT_VERSION; }

int mpcrl_traj_vjp(mpcrl_handle h, int flags, const double *gX, const double *gU, double *g_x0, double *g_theta, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included: with u_0 pinned the system has other unknowns)
    if (h->is_large) return MPCRL_E_MODEL;
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    if ((!gX && !gU) || (!g_x0 && !g_theta)) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    return launch_lanes_model<small_traj_vjp_kernel_p>(h, h->B, TrajVjpArgs{iterate_args(h), gX, gU, g_x0, g_theta}, (hipStream_t)stream);
}

int mpcrl_traj_jvp_ext_version(void) { return MPCRL_TRAJ_JVP_EXT_VERSION; }

int mpcrl_traj_jvp(mpcrl_handle h, int flags, int ndir, const double *dx0, const double *dtheta, double *dX, double *dU, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included, as in mpcrl_traj_vjp)
    if (h->is_large) return MPCRL_E_MODEL;
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    if (ndir < 1 || (!dx0 && !dtheta) || (!dX && !dU)) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    const TrajJvpArgs a{iterate_args(h), ndir, dx0, dtheta, dX, dU};
    return launch_lanes_model<small_traj_jvp_kernel_p>(h, (long)h->B * ndir, a, (hipStream_t)stream);
}

int mpcrl_chain_ext_version(void) { return MPCRL_CHAIN_EXT_VERSION; }

int mpcrl_chain_policy_state_sens(mpcrl_handle h, int flags, const int32_t *status, double *dpi_dx0, void *stream) {
    if (!h || (flags & ~MPCRL_STATE_Q_MODE) || !status || !dpi_dx0) return MPCRL_E_ARG;
    if (!h->is_large) return MPCRL_E_MODEL;
    if (!h->chain_ws_current) return MPCRL_E_ARG;
    const MpcrlChainEntry *e = chain_entry(h->n_mass);
    if (!e) return MPCRL_E_MODEL;
    ON_DEVICE(h->device);
    const hipStream_t st = (hipStream_t)stream;
    if (flags & MPCRL_STATE_Q_MODE) {   // u_0 is data: du0/dx0 = 0, as du0/dp is
        HIP_OK(hipMemsetAsync(dpi_dx0, 0, (size_t)h->B * h->nu * h->nx * sizeof(double), st));
        return 0;
    }
    return e->policy_state_sens(h, status, dpi_dx0, h->chain_adjoint_current, st);
}

int mpcrl_chain_traj_ext_version(void) { return MPCRL_CHAIN_TRAJ_EXT_VERSION; }

int mpcrl_chain_traj_vjp(mpcrl_handle h, int flags, const int32_t *status, const double *gX, const double *gU, double *g_x0,
                         double *g_theta, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included: with u_0 pinned the system has other unknowns)
    if (!h->is_large) return MPCRL_E_MODEL;
    if (!status || (!gX && !gU) || (!g_x0 && !g_theta)) return MPCRL_E_ARG;
    if (!h->chain_ws_current) return MPCRL_E_ARG;
    const MpcrlChainEntry *e = chain_entry(h->n_mass);
    if (!e) return MPCRL_E_MODEL;
    ON_DEVICE(h->device);
    // the solution and its parameter terms have a region of their own in the workspace: chain_adjoint_current stays as it is
    return e->traj_vjp(h, status, gX, gU, g_x0, g_theta, nullptr, nullptr, h->chain_adjoint_current, (hipStream_t)stream);
}

int mpcrl_chain_traj_jvp_ext_version(void) { return MPCRL_CHAIN_TRAJ_JVP_EXT_VERSION; }

int mpcrl_chain_traj_jvp(mpcrl_handle h, int flags, const int32_t *status, int ndir, const double *dx0, const double *dtheta, double *dX,
                         double *dU, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included, as in mpcrl_chain_traj_vjp)
    if (!h->is_large) return MPCRL_E_MODEL;
    if (!status || ndir < 1 || (!dx0 && !dtheta) || (!dX && !dU)) return MPCRL_E_ARG;
    if (!h->chain_ws_current) return MPCRL_E_ARG;
    const MpcrlChainEntry *e = chain_entry(h->n_mass);
    if (!e) return MPCRL_E_MODEL;
    ON_DEVICE(h->device);
    // the right-hand side and the solution live in regions every factorisation fills before it reads them: chain_adjoint_current stays
    return e->traj_jvp(h, status, ndir, dx0, dtheta, dX, dU, h->chain_adjoint_current, (hipStream_t)stream);
}

int mpcrl_bound_ext_version(void) { return MPCRL_BOUND_EXT_VERSION; }

int mpcrl_bound_value_grad(mpcrl_handle h, int flags, double *dV_dlb, double *dV_dub, void *stream) {
    if (!h || (flags & ~MPCRL_STATE_Q_MODE)) return MPCRL_E_ARG;
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    if (!dV_dlb && !dV_dub) return MPCRL_E_ARG;
    if (h->nu + h->nx > BOUND_MAXNW) return MPCRL_E_MODEL;   // (no model has more: not reached)
    ON_DEVICE(h->device);
    const hipStream_t st = (hipStream_t)stream;
    BoundValueArgs a{};
    a.B = h->B, a.N = h->N, a.theta_stride = h->theta_stride, a.qmode = (flags & MPCRL_STATE_Q_MODE) != 0, a.theta = h->theta;
    a.X = h->X, a.U = h->U, a.PI = h->PI, a.BND = h->BND, a.RES = h->RES, a.dlb = dV_dlb, a.dub = dV_dub;
    if (h->is_large) bound_rows_of(h->large, h->nu, h->nx, a.qmode, a.rows);
    else bound_rows_of(h->small, h->nu, h->nx, a.qmode, a.rows);
    if (h->model == MPCRL_MODEL_CARTPOLE) return launch_bound_value<CartpoleDev>(h, a, st);
    if (h->model == MPCRL_MODEL_LINEAR) return launch_bound_value<LinearDev>(h, a, st);
    switch (h->n_mass) {
        case 3: return launch_bound_value<ChainDev<3>>(h, a, st);
        case 4: return launch_bound_value<ChainDev<4>>(h, a, st);
        case 5: return launch_bound_value<ChainDev<5>>(h, a, st);
        case 6: return launch_bound_value<ChainDev<6>>(h, a, st);
        case 7: return launch_bound_value<ChainDev<7>>(h, a, st);
    }
    return MPCRL_E_MODEL;
}

int mpcrl_bound_vjp(mpcrl_handle h, int flags, const double *gX, const double *gU, double *g_x0, double *g_theta, double *g_lb,
                    double *g_ub, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included, as in mpcrl_traj_vjp)
    if (h->is_large) return MPCRL_E_MODEL;
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    if ((!gX && !gU) || (!g_x0 && !g_theta && !g_lb && !g_ub)) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    const TrajVjpArgs t{iterate_args(h), gX, gU, g_x0, g_theta};
    if (!g_lb && !g_ub) return launch_lanes_model<small_traj_vjp_kernel_p>(h, h->B, t, (hipStream_t)stream);   // the launch of mpcrl_traj_vjp itself: its bits
    const BoundVjpArgs a{t, g_lb, g_ub};
    return launch_lanes_model<small_bound_vjp_kernel_p>(h, h->B, a, (hipStream_t)stream);
}

int mpcrl_chain_bound_vjp(mpcrl_handle h, int flags, const int32_t *status, const double *gX, const double *gU, double *g_x0,
                          double *g_theta, double *g_lb, double *g_ub, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included, as in mpcrl_chain_traj_vjp)
    if (!h->is_large) return MPCRL_E_MODEL;
    if (!status || (!gX && !gU) || (!g_x0 && !g_theta && !g_lb && !g_ub)) return MPCRL_E_ARG;
    if (!h->chain_ws_current) return MPCRL_E_ARG;
    const MpcrlChainEntry *e = chain_entry(h->n_mass);
    if (!e) return MPCRL_E_MODEL;
    ON_DEVICE(h->device);
    return e->traj_vjp(h, status, gX, gU, g_x0, g_theta, g_lb, g_ub, h->chain_adjoint_current, (hipStream_t)stream);
}

int mpcrl_cost_ext_version(void) { return MPCRL_COST_EXT_VERSION; }

int mpcrl_cost_value_grad(mpcrl_handle h, int flags, double *dV_dcost, void *stream) {
    if (!h || flags || !dV_dcost) return MPCRL_E_ARG;
    if (h->model != MPCRL_MODEL_CARTPOLE) return MPCRL_E_MODEL;
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    CostValueArgs a;
    a.B = h->B, a.N = h->N, a.theta_stride = h->theta_stride, a.cost_kind = h->small.cost_kind;
    a.dT = h->small.dT, a.gamma = h->small.gamma, a.theta = h->theta;
    a.X = h->X, a.U = h->U, a.PI = h->PI, a.RES = h->RES, a.dV = dV_dcost;
    hipLaunchKernelGGL(cost_value_grad_kernel<CartpoleDev>, dim3((unsigned)h->B), dim3(64), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_cost_vjp(mpcrl_handle h, int flags, const double *gX, const double *gU, double *g_x0, double *g_theta, double *g_lb,
                   double *g_ub, double *g_cost, void *stream) {
    if (!h || flags) return MPCRL_E_ARG;   // (MPCRL_STATE_Q_MODE included, as in mpcrl_traj_vjp)
    if (h->model != MPCRL_MODEL_CARTPOLE) return MPCRL_E_MODEL;
    if (!g_cost) {   // the launch of mpcrl_bound_vjp itself: its refusals, its bits
        if (!g_x0 && !g_theta && !g_lb && !g_ub) return MPCRL_E_ARG;
        return mpcrl_bound_vjp(h, flags, gX, gU, g_x0, g_theta, g_lb, g_ub, stream);
    }
    if (!h->have_iterate || h->dual_cold) return MPCRL_E_ARG;
    if (!gX && !gU) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    const CostVjpArgs a{BoundVjpArgs{TrajVjpArgs{iterate_args(h), gX, gU, g_x0, g_theta}, g_lb, g_ub}, g_cost};
    return launch_lanes<small_cost_vjp_kernel_p, CartpoleDev>(h, h->B, a, (hipStream_t)stream);
}

}  // extern "C"
