// chain_inst.hip — the chain-of-masses kernels of ONE chain size (-DMPCRL_CHAIN_NMASS=3..7) and their launch sequence; one translation
// unit per size so that the sizes compile in parallel (mpcrl_host.hpp, csrc/Makefile).
#include "mpcrl_host.hpp"

#include "chain_kernel.hpp"

#ifndef MPCRL_CHAIN_NMASS
#error "compile with -DMPCRL_CHAIN_NMASS=3..7"
#endif

using namespace mpcrl;

namespace {

using Model = ChainDev<MPCRL_CHAIN_NMASS>;

// dynamic LDS of the chain kernels for a horizon of N stages (bytes): the SQP / adjoint-Riccati kernels, the second-order point pass,
// the mixed-term kernel, the output reduction.  mpcrl_create refuses a (chain size, horizon) pair whose largest request does not fit.
template <class M>
struct LargeLds {
    unsigned sqp, point, mix2, out;
    explicit LargeLds(int N)
        : sqp((unsigned)(ChainCfg<M>::lds_doubles(N) * sizeof(double))),
          point((unsigned)((M::NTD + N * M::NX) * sizeof(double))),
          mix2((unsigned)((M::NTD + M::NX) * 64 * sizeof(double))),
          out((unsigned)((64 + (1 + M::NU) * ((N + 1) * M::NX + N * M::NU)) * sizeof(double))) {}
    bool fits() const {   // 64 KB per workgroup; the SQP kernel also holds ~1 KB of static LDS
        return sqp + 1024 <= 64 * 1024 && point <= 64 * 1024 && mix2 <= 64 * 1024 && out <= 64 * 1024;
    }
};

template <class M>
int launch_large(MpcrlSolver *h, LargeArgs a, hipStream_t st) {
    a.ws = h->ws, a.ws_stride = h->ws_stride;
    const int B = h->B, N = h->N;
    const LargeLds<M> lds(N);
    if (!lds.fits()) return MPCRL_E_ARG;   // (mpcrl_create has checked: not reached)
    hipLaunchKernelGGL(chain_init_kernel<M>, dim3(B), dim3(64), 0, st, h->large, a);
    // the whole SQP loop of an instance runs inside one wavefront of one launch (linearisation, QP, step; chain_linearise.hpp)
    hipLaunchKernelGGL(chain_sqp_kernel<M>, dim3(B), dim3(64), lds.sqp, st, h->large, a);
    HIP_OK(hipGetLastError());
    if (a.flags & (MPCRL_SENS_V | MPCRL_SENS_PI)) {
        const bool want_pi = (a.flags & MPCRL_SENS_PI) && a.dpi && !a.u0fix;
        // second-order point pass, then grad_theta (nu' F) from its tables: the same evaluation order for dV/dp whatever the flags
        hipLaunchKernelGGL((chain_point_kernel<M, true>), dim3((unsigned)B), dim3(64), lds.point, st, h->large, a);
        hipLaunchKernelGGL(chain_sens_th2_kernel<M>, dim3((unsigned)(((long)B * N + 63) / 64)), dim3(64), 0, st, h->large, a);
        if (want_pi) {
            hipLaunchKernelGGL(chain_sens_ad_kernel<M>, dim3((unsigned)(B * HexCfg<M>::groups(N))), dim3(64), 0, st, h->large, a);
            hipLaunchKernelGGL(chain_sens_riccati_kernel<M>, dim3(B), dim3(64), lds.sqp, st, h->large, a);
            hipLaunchKernelGGL(chain_sens_mix2_kernel<M>, dim3((unsigned)(((long)B * N * M::NU + 63) / 64)), dim3(64), lds.mix2, st, h->large, a);
        }
        // one workgroup of 1024 lanes per instance; its trajectories staged in LDS (chain_sens_out_kernel)
        hipLaunchKernelGGL(chain_sens_out_kernel<M>, dim3((unsigned)B), dim3(1024), lds.out, st, h->large, a);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

// du0*/dx0 of the handle's last solve (include/mpcrl_chain_ext.h).  With the exact Hessians and the adjoint solutions of that solve
// in the workspace: the contraction alone.  Otherwise the adjoint pipeline first, launched as launch_large launches it on the stored
// iterate, without the parameter terms (chain_sens_th2, chain_sens_mix2 and chain_sens_out do not run).
template <class M>
int launch_policy_state_sens(MpcrlSolver *h, const int32_t *status, double *dpi_dx0, bool adjoint_current, hipStream_t st) {
    const int B = h->B, N = h->N;
    const LargeLds<M> lds(N);
    if (!lds.fits()) return MPCRL_E_ARG;   // (mpcrl_create has checked: not reached)
    LargeArgs a{};
    a.B = B, a.theta_stride = h->theta_stride, a.theta = h->theta;
    a.X = h->X, a.U = h->U, a.PI = h->PI, a.BND = h->BND, a.RES = h->RES, a.LAG = h->LAG;
    a.ws = h->ws, a.ws_stride = h->ws_stride, a.status = const_cast<int32_t *>(status);
    // what chain_sens_riccati_kernel's guard asks for: the policy pass in V mode.  It writes nothing through a.dpi (chain_sens_out does)
    a.flags = MPCRL_SENS_PI, a.dpi = dpi_dx0, a.u0fix = nullptr;
    if (!adjoint_current) {
        hipLaunchKernelGGL((chain_point_kernel<M, true>), dim3((unsigned)B), dim3(64), lds.point, st, h->large, a);
        hipLaunchKernelGGL(chain_sens_ad_kernel<M>, dim3((unsigned)(B * HexCfg<M>::groups(N))), dim3(64), 0, st, h->large, a);
        hipLaunchKernelGGL(chain_sens_riccati_kernel<M>, dim3(B), dim3(64), lds.sqp, st, h->large, a);
    }
    hipLaunchKernelGGL(chain_state_sens_kernel<M>, dim3((unsigned)B), dim3(64), 0, st, h->large, a, dpi_dx0);
    HIP_OK(hipGetLastError());
    return 0;
}

// The trajectory VJP of the handle's last solve (include/mpcrl_chain_traj_ext.h).  The exact Hessians and the point tables are in the
// workspace after a solve that ran MPCRL_SENS_PI in V mode; otherwise the second-order point pass and chain_sens_ad first, as above.
// Then the adjoint solve for the cotangent, the mixed term of its one solution (only g_theta reads it) and the outputs.  Every
// dynamic-LDS request is at most the du0*/dp pass's (LargeLds: one solution staged instead of 1 + NU).
// g_lb / g_ub (include/mpcrl_bound_ext.h, mpcrl_chain_bound_vjp; both null for mpcrl_chain_traj_vjp): one launch more, of
// chain_bound_out_kernel on the solution the adjoint solve left, when either is requested; g_x0 and g_theta may then both be null,
// and chain_traj_out_kernel runs only when one of them is requested.
template <class M>
int launch_traj_vjp(MpcrlSolver *h, const int32_t *status, const double *gX, const double *gU, double *g_x0, double *g_theta,
                    double *g_lb, double *g_ub, bool adjoint_current, hipStream_t st) {
    const int B = h->B, N = h->N;
    const LargeLds<M> lds(N);
    if (!lds.fits()) return MPCRL_E_ARG;   // (mpcrl_create has checked: not reached)
    LargeArgs a{};
    a.B = B, a.theta_stride = h->theta_stride, a.theta = h->theta;
    a.X = h->X, a.U = h->U, a.PI = h->PI, a.BND = h->BND, a.RES = h->RES, a.LAG = h->LAG;
    a.ws = h->ws, a.ws_stride = h->ws_stride, a.status = const_cast<int32_t *>(status);
    a.flags = MPCRL_SENS_PI, a.u0fix = nullptr;      // (as launch_policy_state_sens; a.dpi stays null: nothing here reads or writes it)
    if (!adjoint_current) {
        hipLaunchKernelGGL((chain_point_kernel<M, true>), dim3((unsigned)B), dim3(64), lds.point, st, h->large, a);
        hipLaunchKernelGGL(chain_sens_ad_kernel<M>, dim3((unsigned)(B * HexCfg<M>::groups(N))), dim3(64), 0, st, h->large, a);
    }
    hipLaunchKernelGGL(chain_traj_riccati_kernel<M>, dim3(B), dim3(64), lds.sqp, st, h->large, a, gX, gU);
    if (g_theta)
        hipLaunchKernelGGL((chain_sens_mix2_kernel<M, 1>), dim3((unsigned)(((long)B * N + 63) / 64)), dim3(64), lds.mix2, st, h->large, a);
    const unsigned lds_out = (unsigned)((64 + 2 * ((N + 1) * M::NX + N * M::NU)) * sizeof(double));
    if (g_x0 || g_theta)
        hipLaunchKernelGGL(chain_traj_out_kernel<M>, dim3((unsigned)B), dim3(1024), lds_out, st, h->large, a, gX, g_x0, g_theta);
    if (g_lb || g_ub) hipLaunchKernelGGL(chain_bound_out_kernel<M>, dim3((unsigned)B), dim3(64), 0, st, h->large, a, g_lb, g_ub);
    HIP_OK(hipGetLastError());
    return 0;
}

// The trajectory JVP of the handle's last solve (include/mpcrl_chain_traj_jvp_ext.h).  The exact Hessians and the point tables as in
// launch_traj_vjp; then per direction the right-hand side from the point tables (only with dtheta) and the primal solve, in sequence on
// the stream: the directions of an instance share its workspace (rt / rb, the gain rows of the stage blocks, Dx / Du).  2 ndir launches
// (ndir without dtheta), two more when the adjoint is not current — whatever the horizon.  The dynamic LDS of the right-hand-side
// kernel (3 NX doubles per lane) is less than the mixed-term kernel's (NTD + NX).
template <class M>
int launch_traj_jvp(MpcrlSolver *h, const int32_t *status, int ndir, const double *dx0, const double *dtheta, double *dX, double *dU,
                    bool adjoint_current, hipStream_t st) {
    const int B = h->B, N = h->N;
    const LargeLds<M> lds(N);
    if (!lds.fits()) return MPCRL_E_ARG;   // (mpcrl_create has checked: not reached)
    LargeArgs a{};
    a.B = B, a.theta_stride = h->theta_stride, a.theta = h->theta;
    a.X = h->X, a.U = h->U, a.PI = h->PI, a.BND = h->BND, a.RES = h->RES, a.LAG = h->LAG;
    a.ws = h->ws, a.ws_stride = h->ws_stride, a.status = const_cast<int32_t *>(status);
    a.flags = MPCRL_SENS_PI, a.u0fix = nullptr;      // (as launch_traj_vjp)
    if (!adjoint_current) {
        hipLaunchKernelGGL((chain_point_kernel<M, true>), dim3((unsigned)B), dim3(64), lds.point, st, h->large, a);
        hipLaunchKernelGGL(chain_sens_ad_kernel<M>, dim3((unsigned)(B * HexCfg<M>::groups(N))), dim3(64), 0, st, h->large, a);
    }
    const unsigned lds_rhs = (unsigned)(3 * M::NX * 64 * sizeof(double));
    for (int d = 0; d < ndir; ++d) {
        if (dtheta)
            hipLaunchKernelGGL(chain_jvp_rhs_kernel<M>, dim3((unsigned)(((long)B * N + 63) / 64)), dim3(64), lds_rhs, st, h->large, a, dtheta, ndir, d);
        hipLaunchKernelGGL(chain_traj_jvp_riccati_kernel<M>, dim3(B), dim3(64), lds.sqp, st, h->large, a, dx0, dtheta, dX, dU, ndir, d);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

size_t ws_doubles(int N) { return LargeLayout<Model>(N).total; }
bool lds_fits(int N) { return LargeLds<Model>(N).fits(); }

#ifdef MPCRL_PROFILE_PHASES
int debug_phases(unsigned long long *out, int reset) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_ticks), sizeof(unsigned long long) * 16));
    if (reset) {
        unsigned long long z[16] = {0};
        HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_ticks), z, sizeof(z)));
    }
    return 0;
}
#else
constexpr int (*debug_phases)(unsigned long long *, int) = nullptr;
#endif

}  // namespace

#define MPCRL_CAT_(a, b) a##b
#define MPCRL_CAT(a, b) MPCRL_CAT_(a, b)
const MpcrlChainEntry *MPCRL_CAT(mpcrl_chain_entry_, MPCRL_CHAIN_NMASS)() {
    static const MpcrlChainEntry e = {MPCRL_CHAIN_NMASS, (long)Model::NP, ws_doubles, lds_fits, launch_large<Model>, debug_phases,
                                     launch_policy_state_sens<Model>, launch_traj_vjp<Model>, launch_traj_jvp<Model>};
    return &e;
}
