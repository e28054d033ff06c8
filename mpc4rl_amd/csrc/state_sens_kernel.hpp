// state_sens_kernel.hpp — derivatives of a solve with respect to its initial state and its pinned first control
// (include/mpcrl_ext.h, mpcrl_state_sens), on the iterate (x, u, pi, lam, t) a solve kernel stored:
//
//   stage0_grad_kernel<M>            dV/dx0 (dQ/dx0 in Q mode) = grad_x l0 and dQ/du0 = grad_u l0 at (x_0, u_0), with
//                                    l0(x, u) = c_0 l_0(x, u, theta) + pi_1' F(x, u, theta).  All three models.
//   small_state_sens_kernel<M, S>    du0*/dx0 of the cartpole and the linear system: the adjoint solve of the du0*/dp pass
//                                    (SmallSolver::kkt_assemble / kkt_solve, small_kernel.hpp), contracted with the two places x0
//                                    enters once x_0 is eliminated: the (u, x) block of the stage-0 Hessian and A_0
//                                    (SmallSolver::dx0_contract).  No parameter jets run.
//
// Neither kernel has the status word of the solve (mpcrl_solve writes it into the caller's array, the handle does not keep it): an
// instance counts as solved when its stored residuals, its stored x, u, pi and its dynamics parameters are all finite
// (iterate_entry_bad below, the same rule in both kernels).
#pragma once
#include <type_traits>

#include "small_kernel.hpp"

namespace mpcrl {

// the iterate a solve stored, as the lane-layout kernels of this unit take it (mpcrl_state.hip: iterate_args)
struct IterateArgs {
    int B, theta_stride;
    const int *perm;                         // packing order of the handle or null (results do not depend on it)
    const double *theta;                     // [np] or [B, np]
    const double *X, *U, *PI, *BND, *RES;    // stored iterate, layouts of mpcrl_get_iterate
};

struct Stage0Args {
    int B, N, theta_stride, rk_steps;
    double h, c0;                      // RK4 step, cost scaling of stage 0
    const double *theta;               // [np] or [B, np]
    const double *X, *U, *PI, *RES;    // stored iterate, layouts of mpcrl_get_iterate
    const double *consts;              // chain: x_ss (device); else null
    double *dV, *dQ;                   // [B, nx] / [B, nu]; either may be null
};

MPCRL_DI bool iterate_entry_bad(double v) { return !(fabs(v) < 1e300); }

// d l_0 / d v_c of the UNSCALED stage-0 cost, v = [u; x]; x, u point at the stored stage 0, p at the full parameter vector
template <class M>
MPCRL_DI double stage0_cost_grad(int c, const double *x, const double *u, const double *p, const double *consts) {
    constexpr int NU = M::NU, NW = M::NX + M::NU;
    if constexpr (std::is_same<M, CartpoleDev>::value) {   // 1/2 r' W_0 r, r = y - yref_0, y = [x; u] (models_dev.hpp)
        const double *W = p + M::P_W0;
        double a = 0.0;
        for (int j = 0; j < NW; ++j) {
            const double vj = j < NU ? u[j] : x[j - NU];
            a = fma(0.5 * (W[M::yi(j) * 5 + M::yi(c)] + W[M::yi(c) * 5 + M::yi(j)]), vj - p[M::P_YREF0 + M::yi(j)], a);
        }
        return a;
    } else if constexpr (std::is_same<M, LinearDev>::value) {   // V_0 + 1/2 y'y + f'y, f = p[9 .. 11] in y = [x; u] order
        return c < NU ? u[0] + p[11] : x[c - NU] + p[9 + c - NU];
    } else {   // chain: 1/2 (x - x_ss)' Q (x - x_ss) + 1/2 u' R u
        double a = 0.0;
        if (c < NU)
            for (int j = 0; j < NU; ++j) a = fma(M::Rs(p, c, j), u[j], a);
        else
            for (int j = 0; j < M::NX; ++j) a = fma(M::Qs(p, c - NU, j), x[j] - consts[j], a);
        return a;
    }
}

// One wavefront per instance, lane c < NU + NX = coordinate c of [u_0; x_0]: a single-direction first-order jet through the discrete
// map, dotted with pi_1, plus the cost term.  All 64 lanes scan the instance's iterate for the "solved" rule first.
template <class M>
__global__ void __launch_bounds__(64) stage0_grad_kernel(const Stage0Args a) {
    constexpr int NX = M::NX, NU = M::NU, NW = NX + NU;
    constexpr bool SMALL = std::is_same<M, CartpoleDev>::value || std::is_same<M, LinearDev>::value;
    const int c = threadIdx.x;
    const long inst = blockIdx.x;
    const int N = a.N;
    const double *p = a.theta + (size_t)inst * a.theta_stride;
    const double *X = a.X + (size_t)inst * (N + 1) * NX, *U = a.U + (size_t)inst * N * NU, *PI = a.PI + (size_t)inst * N * NX;
    bool bad = false;
    for (int e = c; e < (N + 1) * NX; e += 64) bad |= iterate_entry_bad(X[e]);
    for (int e = c; e < N * NU; e += 64) bad |= iterate_entry_bad(U[e]);
    for (int e = c; e < N * NX; e += 64) bad |= iterate_entry_bad(PI[e]);
    for (int e = c; e < M::NTD; e += 64) bad |= iterate_entry_bad(p[M::td_index(e)]);
    if (c < 4) bad |= iterate_entry_bad(a.RES[inst * 4 + c]);
    const bool solved = !__any(bad);
    if (c >= NW) return;
    using J = Jet1<1>;
    J jx[NX], ju[NU], jn[NX];
#pragma unroll
    for (int i = 0; i < NU; ++i) ju[i] = J(U[i]), ju[i].d[0] = c == i ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) jx[i] = J(X[i]), jx[i].d[0] = c == NU + i ? 1.0 : 0.0;
    if constexpr (SMALL) {
        J jt[M::NTD];
#pragma unroll
        for (int i = 0; i < M::NTD; ++i) jt[i] = J(p[M::td_index(i)]);
        disc_map<M, J>(jx, ju, jt, jn, a.h, a.rk_steps);
    } else
        disc_map_p<M, J>(jx, ju, p, jn, a.h, a.rk_steps);
    double g = a.c0 * stage0_cost_grad<M>(c, X, U, p, a.consts);
#pragma unroll
    for (int m = 0; m < NX; ++m) g = fma(PI[m], jn[m].d[0], g);
    g = solved ? g : 0.0;
    if (c < NU) {
        if (a.dQ) a.dQ[inst * NU + c] = g;
    } else if (a.dV)
        a.dV[inst * NX + (c - NU)] = g;
}

struct StateSensArgs {
    IterateArgs it;
    double *dpi;   // [B, nu, nx]
};

// Lane layout, loads and linearisation of small_sens_kernel (one lane per stage, min(64 / (N + 1), M::MAX_IPW) instances per
// wavefront); V mode only (the host writes the zeros of Q mode).  The linearised KKT system and its solve are SmallSolver's
// (kkt_assemble, kkt_solve in small_kernel.hpp), the ones of the du0*/dp pass.
template <class M, bool SHORT = false>
__global__ void __launch_bounds__(64) small_state_sens_kernel(const SmallSpec sp, const StateSensArgs a) {
    using SS = SmallSolver<M, SHORT>;
    constexpr int NX = M::NX, NU = M::NU, NW = NX + NU, NTD = M::NTD, NTC = M::NTC;
    const int lane = threadIdx.x;
    const int N = sp.N, lpi = N + 1, ipw = min(64 / lpi, M::MAX_IPW);
    const int slot = lane / lpi, k = lane - slot * lpi, base = slot * lpi;
    long inst = (long)blockIdx.x * ipw + slot;
    const bool valid = slot < ipw && inst < a.it.B;
    if (!valid) inst = a.it.B - 1;
    if (a.it.perm) inst = a.it.perm[inst];
    SS S(sp, k, lpi, base);
    __shared__ __attribute__((aligned(16))) double mx_lds[SS::MX ? SS::MX_LDS : 2];
    S.ms = mx_lds;
    const bool term = S.term, first = S.first;
    S.qmode = false;
    S.init_bounds();
    if (sp.cost_kind == 0)
        S.ck = term ? 1.0 : sp.dT;
    else
        S.ck = first ? sp.dT : (term ? pow(sp.gamma, (double)N) : pow(sp.gamma, (double)k) * sp.dT);
    const double *th = a.it.theta + (size_t)inst * a.it.theta_stride;
    __shared__ double c_lds[M::MAX_IPW * SS::CTAB];
    S.fill_cost_table(c_lds, slot < ipw ? slot : 0, slot < ipw, th);
    SS::wave_lds_sync();
    S.load_hc();
    // (lanes past the last instance slot shadow another instance: they get a slot of their own)
    __shared__ double th_slots[SS::TH_LDS ? (M::MAX_IPW + 1) * SS::TH_DOUBLES : 1];
    S.bind_theta(th_slots + (slot < ipw ? slot : M::MAX_IPW) * SS::TH_DOUBLES);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NTD; ++i) {
        const double v = th[M::td_index(i)];
        S.thd.set(i, v), bad |= iterate_entry_bad(v);
    }
#pragma unroll
    for (int i = 0; i < NTC; ++i) S.thc.set(i, th[M::tc_index(i)]);
    const size_t nb = (size_t)(N + 1) * NW;
    const double *bnd = a.it.BND + (size_t)inst * 10 * nb + (size_t)k * NW;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        S.x[i] = a.it.X[(inst * (N + 1) + k) * NX + i];
        S.nu_[i] = first ? 0.0 : a.it.PI[(inst * N + k - 1) * NX + i];
        bad |= iterate_entry_bad(S.x[i]) || iterate_entry_bad(S.nu_[i]);
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) S.u[i] = term ? 0.0 : a.it.U[(inst * N + k) * NU + i], bad |= iterate_entry_bad(S.u[i]);
#pragma unroll
    for (int i = 0; i < NW; ++i) S.lam[0][i] = bnd[0 * nb + i], S.lam[1][i] = bnd[1 * nb + i], S.t[0][i] = bnd[2 * nb + i], S.t[1][i] = bnd[3 * nb + i];
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= iterate_entry_bad(a.it.RES[inst * 4 + j]);
    const bool sv = valid && seg_max<M::SEG_SKIP, SHORT>(bad ? 1.0 : 0.0, k, lpi, base) < 0.5;
    double nun[NX], hdd[SS::NHD], Hx[SS::NHT];
    // the dynamics Jacobians and the second-order term of the final iterate, as the du0*/dp pass linearises it
    double xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = lane_dn(S.x[i]), nun[i] = lane_dn(S.nu_[i]);
    S.template linearize<true>(xn, nun, hdd);
#pragma unroll
    for (int i = 0; i < SS::NPK; ++i) S.P[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) S.p[i] = 0.0;
    const bool capped_x = S.kkt_assemble(Hx, hdd);
    double zero[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) zero[i] = 0.0;
    bool okall = true;
#pragma unroll
    for (int iu = 0; iu < NU; ++iu) {
#pragma unroll
        for (int i = 0; i < NW; ++i) S.rt[i] = (first && i == iu) ? -1.0 : 0.0;
        S.template kkt_solve<true>(Hx, zero, capped_x, iu, okall);
        // The parameter pass solves with the right-hand side -e and stores minus its sums; so does this one.
        double ynn[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) ynn[i] = lane_dn(S.Dnu[i]);
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const double s = S.dx0_contract(Hx, ynn, j);
            if (first && valid) a.dpi[(inst * NU + iu) * NX + j] = sv ? (okall ? -s : NAN) : 0.0;
        }
    }
}

}  // namespace mpcrl
