// traj_vjp_kernel.hpp — vector-Jacobian product of a solve's whole planned trajectory (include/mpcrl_traj_ext.h, mpcrl_traj_vjp), on
// the iterate (x, u, pi, lam, t) a solve kernel stored:
//
//   small_traj_vjp_kernel<M, S>    for a cotangent G = (G_X [N + 1, nx], G_U [N, nu]) on (X*, U*) of the cartpole and the linear system:
//                                  g_theta = sum_k G_X[k]' dx_k*/dtheta + G_U[k]' du_k*/dtheta and g_x0, the same sums over d/dx0.
//
// The KKT matrix of the du0*/dp pass (SmallSolver::kkt_assemble / kkt_solve, small_kernel.hpp) is symmetric, so G' dw*/d(.) =
// -(K^-1 G)' dR/d(.): ONE adjoint solve with the right-hand side -G spread over the stages, whatever the horizon, then the two
// contractions the library already has for the right-hand side -e_{u_0}: with dR/dtheta as sensitivities() contracts it
// (SmallSolver::dtheta_contract), and with dR/dx0 as small_state_sens_kernel contracts it (SmallSolver::dx0_contract), plus G_X[0]
// itself because x_0 = x0.  Lane layout, loads, the "solved" rule and the linearisation are those of small_state_sens_kernel.
//
// The kernel's body is small_traj_vjp_body<M, S, BOUNDS, COST>: BOUNDS = false is this kernel, BOUNDS = true the kernel of
// include/mpcrl_bound_ext.h (bound_vjp_kernel.hpp), which contracts the same solution with the bound rows as well.  Everything the
// bound outputs add sits behind `if constexpr (BOUNDS)`, so this kernel's arithmetic and its order are untouched by it.  COST is a hook
// of the same kind: a functor with COST::ON that contracts the merged solution with the stage's cost residual (cost_vjp_kernel.hpp,
// include/mpcrl_cost_ext.h); the default, NoCostOut, is never called.
#pragma once
#include "state_sens_kernel.hpp"

namespace mpcrl {

struct NoCostOut {
    static constexpr bool ON = false;
};

struct TrajVjpArgs {
    IterateArgs it;
    const double *gX, *gU;     // cotangents [B, N + 1, nx] / [B, N, nu]; null = zeros
    double *g_x0, *g_theta;    // [B, nx] / [B, np]; either may be null
};

// Every requested row is written in full: zeros for an instance without a solved iterate and at the entries of p the sensitivity pass
// does not differentiate (M::p_has_gradient), NaN where the factorisation met a non-positive pivot.
// g_lb / g_ub [B, N + 1, nu + nx] (BOUNDS only; either may be null): for the bound row of side sd on coordinate i of this stage's
// v = [u; x], dR/db is -sgn in the row h + t of that bound alone, and eliminating (lam, t) leaves G' dw*/db = (lam / t) y_v[i] for
// either side — with the weight the solve used, min(lam / t, SENS_W_MAX).  Exactly 0 where has() says there is no row.
template <class M, bool SHORT, bool BOUNDS, class COST = NoCostOut>
MPCRL_DI void small_traj_vjp_body(const SmallSpec sp, const TrajVjpArgs a, double *g_lb, double *g_ub, [[maybe_unused]] const COST cost = COST()) {
    using SS = SmallSolver<M, SHORT>;
    constexpr int NX = M::NX, NU = M::NU, NW = NX + NU, NP = M::NP, NTD = M::NTD, NTC = M::NTC, NT = NTD + NTC;
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
    // the cotangent of this stage: no control at the terminal stage, and x_0 is eliminated (G_X[0] enters g_x0 directly, below)
    double gx0[NX];
#pragma unroll
    for (int i = 0; i < NU; ++i) S.rt[i] = (term || !a.gU) ? 0.0 : -a.gU[(inst * N + k) * NU + i];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const double g = a.gX ? a.gX[(inst * (N + 1) + k) * NX + i] : 0.0;
        S.rt[NU + i] = first ? 0.0 : -g;
        gx0[i] = g;   // (read on the first lane only)
    }
    double nun[NX], hdd[SS::NHD];
    // the dynamics Jacobians and the second-order term of the final iterate, as the du0*/dp pass linearises it
    double xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = lane_dn(S.x[i]), nun[i] = lane_dn(S.nu_[i]);
    S.template linearize<true>(xn, nun, hdd);
#pragma unroll
    for (int i = 0; i < SS::NPK; ++i) S.P[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) S.p[i] = 0.0;
    // the Hessian fill of SmallSolver::kkt_assemble, in this body's own text as well
    double Hx[SS::NHT];
#pragma unroll
    for (int i = 0; i < NW; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Hx[SS::sym(i, j)] = S.ck * S.hess_of_stage(i, j);
#pragma unroll
    for (int di = 0; di < M::NLD; ++di)
#pragma unroll
        for (int dj = 0; dj <= di; ++dj) Hx[SS::sym(M::lin_coord(di), M::lin_coord(dj))] += hdd[di * (di + 1) / 2 + dj];
    // From here to the bound rows after the solve this body keeps its OWN text of SmallSolver::barrier_diag / kkt_solve (the barrier
    // diagonal capped at SENS_W_MAX, the solve, the per-instance extrapolation with its second solve at SENS_W_MAX / 2, the merge): with
    // the shared members, bound_rows as a hook of kkt_solve, the cartpole cost kernel measured 0.4 .. 1.0 us slower on its g_cost-only
    // call than the parent's whichever build ran first; with this text the six cartpole kernels of this body compile to the parent's
    // instructions (profiles/sens_kkt_kernel_resources.txt).  A change to the cap rule or to the extrapolation is made in both places.
    bool capped_x = false;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        double d = 0.0;
#pragma unroll
        for (int sd = 0; sd < 2; ++sd)
            if (S.has(sd, i)) {
                const double w = S.lam[sd][i] / S.t[sd][i];
                d += fmin(w, SENS_W_MAX);
                if (i >= NU && w > SENS_W_MAX) capped_x = true;
            }
        S.Dg[i] = d;
    }
    auto Hs = [&](int i, int j) { return Hx[SS::sym(i, j)]; };
    S.hscale = 1.0;
    double zero[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) zero[i] = 0.0;
    bool okall = true;
    // BOUNDS: the products w y_v of this stage's rows, from the solution (yx, yu) at the cap W and, where the instance extrapolates
    // (ex), also from the one at W / 2 still in S.Dx / S.Du: each solve with its own capped weight, then 2 w1 y(W) - w2 y(W / 2).  On a
    // capped row y = a / c + b / c^2 + ..., so c y = a + b / c: the extrapolation takes b / c out only if it acts on the product.
    [[maybe_unused]] auto bound_rows = [&](const double *yx, const double *yu, bool ex) {
        if constexpr (!BOUNDS) return;   // (and nothing is captured)
        else {
        if (!valid) return;
        const size_t row = ((size_t)inst * (N + 1) + k) * NW;
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
            double *o = sd ? g_ub : g_lb;
            if (!o) continue;   // (wave-uniform)
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                double v = 0.0;
                if (S.has(sd, i)) {
                    const double w = S.lam[sd][i] / S.t[sd][i];
                    v = fmin(w, SENS_W_MAX) * S.dvc(yx, yu, i);
                    if (ex) v = fma(2.0, v, -(fmin(w, 0.5 * SENS_W_MAX) * S.dvc(S.Dx, S.Du, i)));
                    v = sv ? (okall ? v : NAN) : 0.0;
                }
                o[row + i] = v;
            }
        }
        }
    };
    [[maybe_unused]] bool rows_done = false;   // (wave-uniform)
    if constexpr (SS::MX) {
        const bool okf = S.template mx_pred<true>(Hs, S.rt, zero);
        S.mx_dnu(S.rt, true);
        double oe[2] = {okf ? 0.0 : 1.0, capped_x ? 1.0 : 0.0};
        seg_reduce<2, 0, M::SEG_SKIP, SHORT>(oe, nullptr, k, lpi, base);
        okall = oe[0] < 0.5;
        const bool extrap = oe[1] > 0.5;   // per instance; the second solve runs for the wavefront when any of its instances needs it
        if (__any(extrap)) {
            double y1x[NX], y1n[NX];
            const double y1u = S.Du[0];
#pragma unroll
            for (int i = 0; i < NX; ++i) y1x[i] = S.Dx[i], y1n[i] = S.Dnu[i];
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                double d = 0.0;
#pragma unroll
                for (int sd = 0; sd < 2; ++sd)
                    if (S.has(sd, i)) d += fmin(S.lam[sd][i] / S.t[sd][i], 0.5 * SENS_W_MAX);
                S.Dg[i] = d;
            }
            const bool okf2 = S.template mx_pred<true>(Hs, S.rt, zero);
            S.mx_dnu(S.rt, true);
            const bool ok2 = seg_max<M::SEG_SKIP, SHORT>(okf2 ? 0.0 : 1.0, k, lpi, base) < 0.5;
            okall = okall && (ok2 || !extrap);
            if constexpr (BOUNDS) bound_rows(y1x, &y1u, extrap), rows_done = true;   // (before the two solutions are merged)
            S.Du[0] = extrap ? fma(2.0, y1u, -S.Du[0]) : y1u;
#pragma unroll
            for (int i = 0; i < NX; ++i)
                S.Dx[i] = extrap ? fma(2.0, y1x[i], -S.Dx[i]) : y1x[i], S.Dnu[i] = extrap ? fma(2.0, y1n[i], -S.Dnu[i]) : y1n[i];
        }
    } else {
        const bool okf = S.backward(Hs, S.rt, zero);
        okall = seg_max<M::SEG_SKIP, SHORT>(okf ? 0.0 : 1.0, k, lpi, base) < 0.5;
        S.forward_scan(zero);
    }
    if constexpr (BOUNDS)
        if (!rows_done) bound_rows(S.Dx, S.Du, false);
    if constexpr (COST::ON) cost(S, inst, valid, sv, okall);   // (after the two solutions are merged: the product is linear in y)
    double ynn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) ynn[i] = lane_dn(S.Dnu[i]);
    // x_0 itself is x0, and the solve had the right-hand side -G, so the product is minus the sums.
    if (a.g_x0) {
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const double s = S.dx0_contract(Hx, ynn, j);
            if (first && valid) a.g_x0[inst * NX + j] = sv ? (okall ? gx0[j] - s : NAN) : 0.0;
        }
    }
    if (!a.g_theta) return;   // (wave-uniform)
    double sums[NT];
    S.dtheta_contract(nun, ynn, sums, nullptr);
    seg_reduce<0, NT, M::SEG_SKIP, SHORT>(nullptr, sums, k, lpi, base);
#pragma unroll
    for (int d = 0; d < NTD; ++d)
        if (first && valid) a.g_theta[inst * NP + M::td_index(d)] = sv ? (okall ? -sums[d] : NAN) : 0.0;
#pragma unroll
    for (int d = 0; d < NTC; ++d)
        if (first && valid) a.g_theta[inst * NP + M::tc_index(d)] = sv ? (okall ? -sums[NTD + d] : NAN) : 0.0;
    // the entries of p the pass has no gradient for; the two sets of addresses are disjoint
    if (valid)
        for (int e = k; e < NP; e += lpi)
            if (!M::p_has_gradient(e)) a.g_theta[inst * NP + e] = 0.0;
}

template <class M, bool SHORT = false>
__global__ void __launch_bounds__(64) small_traj_vjp_kernel(const SmallSpec sp, const TrajVjpArgs a) {
    small_traj_vjp_body<M, SHORT, false>(sp, a, nullptr, nullptr);
}

}  // namespace mpcrl
