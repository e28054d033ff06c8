// traj_jvp_kernel.hpp — Jacobian-vector product of a solve's whole planned trajectory (include/mpcrl_traj_jvp_ext.h, mpcrl_traj_jvp),
// on the iterate (x, u, pi, lam, t) a solve kernel stored:
//
//   small_traj_jvp_kernel<M, S>    for R directions (dx0 [nx], dtheta [np]) per instance of the cartpole and the linear system:
//                                  dX[k] = dx_k*/dx0 dx0 + dx_k*/dtheta dtheta and dU[k], the same for u_k*.
//
// The forward mode of small_traj_vjp_kernel (traj_vjp_kernel.hpp): the same KKT matrix K of the du0*/dp pass
// (SmallSolver::kkt_assemble / kkt_solve, small_kernel.hpp), solved once with the right-hand side
// -(dR/dtheta dtheta + dR/dx0 dx0), and the primal part of the solution written out.
// In the solver's terms, min 1/2 Dv' H Dv + g' Dv subject to Dx_{k+1} = A Dx_k + B Du_k + bb_k with, on stage lane k,
//     bb_k   = dF_k/dtheta dtheta                          (k < N)           + A_0 dx0 on stage 0
//     g_k[i] = sum_m nu_{k+1,m} d2 F_{k,m} / dv_i dtheta dtheta
//              + d(c_k grad_{v_i} l_k)/dtheta dtheta                         + sum_j Hx(u_i, x_j) dx0_j on the u rows of stage 0
// and (Dx, Du) is +dw*.  The two dynamics terms are ONE Jet2<NW> evaluation of the discrete map: outer tangents on the coordinates of
// v = [u; x], the inner tangent dtheta on the parameter jets, so jn[m].e is bb_k and sum_m nu_{k+1,m} jn[m].m[i] the first term of
// g_k[i].  The cost term exists on the linear system only (V_0, f); M::cost_mixed is linear in y, so the unit vectors e_i give the mixed
// derivatives.  x_0 is eliminated as in the VJP: its lane solves with Dx_0 = 0 and the output row dX[0] is dx0 itself.  Of dtheta only
// the entries M::td_index(i) and M::tc_index(i) are read, the entries g_theta of the VJP is non-zero at; the rest (the cartpole's cost
// block) is ignored.
//
// Lane layout, loads, the "solved" rule and the linearisation are those of small_traj_vjp_body.  Work item j = inst R + r takes
// the place the instance has there; every item linearises and factors for itself.  The packing order of the handle is not used.
#pragma once
#include "state_sens_kernel.hpp"

namespace mpcrl {

struct TrajJvpArgs {
    IterateArgs it;                          // (perm is not read)
    int R;
    const double *dx0, *dth;                 // directions [B, R, nx] / [B, R, np]; null = zeros
    double *dX, *dU;                         // [B, R, N + 1, nx] / [B, R, N, nu]; either may be null
};

// Every requested row is written in full: zeros for an item whose instance holds no solved iterate, NaN where the factorisation met a
// non-positive pivot.
template <class M, bool SHORT = false>
__global__ void __launch_bounds__(64) small_traj_jvp_kernel(const SmallSpec sp, const TrajJvpArgs a) {
    using SS = SmallSolver<M, SHORT>;
    constexpr int NX = M::NX, NU = M::NU, NW = NX + NU, NTD = M::NTD, NTC = M::NTC;
    const int lane = threadIdx.x;
    const int N = sp.N, lpi = N + 1, ipw = min(64 / lpi, M::MAX_IPW);
    const int slot = lane / lpi, k = lane - slot * lpi, base = slot * lpi;
    const long items = (long)a.it.B * a.R;
    long item = (long)blockIdx.x * ipw + slot;
    const bool valid = slot < ipw && item < items;
    if (!valid) item = items - 1;
    const long inst = item / a.R;
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
    // (lanes past the last item slot shadow another item: they get a slot of their own)
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
    // the direction of this item
    double dx0[NX], dtd[NTD], dtc[NTC > 0 ? NTC : 1];
#pragma unroll
    for (int i = 0; i < NX; ++i) dx0[i] = a.dx0 ? a.dx0[item * NX + i] : 0.0;
#pragma unroll
    for (int i = 0; i < NTD; ++i) dtd[i] = a.dth ? a.dth[item * M::NP + M::td_index(i)] : 0.0;
#pragma unroll
    for (int i = 0; i < NTC; ++i) dtc[i] = a.dth ? a.dth[item * M::NP + M::tc_index(i)] : 0.0;
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
    // the Hessian fill of SmallSolver::kkt_assemble in this kernel's own text: through the shared function the cartpole
    // instantiations spill 92 bytes of scratch per lane instead of 76 (profiles/sens_kkt_kernel_resources.txt)
    double Hx[SS::NHT];
#pragma unroll
    for (int i = 0; i < NW; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Hx[SS::sym(i, j)] = S.ck * S.hess_of_stage(i, j);
#pragma unroll
    for (int di = 0; di < M::NLD; ++di)
#pragma unroll
        for (int dj = 0; dj <= di; ++dj) Hx[SS::sym(M::lin_coord(di), M::lin_coord(dj))] += hdd[di * (di + 1) / 2 + dj];
    const bool capped_x = S.barrier_diag(SENS_W_MAX);
    S.hscale = 1.0;
    // the right-hand side: (dR/dtheta dtheta + dR/dx0 dx0) of this stage, stationarity rows in S.rt and dynamics rows in bb
    double bb[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) bb[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) S.rt[i] = 0.0;
    if (!term) {
        Jet2<NW> jx[NX], ju[NU], jt[NTD], jn[NX];
#pragma unroll
        for (int i = 0; i < NU; ++i) ju[i] = Jet2<NW>(S.u[i]), ju[i].g[i] = 1.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) jx[i] = Jet2<NW>(S.x[i]), jx[i].g[NU + i] = 1.0;
#pragma unroll
        for (int i = 0; i < NTD; ++i) jt[i] = Jet2<NW>(S.thd[i]), jt[i].e = dtd[i];
        disc_map<M, Jet2<NW>>(jx, ju, jt, jn, sp.h, sp.rk_steps);
#pragma unroll
        for (int m = 0; m < NX; ++m) bb[m] = jn[m].e;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; ++m) s = fma(nun[m], jn[m].m[i], s);
            S.rt[i] = s;
        }
    }
    if constexpr (NTC > 0) {   // d(c grad_v l)/d(cost parameters) dtheta, column by column (cost_mixed is linear in y and adds sc * ...)
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            double e[NW], outc[NTC];
#pragma unroll
            for (int j = 0; j < NW; ++j) e[j] = j == i ? 1.0 : 0.0;
#pragma unroll
            for (int d = 0; d < NTC; ++d) outc[d] = 0.0;
            M::cost_mixed(term, e, S.ck, outc);
            double s = S.rt[i];
#pragma unroll
            for (int d = 0; d < NTC; ++d) s = fma(outc[d], dtc[d], s);
            S.rt[i] = s;
        }
    }
    // x_0 is eliminated: dx0 enters the stationarity row of u_0 through d2 l0 / du dx and the dynamics row F(x0, u_0) - x_1 through A_0
    // (small_state_sens_kernel and the VJP's g_x0 contract with this block transposed); the x rows of stage 0 are not unknowns
    if (first) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            double s = S.rt[i];
#pragma unroll
            for (int j = 0; j < NX; ++j) s = fma(Hx[SS::sym(i, NU + j)], dx0[j], s);
            S.rt[i] = s;
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            double s = bb[m];
#pragma unroll
            for (int j = 0; j < NX; ++j) s = fma(S.Aget(m * NX + j), dx0[j], s);
            bb[m] = s;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) S.rt[NU + i] = 0.0;
    }
    if (term) {
#pragma unroll
        for (int i = 0; i < NU; ++i) S.rt[i] = 0.0;
    }
    bool okall = true;
    S.template kkt_solve<false>(Hx, bb, capped_x, 0, okall);
    if (!valid) return;
    if (a.dX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const double v = first ? dx0[i] : S.Dx[i];
            a.dX[(item * (N + 1) + k) * NX + i] = sv ? (okall ? v : NAN) : 0.0;
        }
    }
    if (a.dU && !term) {
#pragma unroll
        for (int i = 0; i < NU; ++i) a.dU[(item * N + k) * NU + i] = sv ? (okall ? S.Du[i] : NAN) : 0.0;
    }
}

}  // namespace mpcrl
