// cost_vjp_kernel.hpp — derivatives of a cartpole solve with respect to its tracking cost (include/mpcrl_cost_ext.h), on the iterate
// (x, u, pi, lam, t) a solve kernel stored:
//
//   small_cost_vjp_kernel<M, S>     mpcrl_cost_vjp: small_bound_vjp_kernel (ONE adjoint solve y = K^-1 [G; 0] for a cotangent G on the
//                                   whole plan, g_x0, g_theta, g_lb, g_ub) plus, on the stage lane that already holds x, u, the cost
//                                   table and y, the contraction with the stage's cost residual (CostVjpOut, the COST hook of
//                                   small_traj_vjp_body).
//   cost_value_grad_kernel<M>       mpcrl_cost_value_grad: dV/dcost from the stored X, U and theta.
//
// Unscaled stage cost l = 1/2 r' W r, r = y - yref, y = [x; u] (y = x on stage N); every entry of (W, yref) is an independent variable
// and the solve uses H = 1/2 (W + W') (M::hess).  A cost parameter enters the KKT residual only through grad_v l_k = H r:
//     d(H r)_i / dW[a, b] = 1/2 (d_ia r_b + d_ib r_a),     d(H r) / dyref[a] = -H[:, a],
// so with the adjoint solution y of the right-hand side -G (the product is minus the sums, as for g_theta) and c_k = S.ck
//     G' dw*/dW[a, b] = -sum_k c_k 1/2 (y_a r_b + y_b r_a),     G' dw*/dyref[a] = +sum_k c_k (H y)_a,
//     dV/dW[a, b]     =  sum_k c_k 1/2 r_a r_b,                 dV/dyref[a]     = -sum_k c_k (H r)_a,
// each sum over the stages of the block: stage 0 for (W_0, yref_0), stages 1 .. N - 1 for (W, yref), stage N for (W_e, yref_e).
#pragma once
#include "bound_vjp_kernel.hpp"

namespace mpcrl {

// The COST hook of small_traj_vjp_body.  Every lane forms the 15 + 5 products of its own stage (the W gradient is symmetric) in
// stage-vector order v = [u; x]; stage 0 and stage N write theirs to their own blocks, the interior lanes' are summed in ONE
// segmented tree for all 20 (a cross-lane round trip per level whatever the count, small_kernel.hpp seg_reduce) and written by the
// first lane.  A row is written in full: exact zeros on the dynamics block, zeros for an instance without a solved iterate, NaN on
// the cost block where the factorisation met a non-positive pivot.  Shadow lanes (!valid) write nothing.
template <class M, bool SHORT>
struct CostVjpOut {
    static constexpr bool ON = true;
    double *g_cost;   // [B, np]

    template <class SS>
    MPCRL_DI void operator()(const SS &S, long inst, bool valid, bool sv, bool okall) const {
        constexpr int NU = M::NU, NW = M::NX + M::NU, NX = M::NX, NHT = SS::NHT, NS = NHT + NW;
        double yv[NW], r[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) yv[i] = S.dvc(S.Dx, S.Du, i), r[i] = S.vc(i) - S.ctab[NHT + i];
        double own[NS], sums[NS];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) own[SS::sym(i, j)] = -(S.ck * (0.5 * fma(yv[i], r[j], yv[j] * r[i])));
            double hy = 0.0;
#pragma unroll
            for (int j = 0; j < NW; ++j) hy = fma(S.hess_of_stage(i, j), yv[j], hy);
            own[NHT + i] = S.ck * hy;
        }
        const bool interior = !S.first && !S.term;
#pragma unroll
        for (int e = 0; e < NS; ++e) sums[e] = interior ? own[e] : 0.0;
        seg_reduce<0, NS, M::SEG_SKIP, SHORT>(nullptr, sums, S.k, S.lpi, S.base);
        if (!valid) return;
        double *o = g_cost + inst * M::NP;
        auto out = [&](double v) { return sv ? (okall ? v : NAN) : 0.0; };
        if (S.first) {
#pragma unroll
            for (int e = 0; e < M::NTD; ++e) o[M::td_index(e)] = 0.0;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    const double v0 = out(own[SS::sym(i, j)]), v1 = out(sums[SS::sym(i, j)]);
                    o[M::P_W0 + M::yi(j) * NW + M::yi(i)] = v0, o[M::P_W0 + M::yi(i) * NW + M::yi(j)] = v0;
                    o[M::P_W + M::yi(j) * NW + M::yi(i)] = v1, o[M::P_W + M::yi(i) * NW + M::yi(j)] = v1;
                }
                o[M::P_YREF0 + M::yi(i)] = out(own[NHT + i]);
                o[M::P_YREF + M::yi(i)] = out(sums[NHT + i]);
            }
        }
        if (S.term) {
#pragma unroll
            for (int i = NU; i < NW; ++i) {
#pragma unroll
                for (int j = NU; j <= i; ++j) {
                    const double v = out(own[SS::sym(i, j)]);
                    o[M::P_WE + (j - NU) * NX + (i - NU)] = v, o[M::P_WE + (i - NU) * NX + (j - NU)] = v;
                }
                o[M::P_YREFE + i - NU] = out(own[NHT + i]);
            }
        }
    }
};

struct CostVjpArgs {
    BoundVjpArgs b;      // what small_bound_vjp_kernel takes; all four outputs may be null here
    double *g_cost;      // [B, np], not null
};

template <class M, bool SHORT = false>
__global__ void __launch_bounds__(64) small_cost_vjp_kernel(const SmallSpec sp, const CostVjpArgs a) {
    small_traj_vjp_body<M, SHORT, true, CostVjpOut<M, SHORT>>(sp, a.b.t, a.b.g_lb, a.b.g_ub, CostVjpOut<M, SHORT>{a.g_cost});
}

struct CostValueArgs {
    int B, N, theta_stride, cost_kind;
    double dT, gamma;
    const double *theta;             // [np] or [B, np]
    const double *X, *U, *PI, *RES;  // stored iterate, layouts of mpcrl_get_iterate
    double *dV;                      // [B, np]
};

// One wavefront per instance: all 64 lanes scan the instance's iterate for the "solved" rule of stage0_grad_kernel and leave the
// residuals r_k = y_k - yref of every stage in LDS (N + 1 <= 64 stages, as in every small-model kernel), then a lane per entry of p
// (in strides of 64) sums over the stages of the entry's block.  dV/dyref[a] = -sum_j H[a, j] (sum_k c_k r_k[j]): the weight is
// read once per entry, not once per stage.  W[a, b] and W[b, a] run the same operations on the same operands (r_a r_b commutes), so
// they hold the same bits.
template <class M>
__global__ void __launch_bounds__(64) cost_value_grad_kernel(const CostValueArgs a) {
    constexpr int NX = M::NX, NU = M::NU, NY = NX + NU, NP = M::NP;
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
    __shared__ double r_lds[64 * NY];   // r_k[i] at k * NY + i, y order; the control part of stage N is 0
    for (int e = c; e < (N + 1) * NY; e += 64) {
        const int k = e / NY, i = e - k * NY;
        const double y = i < NX ? X[k * NX + i] : (k < N ? U[k * NU + (i - NX)] : 0.0);
        const double yr = k == N ? (i < NX ? p[M::P_YREFE + i] : 0.0) : p[(k == 0 ? M::P_YREF0 : M::P_YREF) + i];
        r_lds[e] = y - yr;
    }
    __syncthreads();
    for (int e = c; e < NP; e += 64) {
        double v = 0.0;
        if (solved && e >= M::P_W0) {
            // the entry's block: its weight in p, its side (4 on stage N, 5 otherwise), its stages k0 .. k1
            const bool isW = e < M::P_YREF0;
            const int kind = isW ? (e < M::P_W ? 0 : (e < M::P_WE ? 1 : 2)) : (e < M::P_YREF ? 0 : (e < M::P_YREFE ? 1 : 2));
            const int pW = kind == 0 ? M::P_W0 : (kind == 1 ? M::P_W : M::P_WE);
            const int n = kind == 2 ? NX : NY;
            const int k0 = kind == 0 ? 0 : (kind == 1 ? 1 : N), k1 = kind == 0 ? 0 : (kind == 1 ? N - 1 : N);
            const int idx = e - (isW ? pW : (kind == 0 ? M::P_YREF0 : (kind == 1 ? M::P_YREF : M::P_YREFE)));
            const int ia = isW ? idx % n : idx, ib = isW ? idx / n : 0;
            auto ck = [&](int k) {
                if (a.cost_kind == 0) return k == N ? 1.0 : a.dT;
                return k == 0 ? a.dT : (k == N ? pow(a.gamma, (double)N) : pow(a.gamma, (double)k) * a.dT);
            };
            if (isW) {
                for (int k = k0; k <= k1; ++k) v = fma(ck(k), 0.5 * (r_lds[k * NY + ia] * r_lds[k * NY + ib]), v);
            } else {
                for (int j = 0; j < n; ++j) {
                    double sj = 0.0;
                    for (int k = k0; k <= k1; ++k) sj = fma(ck(k), r_lds[k * NY + j], sj);
                    v = fma(-0.5 * (p[pW + j * n + ia] + p[pW + ia * n + j]), sj, v);
                }
            }
        }
        a.dV[inst * NP + e] = v;
    }
}

}  // namespace mpcrl
