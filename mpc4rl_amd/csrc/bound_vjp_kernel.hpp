// bound_vjp_kernel.hpp — derivatives of a solve with respect to its box bounds (include/mpcrl_bound_ext.h), on the iterate
// (x, u, pi, lam, t) a solve kernel stored:
//
//   small_bound_vjp_kernel<M, S>     mpcrl_bound_vjp on the cartpole and the linear system: small_traj_vjp_kernel (ONE adjoint solve
//                                    y = K^-1 [G; 0] for a cotangent G on the whole plan, g_x0, g_theta) plus, on the stage lane that
//                                    already holds lam, t, has() and y, the contraction with the bound rows.
//   bound_value_grad_kernel<M>       mpcrl_bound_value_grad, all three models: dV/dlb = lam_l, dV/dub = -lam_u from the stored planes.
//
// A bound b of side sd on coordinate i of stage k enters the KKT residual R = [grad_w L; g; h + t; lam t - tau] only through its own row
// h + t, h = sgn (v_k[i] - b) [- slack]: dR/db = -sgn there.  Eliminating (lam, t) of that row from (dR/dz) dz = -dR/db leaves the
// right-hand side (lam / t) e_{v_k[i]} on the reduced system K for EITHER side (sgn^2), so for a cotangent G on w = (U, X)
//     G' dw*/dlb[k, i] = (lam_l / t_l)[k, i] y_v[k, i],     G' dw*/dub[k, i] = (lam_u / t_u)[k, i] y_v[k, i],     y = K^-1 [G; 0],
// and, V being the Lagrangian at the KKT point, dV/dlb[k, i] = lam_l[k, i] and dV/dub[k, i] = -lam_u[k, i].  Soft rows as the du0*/dp
// pass treats them: their slacks are constants (quirk q1 of the reference's mirror), so a soft row is a row like any other here.
//
// The weight in the product is the one the solve used, min(lam / t, SENS_W_MAX).  Where the cartpole pass extrapolates (a capped state
// row), each of the two solves is contracted with its own capped diagonal and the PRODUCTS are extrapolated, 2 w1 y(W) - w2 y(W / 2):
// on a capped row y = a / c + b / c^2 + ..., so c y = a + b / c, and only the extrapolation of the product removes b / c.
//
// Active state rows.  There y_x is the small difference of O(1) terms of the forward sweep, multiplied by up to 1e9.  This kernel
// forms the product directly, w y_v[i], as on every other row; the alternative — the same quantity from the stationarity row of the
// adjoint system, G[i] - (H y_v)[i] - ([B A]' y_pi,k+1)[i] + y_pi,k[i], free of that cancellation — was not built: the direct product
// is 4e-12 .. 9e-8 from the mirror on every fixture instance with an active hard state row (cartpole N 15 .. 63, runs of up to 11
// active stages) at a bar of 1e-6 (MEASURED in tests/test_gpu_bound_vjp.py), so the second form's error is not measured.
#pragma once
#include "traj_vjp_kernel.hpp"

namespace mpcrl {

struct BoundVjpArgs {
    TrajVjpArgs t;             // what small_traj_vjp_kernel takes; g_x0 and g_theta may both be null here
    double *g_lb, *g_ub;       // [B, N + 1, nu + nx]; either may be null
};

// Every requested row is written in full, as small_traj_vjp_kernel writes its own: values for an instance with a solved iterate, zeros
// otherwise and where no bound row exists, NaN where the factorisation met a non-positive pivot.
template <class M, bool SHORT = false>
__global__ void __launch_bounds__(64) small_bound_vjp_kernel(const SmallSpec sp, const BoundVjpArgs a) {
    small_traj_vjp_body<M, SHORT, true>(sp, a.t, a.g_lb, a.g_ub);
}

constexpr int BOUND_MAXNW = 40;   // >= LARGE_MAXNW, SMALL_MAXNW

struct BoundValueArgs {
    int B, N, theta_stride;
    bool qmode;
    const double *theta;                     // [np] or [B, np]
    const double *X, *U, *PI, *BND, *RES;    // stored iterate, layouts of mpcrl_get_iterate
    unsigned char rows[3][BOUND_MAXNW];      // bit sd of rows[g][i]: the handle has the bound of side sd on coordinate i of v = [u; x]
                                             // in group g (0 stage 0, 1 stages 1 .. N - 1, 2 stage N), stage kind and mode included
    double *dlb, *dub;                       // [B, N + 1, nu + nx]; either may be null
};

// One wavefront per instance: all 64 lanes scan the instance's iterate for the "solved" rule of stage0_grad_kernel, then a lane per
// entry (in strides of 64) copies the multiplier with its sign, or writes the zero of an entry without a row / an unsolved instance.
template <class M>
__global__ void __launch_bounds__(64) bound_value_grad_kernel(const BoundValueArgs a) {
    constexpr int NX = M::NX, NU = M::NU, NW = NX + NU;
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
    const size_t nb = (size_t)(N + 1) * NW;
    const double *bnd = a.BND + (size_t)inst * 10 * nb;
    for (int e = c; e < (int)nb; e += 64) {
        const int k = e / NW, i = e - k * NW;
        const unsigned char m = a.rows[k == 0 ? 0 : (k == N ? 2 : 1)][i];
        if (a.dlb) a.dlb[inst * nb + e] = (solved && (m & 1)) ? bnd[e] : 0.0;
        if (a.dub) a.dub[inst * nb + e] = (solved && (m & 2)) ? -bnd[nb + e] : 0.0;
    }
}

}  // namespace mpcrl
