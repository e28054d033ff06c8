// chain_jvp_rhs.hpp — the right-hand side of the chain's trajectory JVP (include/mpcrl_chain_traj_jvp_ext.h) for ONE stage and ONE
// direction dtheta of the parameters, on the point tables of chain_point_kernel<M, true>: the exact transpose of the map
// chain_sens_mix2_kernel applies to an adjoint solution (y_x, y_u, y_nu) of that stage,
//     term2 = y_v' d/dv grad_theta (nu' F) + y_nu' dF/dtheta          (mix2)
//     b = dF/dtheta dtheta,      g = d/dtheta [grad_v (nu_{k+1}' F_k)] dtheta          (here; v = [u; x] fixed)
// so that term2 . dtheta = y_x . g_x + y_u . g_u + y_nu . b for every table content — every line below is the transposed line of
// mix2, and the sums have its coefficients.  Read the other way round it is forward over reverse on the tables:
//   1. b: the RK4 tangent of the evaluation states along dtheta — ode_tan with zero start and control tangent plus, at every
//      evaluation point, the parameter source of the link forces (m, D, L through the spring term, C through the velocity
//      differences) and of the disturbance w, which enters the accelerations directly;
//   2. g: the tangent of the reverse sweep of nu_{k+1} through the same points — the linear recursion ode_tan_T on the tangent
//      adjoints (zero at the start: nu is fixed) with, per evaluation point and link, the sources
//        (d dist / dx)' G_{e,i} d dist_{e,i}                       from the state tangents of 1., as in mix2's step 2,
//        (d dist / dx)' d/dtheta [(dFs / d dist)' q_{e,i}]           the dtheta-derivative of the recursion's own coefficients,
//        (d dv / d(x, u))' (dC q_{e,i})                             the same for the damping term; the last link's dv reads u.
// As in mix2 the evaluation states are recomputed where the reverse sweep needs them (one state, one ODE tangent and the adjoint vectors
// live; runtime loops over the evaluation points on purpose); the start state of the second RK4 step and the two vectors of the reverse
// sweep that are touched once per evaluation point are per-lane scratch (3 NX doubles, LDS in the kernel).  dtheta is read where it is
// used, indexed like p (no NTD-wide per-lane copy): the lanes of an instance read the same addresses.
#pragma once
#include "models_dev.hpp"

namespace mpcrl {

// An opaque copy of a pointer inside a loop body: what is loaded through it cannot be hoisted out of the loops over the evaluation
// points (th and dtheta are loop invariants: hoisted, 20 NL doubles of them stay live per lane through the whole kernel).
#ifndef MPCRL_JVP_OPAQUE
#define MPCRL_JVP_OPAQUE(ptr) asm volatile("" : "+v"(ptr))
#endif

// tab / Gt / qv: the stage's slices of ptab / gtab / qvtab; th: the instance's p; dth: the direction, indexed like p (only the
// dynamics entries m, D, L, C, w are read); scr(slot, i): per-lane scratch, three slots of NX doubles (the start state of the second
// RK4 step, the tangent adjoint the step started from, its running sum); b[NX]: the dynamics row; g[NU + NX]: the stationarity
// rows in stage-vector order [u; x].  rk_steps is 1 or 2 (the tables hold eight evaluation points).
template <class M, class Scratch>
MPCRL_DI void chain_jvp_rhs_lane(const double *tab, const double *Gt, const double *qv, const double *th, const double *dth, const double h,
                                 const int steps, Scratch scr, double *b, double *g) {
    constexpr int NX = M::NX, NU = M::NU, NL = M::NL, TAB2 = M::TAB2, MM = M::M;
    const double *Cp = th + 7 * NL;
    const double zu[NU] = {0.0, 0.0, 0.0};
    // ODE tangent along (dX, dtheta) at evaluation point e: the state part on the tables, the parameter source of every link force
    auto tan_src = [&](int e, const double (&dX)[NX], double (&dk)[NX]) {
        const double *tb = tab + (size_t)e * NL * TAB2, *thl = th, *dthl = dth;
        MPCRL_JVP_OPAQUE(thl);
        MPCRL_JVP_OPAQUE(dthl);
        const double *mp = thl, *Dp = thl + NL, *Lp = thl + 4 * NL;
        const double *dmp = dthl, *dDp = dthl + NL, *dLp = dthl + 4 * NL, *dCp = dthl + 7 * NL, *dwp = dthl + M::OFF_W;
        M::template ode_tan<TAB2, false>(tb, th, dX, zu, dk, nullptr);
        double *dacc = dk + 3 * (MM + 1);
#pragma unroll
        for (int i = 0; i < 3 * MM; ++i) dacc[i] += dwp[i];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const double *t = tb + i * TAB2, *dv = qv + ((size_t)e * NL + i) * 6 + 3;
            const double inrm = sqrt(t[12] * (1.0 / 3.0)), im = 1.0 / mp[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double Lj = Lp[3 * i + j], kap = Dp[3 * i + j] * im, dkap = im * (dDp[3 * i + j] - kap * dmp[i]);
                const double sg = dkap * (1.0 - Lj * inrm) - kap * (dLp[3 * i + j] * inrm);
                const double sF = fma(sg, t[j], dCp[3 * i + j] * dv[j]);
                if (i < MM) dacc[3 * (i < MM ? i : 0) + j] -= sF;
                if (i > 0) dacc[3 * (i > 0 ? i - 1 : 0) + j] += sF;
            }
        }
    };
    auto start = [&](int s, int i) { return s == 0 ? 0.0 : scr(0, i); };      // start-state tangent of step s
    auto state_at = [&](int s, int n, double (&dX)[NX]) {                  // evaluation state n (0..3) of step s
#pragma unroll
        for (int i = 0; i < NX; ++i) dX[i] = start(s, i);
#pragma unroll 1
        for (int m = 0; m < n; ++m) {
            double dk[NX];
            tan_src(4 * s + m, dX, dk);
            const double c = m == 2 ? h : 0.5 * h;
#pragma unroll
            for (int i = 0; i < NX; ++i) dX[i] = start(s, i) + c * dk[i];
        }
    };
    // 1. the dynamics row: RK4 of the tangent, one step at a time
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        double dX[NX], acc[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) dX[i] = start(s, i), acc[i] = 0.0;
#pragma unroll 1
        for (int m = 0; m < 4; ++m) {
            double dk[NX];
            tan_src(4 * s + m, dX, dk);
            const double c = m == 2 ? h : 0.5 * h, wgt = (m == 0 || m == 3) ? 1.0 : 2.0;
#pragma unroll
            for (int i = 0; i < NX; ++i) acc[i] = fma(wgt, dk[i], acc[i]), dX[i] = start(s, i) + c * dk[i];
        }
        if (s + 1 < steps) {
#pragma unroll
            for (int i = 0; i < NX; ++i) scr(0, i) = start(s, i) + (h / 6.0) * acc[i];
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) b[i] = start(s, i) + (h / 6.0) * acc[i];
        }
    }
    // 2. the stationarity rows: the tangent of the reverse sweep
    double gu[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) scr(1, i) = 0.0;
#pragma unroll
    for (int c = 0; c < NU; ++c) gu[c] = 0.0;
#pragma unroll 1
    for (int s = steps - 1; s >= 0; --s) {
        double kbd[NX], Xbd[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) scr(2, i) = scr(1, i), Xbd[i] = 0.0;
#pragma unroll 1
        for (int n = 3; n >= 0; --n) {
            const double ca = (n == 3 || n == 0) ? h / 6.0 : h / 3.0, cb = n == 3 ? 0.0 : (n == 2 ? h : 0.5 * h);
#pragma unroll
            for (int i = 0; i < NX; ++i) kbd[i] = ca * scr(1, i) + cb * Xbd[i];
            const int e = 4 * s + n;
            const double *tb = tab + (size_t)e * NL * TAB2;
            double qd[3 * NL], dX[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) Xbd[i] = 0.0;
            M::template ode_tan_T<TAB2>(tb, th, kbd, Xbd, qd);
#pragma unroll
            for (int j = 0; j < 3; ++j) gu[j] += fma(Cp[3 * MM + j], qd[3 * MM + j], kbd[3 * MM + j]);      // (df/du)' kbd
            state_at(s, n, dX);
            const double *thl = th, *dthl = dth;
            MPCRL_JVP_OPAQUE(thl);
            MPCRL_JVP_OPAQUE(dthl);
            const double *mp = thl, *Dp = thl + NL, *Lp = thl + 4 * NL;
            const double *dmp = dthl, *dDp = dthl + NL, *dLp = dthl + 4 * NL, *dCp = dthl + 7 * NL;
            double *posb = Xbd, *velb = Xbd + 3 * (MM + 1);
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const double *t = tb + i * TAB2, *G = Gt + ((size_t)e * NL + i) * 6, *q = qv + ((size_t)e * NL + i) * 6;
                double dd[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) dd[j] = i ? dX[3 * i + j] - dX[3 * (i > 0 ? i - 1 : 0) + j] : dX[j];
                const double wv[3] = {G[0] * dd[0] + G[1] * dd[1] + G[3] * dd[2], G[1] * dd[0] + G[2] * dd[1] + G[4] * dd[2],
                                      G[3] * dd[0] + G[4] * dd[1] + G[5] * dd[2]};
                const double inrm = sqrt(t[12] * (1.0 / 3.0)), im = 1.0 / mp[i];
                double sg[3], sb = 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double Lj = Lp[3 * i + j], kap = Dp[3 * i + j] * im, dkap = im * (dDp[3 * i + j] - kap * dmp[i]);
                    sg[j] = dkap * (1.0 - Lj * inrm) - kap * (dLp[3 * i + j] * inrm);
                    sb = fma(q[j] * t[j], dkap * Lj + kap * dLp[3 * i + j], sb);
                }
                sb *= inrm * inrm * inrm;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double ddb = wv[j] + fma(q[j], sg[j], t[j] * sb), dvb = q[j] * dCp[3 * i + j];
                    posb[3 * i + j] += ddb;
                    if (i > 0) posb[3 * (i > 0 ? i - 1 : 0) + j] -= ddb;
                    if (i < MM) velb[3 * (i < MM ? i : 0) + j] += dvb;
                    else gu[j] += dvb;
                    if (i > 0) velb[3 * (i > 0 ? i - 1 : 0) + j] -= dvb;
                }
                }
#pragma unroll
            for (int i = 0; i < NX; ++i) scr(2, i) += Xbd[i];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) scr(1, i) = scr(2, i);
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) g[c] = gu[c];
#pragma unroll
    for (int i = 0; i < NX; ++i) g[NU + i] = scr(1, i);
}

}  // namespace mpcrl
