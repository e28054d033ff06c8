// Probe of the dynamics jets (mpcrl_debug_model_jets; tests/test_gpu_model_jets.py): one lane per evaluation point runs the discrete
// map disc_map<M, J> of models_dev.hpp with the jets of jet.hpp seeded as the four evaluations of small_kernel.hpp seed them, and
// stores every block the evaluation yields.  Nothing here is on a hot path and nothing of the kernels is shared with it: the probe
// calls the same templates with the same seeds, so a change to a jet, to a model's ode() or to the RK4 map shows up here block by
// block, at rounding level.
//   WHICH 0: Jet1<NLD>   linearize<false>    row = F[NX], BA[NX][NW] (v = [u; x], closed-form columns included)
//   WHICH 1: JetH<NLD>   linearize<true>     row = F, BA, H[NX][NLD (NLD + 1) / 2], hdd[NLD (NLD + 1) / 2];  aux = nu [n][NX]
//   WHICH 2: Jet1<NTD>   sensitivities()     row = F, Fth[NX][NTD]
//   WHICH 3: Jet2<NTD>   sensitivities()     row = F, e[NX], g[NX][NTD], m[NX][NTD];                          aux = y [n][NW]
#pragma once
#include <type_traits>

#include "jet.hpp"
#include "models_dev.hpp"

namespace mpcrl {

template <class M, int WHICH>
struct JetProbeRow {
    static constexpr int NX = M::NX, NW = M::NX + M::NU, NTD = M::NTD, NH = M::NLD * (M::NLD + 1) / 2;
    static constexpr int SIZE = WHICH == 0 ? NX + NX * NW : WHICH == 1 ? NX + NX * NW + NX * NH + NH : WHICH == 2 ? NX + NX * NTD : 2 * NX + 2 * NX * NTD;
};

template <class M, int WHICH>
__global__ void __launch_bounds__(64) jet_probe_kernel(int n, double h, int rk_steps, const double *xg, const double *ug, const double *thg,
                                                       const double *aux, double *outg) {
    constexpr int NX = M::NX, NU = M::NU, NW = NX + NU, NTD = M::NTD, ND = M::NLD, NH = ND * (ND + 1) / 2;
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    double x[NX], u[NU], thd[NTD];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xg[p * NX + i];
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = ug[p * NU + i];
#pragma unroll
    for (int i = 0; i < NTD; ++i) thd[i] = thg[p * NTD + i];
    double *out = outg + p * JetProbeRow<M, WHICH>::SIZE;
    if constexpr (WHICH == 0 || WHICH == 1) {
        constexpr bool WITH_H = WHICH == 1;
        double *BA = out + NX;
        // small_kernel.hpp linearize<WITH_H>():  J jx[NX], ju[NU], jt[NTD], jn[NX];  ju[i] = J(u[i]);  jx[i] = J(x[i]);
        using J = std::conditional_t<WITH_H, JetH<ND>, Jet1<ND>>;
        J jx[NX], ju[NU], jt[NTD], jn[NX];
#pragma unroll
        for (int i = 0; i < NU; ++i) ju[i] = J(u[i]);
#pragma unroll
        for (int i = 0; i < NX; ++i) jx[i] = J(x[i]);
        // linearize():  const int c = M::lin_coord(d);  if (c < NU) ju[c].g[d] = 1.0; else jx[c - NU].g[d] = 1.0;   (.d[d] without WITH_H)
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int c = M::lin_coord(d);
            if constexpr (WITH_H) {
                if (c < NU) ju[c < NU ? c : 0].g[d] = 1.0; else jx[c >= NU ? c - NU : 0].g[d] = 1.0;
            } else {
                if (c < NU) ju[c < NU ? c : 0].d[d] = 1.0; else jx[c >= NU ? c - NU : 0].d[d] = 1.0;
            }
        }
        // linearize():  for (int i = 0; i < NTD; ++i) jt[i] = J(thd[i]);
#pragma unroll
        for (int i = 0; i < NTD; ++i) jt[i] = J(thd[i]);
        // linearize():  disc_map<M, J>(jx, ju, jt, jn, sp.h, sp.rk_steps);
        disc_map<M, J>(jx, ju, jt, jn, h, rk_steps);
        // linearize():  M::lin_trivial(sp.h * sp.rk_steps, [&](int i, int j, double v) { Aset(i * NX + j, term ? 0.0 : v); });
        M::lin_trivial(h * rk_steps, [&](int i, int j, double v) { BA[i * NW + NU + j] = v; });
        // linearize():  r[i] = jn[i].v - xnext[i];  der = WITH_H ? jn[i].g[d] : jn[i].d[d];  c < NU ? Bset(i * NU + c, der) : Aset(i * NX + c - NU, der)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            out[i] = jn[i].v;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                double der;
                if constexpr (WITH_H) der = jn[i].g[d]; else der = jn[i].d[d];
                BA[i * NW + M::lin_coord(d)] = der;
            }
        }
        if constexpr (WITH_H) {
            double *H = BA + NX * NW, *hdd = H + NX * NH;
            double nu_next[NX];
#pragma unroll
            for (int m = 0; m < NX; ++m) nu_next[m] = aux[p * NX + m];
#pragma unroll
            for (int m = 0; m < NX; ++m)
#pragma unroll
                for (int e = 0; e < NH; ++e) H[m * NH + e] = jn[m].h[e];
            // linearize<true>():  acc = 0.0;  for (int m = 0; m < NX; ++m) acc = fma(nu_next[m], jn[m].h[e], acc);  hdd[e] = acc;
#pragma unroll
            for (int e = 0; e < NH; ++e) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < NX; ++m) acc = fma(nu_next[m], jn[m].h[e], acc);
                hdd[e] = acc;
            }
        }
    } else if constexpr (WHICH == 2) {
        // small_kernel.hpp sensitivities(), first-order branch:  ju[i] = Jet1<NTD>(u[i]);  jx[i] = Jet1<NTD>(x[i]);
        //   jt[i] = Jet1<NTD>(thd[i]), jt[i].d[i] = 1.0;  disc_map<M, Jet1<NTD>>(jx, ju, jt, jn, sp.h, sp.rk_steps);
        Jet1<NTD> jx[NX], ju[NU], jt[NTD], jn[NX];
#pragma unroll
        for (int i = 0; i < NU; ++i) ju[i] = Jet1<NTD>(u[i]);
#pragma unroll
        for (int i = 0; i < NX; ++i) jx[i] = Jet1<NTD>(x[i]);
#pragma unroll
        for (int i = 0; i < NTD; ++i) jt[i] = Jet1<NTD>(thd[i]), jt[i].d[i] = 1.0;
        disc_map<M, Jet1<NTD>>(jx, ju, jt, jn, h, rk_steps);
        // sensitivities():  Fth[m * NTD + d] = jn[m].d[d];
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            out[m] = jn[m].v;
#pragma unroll
            for (int d = 0; d < NTD; ++d) out[NX + m * NTD + d] = jn[m].d[d];
        }
    } else {
        // small_kernel.hpp sensitivities(), second-order pass:  ju[i] = Jet2<NTD>(u[i]), ju[i].e = yv[i];
        //   jx[i] = Jet2<NTD>(x[i]), jx[i].e = yv[NU + i];  jt[i] = Jet2<NTD>(thd[i]), jt[i].g[i] = 1.0;
        //   disc_map<M, Jet2<NTD>>(jx, ju, jt, jn, sp.h, sp.rk_steps);
        double yv[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) yv[i] = aux[p * NW + i];
        Jet2<NTD> jx[NX], ju[NU], jt[NTD], jn[NX];
#pragma unroll
        for (int i = 0; i < NU; ++i) ju[i] = Jet2<NTD>(u[i]), ju[i].e = yv[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) jx[i] = Jet2<NTD>(x[i]), jx[i].e = yv[NU + i];
#pragma unroll
        for (int i = 0; i < NTD; ++i) jt[i] = Jet2<NTD>(thd[i]), jt[i].g[i] = 1.0;
        disc_map<M, Jet2<NTD>>(jx, ju, jt, jn, h, rk_steps);
        // sensitivities():  Fth[m * NTD + d] = jn[m].g[d];  ... fma(nun[m], jn[m].m[d], ...)
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            out[m] = jn[m].v;
            out[NX + m] = jn[m].e;
#pragma unroll
            for (int d = 0; d < NTD; ++d) out[2 * NX + m * NTD + d] = jn[m].g[d], out[2 * NX + NX * NTD + m * NTD + d] = jn[m].m[d];
        }
    }
}

// WHICH 4: out[i] = jet_rcp(x[i]), the reciprocal every division of the jets goes through
__global__ void __launch_bounds__(64) jet_rcp_probe_kernel(int n, const double *x, double *out) {
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p < n) out[p] = jet_rcp(x[p]);
}

}  // namespace mpcrl
