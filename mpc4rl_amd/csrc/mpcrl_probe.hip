// mpcrl_probe.hip — include/mpcrl_probe_ext.h, include/mpcrl_probe_chain_ext.h: test probes of single phases of the solve kernels.  One wavefront, one launch; the shipped
// form of a phase against a reference copy of an earlier form that lives in this unit only (tests/test_gpu_mx_factor_step.py,
// tests/test_gpu_mx_chain_step.py).
#include "mpcrl_host.hpp"

#include <cstring>

#include "../../include/mpcrl_probe_ext.h"
#include "../../include/mpcrl_probe_chain_ext.h"
#include "small_kernel.hpp"

using namespace mpcrl;

namespace {

// The factor sweep as it was before the column-3 copy of p_k, the lane-mask pivot flag and the peeled stage-0 step: a verbatim copy
// (the model's name for M, the mask LANES_C01 the header no longer has), what "the same factors, bit for bit" is measured against.  It
// expects the publish layout of that time: 0.0 at mxRow + 6.
struct MxFactorBefore : SmallSolver<CartpoleDev> {
    using M = CartpoleDev;
    static constexpr unsigned long long LANES_C01 = 0x3333333333333333ull;   // lane & 3 < 2
    MPCRL_DI MxFactorBefore(const SmallSpec &sp_, int k_, int lpi_, int base_) : SmallSolver<CartpoleDev>(sp_, k_, lpi_, base_) {}
    template <bool WANT_P>
    MPCRL_DI void mx_factor() {
        const int l = threadIdx.x & 63, r = l >> 4, blk = (l >> 2) & 3, c = l & 3;
        const int ipw = min(64 / lpi, M::MAX_IPW);
        const bool live = blk < ipw;
        double *S0 = ms + (live ? blk : 0) * lpi * MSLOT;   // an idle block shadows block 0 and stores to the dump
        const int oAH = mxAH + 2 * (4 * r + c), oCol = mxCol + 4 * r + (c >= 1 ? 2 : 0), oB = mxCol + 4 * r, oRow = mxRow + 2 * c;
        // store targets: slot-relative for lanes with something to store, else the dump pair (stride 0)
        double *const dump = ms + mxDump;   // (every lane its own dump word instead of one for all: measured, no difference)
        const bool has1 = live && c < 3, has2 = live && r == 0 && c < 3, has3 = live && c == 1;
        double *const wP = live ? S0 + oAH + 1 : dump;
        double *const w1 = has1 ? S0 + (c == 0 ? mxK + r : (c == 1 ? mxCol + 4 * r + 3 : mxRow + 2 * r)) : dump;   // K[r] | d[r] | q[r]
        double *const w2 = has2 ? S0 + mxMisc + c : dump + 1;                                                      // 1/R | kff | beta
        double *const w3 = has3 ? S0 + mxCol + 4 * r + 1 : dump;                                                   // p[r]
        const int sL = live ? MSLOT : 0, s1 = has1 ? MSLOT : 0, s2 = has2 ? MSLOT : 0, s3 = has3 ? MSLOT : 0;
        double Pm, pcol;
        {
            const double *sl = S0 + N * MSLOT;
            Pm = sl[oAH + 1];
            pcol = c == 1 ? sl[oCol + 1] : 0.0;   // g_x of the terminal stage (column 1)
        }
        double okacc = 1.0;             // > 0 while every pivot was positive
        auto load = [&](MxOps &o, int kk) {
            const double *sl = S0 + (kk > 0 ? kk : 0) * MSLOT;
            o.ah = lds_pair(sl + oAH), o.cp = lds_pair(sl + oCol), o.rp = lds_pair(sl + oRow), o.Br = sl[oB];
        };
        double sV1 = 0.0, sV2 = 0.0, sV3 = 0.0;   // results of a step
        // the arithmetic of one step.  PIN: the step of stage 0 in Q-mode (u_0 pinned: K_0 = 0, kff_0 = 0, P_0 = Q)
        auto head = [&](const MxOps &o, double &Y, double &X1) {
            Y = mfma4(Pm, o.cp.x, pcol);          // column 3 of W is never read: bb there as well (no select)
            X1 = mfma4(Pm, o.ah.x, 0.0);
        };
        auto tail = [&](const MxOps &o, double Y, double X1, bool pin) {
            const double Am = o.ah.x, CZc = lane_select(LANES_C01, o.cp.y, 0.0);
            const double Yb = quad_bcast<0>(Y);
            const double Zc = mfma4(Am, Y, CZc);
            const double Zb = mfma4(o.Br, Y, o.rp.x);
            const double Qt = mfma4(Am, X1, o.ah.y);
            const double Zr = mfma4(Yb, Am, o.rp.y);            // every row = S'
            const double R = quad_bcast<0>(Zb), mvu = quad_bcast<1>(Zb), Sr = quad_bcast<0>(Zc);
            okacc = (R > 0.0 || pin) ? okacc : 0.0;
            const double Rinv = pin ? 0.0 : fast_rcp(R);
            const double Kr = Sr * Rinv;
            Pm = fma(-Kr, Zr, Qt);                              // P_k = Q - K S'
            const double t = fma(-Kr, Zb, Zc);                  // own column: p_k (c = 1), q_k (c = 2)
            pcol = lane_select(LANES_C1, t, 0.0);
            const double kf = mvu * Rinv;
            const double dk = fma(-o.Br, kf, o.cp.x);           // c = 1: bb[r] - B[r] kff
            sV1 = lane_select(LANES_C0, Kr, lane_select(LANES_C1, dk, t));       // K[r] | d[r] | q[r]
            sV2 = lane_select(LANES_C0, Rinv, lane_select(LANES_C1, kf, Zb));    // 1/R | kff | beta
            sV3 = t;
        };
        auto store = [&](int kk) {
            wP[kk * sL] = Pm;
            w1[kk * s1] = sV1;
            w2[kk * s2] = sV2;
            if constexpr (WANT_P) w3[kk * s3] = sV3;
        };
        // the operands of a stage do not depend on the recursion: those of stage kk - 1 are fetched while stage kk is computed
        MxOps on;
        load(on, N - 1);
        for (int kk = N - 1; kk >= 0; --kk) {
            const MxOps o = on;
            load(on, kk - 1);
            double Y, X1;
            head(o, Y, X1);
            tail(o, Y, X1, kk == 0 && qmode);
            store(kk);
        }
        if (live && r == 0 && c == 0) ms[mxFlag + blk] = okacc;
    }
};
static_assert(MxFactorBefore::MSLOT == MPCRL_PROBE_MX_SLOT && MxFactorBefore::MX_SLOTS == 64, "mpcrl_probe_ext.h describes another slot");

// sp carries the horizon only.  Every lane copies its slot in (the entry of column 3 of the published row vector as the chosen form
// publishes it), the wavefront runs the sweep, every lane copies its slot out; lanes 0 .. 3 the four flags.
template <bool WANT_P>
__global__ void __launch_bounds__(64) mx_factor_probe_kernel(SmallSpec sp, const double *in, int pin, int which, double *out, double *ok) {
    using S_t = MxFactorBefore;
    __shared__ __attribute__((aligned(16))) double lds[S_t::MX_LDS];
    const int lane = threadIdx.x, lpi = sp.N + 1, slot = lane / lpi, k = lane - slot * lpi;
    S_t S(sp, k, lpi, slot * lpi);
    S.ms = lds;
    S.qmode = pin != 0;
    double *sl = lds + lane * S_t::MSLOT;
    for (int i = 0; i < S_t::MSLOT; ++i) sl[i] = in[lane * S_t::MSLOT + i];
    sl[S_t::mxRow + 6] = which == 0 ? 0.0 : sl[S_t::mxRow + 2];
    if (lane < 4) lds[S_t::mxFlag + lane] = -1.0;
    if (lane < 2) lds[S_t::mxDump + lane] = 0.0;
    S_t::wave_lds_sync();
    if (which == 0)   // (wave-uniform)
        S.template mx_factor<WANT_P>();
    else
        S.SmallSolver<CartpoleDev>::template mx_factor<WANT_P>();
    S_t::wave_lds_sync();
    for (int i = 0; i < S_t::MSLOT; ++i) out[lane * S_t::MSLOT + i] = sl[i];
    if (lane < 4) ok[lane] = lds[S_t::mxFlag + lane];
}

// The affine chain as it was before its last turns were peeled and the addresses of its loop written out: a verbatim copy (every
// fetch clamps its stage with slot_of; MPCRL_CHAIN_DEPTH at its value of that time), with the slot layout it reads — the one of
// small_kernel.hpp at that time, which the chains have kept (profiles/chain_step.txt).
struct MxChainBefore : SmallSolver<CartpoleDev> {
    using M = CartpoleDev;
    MPCRL_DI MxChainBefore(const SmallSpec &sp_, int k_, int lpi_, int base_) : SmallSolver<CartpoleDev>(sp_, k_, lpi_, base_) {}
    template <bool FWD>
    MPCRL_DI void mx_chain() {
        const int l = threadIdx.x & 63, r = l >> 4, blk = (l >> 2) & 3, c = l & 3;
        const int ipw = min(64 / lpi, M::MAX_IPW);
        const bool live = blk < ipw;
        const double *S0 = ms + (live ? blk : 0) * lpi * MSLOT;
        const int oA = mxAH + (FWD ? 2 * (4 * c + r) : 2 * (4 * r + c)), oBx = mxCol + 4 * (FWD ? c : r), oKx = mxK + (FWD ? r : c),
                  oC = mxCol + 4 * r + 3;
        const bool wr = live && c == 0;
        double *const wO = wr ? ms + (S0 - ms) + (FWD ? mxRow + 2 * r + 1 : mxCol + 4 * r + 1) : ms + mxDump;
        const int sO = wr ? MSLOT : 0;
        double V = 0.0;
        if constexpr (!FWD) {
            V = S0[N * MSLOT + oC];
            wO[N * sO] = V;   // p_N
        }
        constexpr int DEPTH = 3;
        auto slot_of = [&](int s_) { const int sc = s_ < N ? s_ : N - 1; return FWD ? sc : N - 1 - sc; };   // stage of chain step s_ (clamped)
        double Ar[DEPTH], Br_[DEPTH], Kr_[DEPTH], Cr[DEPTH];
        auto fetch = [&](int j, int s_) {
            const double *sl = S0 + slot_of(s_) * MSLOT;
            Ar[j] = sl[oA], Br_[j] = sl[oBx], Kr_[j] = sl[oKx], Cr[j] = sl[oC];
        };
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) fetch(j, j);
        int s_ = 0;
        for (; s_ + DEPTH <= N; s_ += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                V = mfma4(fma(-Br_[j], Kr_[j], Ar[j]), V, Cr[j]);
                wO[(FWD ? slot_of(s_ + j) + 1 : slot_of(s_ + j)) * sO] = V;
                fetch(j, s_ + j + DEPTH);
            }
        }
#pragma unroll
        for (int j = 0; j < DEPTH - 1; ++j)
            if (s_ + j < N) {
                V = mfma4(fma(-Br_[j], Kr_[j], Ar[j]), V, Cr[j]);
                wO[(FWD ? slot_of(s_ + j) + 1 : slot_of(s_ + j)) * sO] = V;
            }
    }
};

// Every lane copies its slot in, the wavefront runs one chain, every lane copies its slot out.
template <bool FWD>
__global__ void __launch_bounds__(64) mx_chain_probe_kernel(SmallSpec sp, const double *in, int which, double *out) {
    using S_t = MxChainBefore;
    __shared__ __attribute__((aligned(16))) double lds[S_t::MX_LDS];
    const int lane = threadIdx.x, lpi = sp.N + 1, slot = lane / lpi, k = lane - slot * lpi;
    S_t S(sp, k, lpi, slot * lpi);
    S.ms = lds;
    double *sl = lds + lane * S_t::MSLOT;
    for (int i = 0; i < S_t::MSLOT; ++i) sl[i] = in[lane * S_t::MSLOT + i];
    if (lane < 4) lds[S_t::mxFlag + lane] = -1.0;
    if (lane < 2) lds[S_t::mxDump + lane] = 0.0;
    S_t::wave_lds_sync();
    if (which == 0)   // (wave-uniform)
        S.template mx_chain<FWD>();
    else
        S.SmallSolver<CartpoleDev>::template mx_chain<FWD>();
    S_t::wave_lds_sync();
    for (int i = 0; i < S_t::MSLOT; ++i) out[lane * S_t::MSLOT + i] = sl[i];
}

}  // namespace

extern "C" {

int mpcrl_probe_ext_version(void) { return MPCRL_PROBE_EXT_VERSION; }

int mpcrl_debug_mx_factor(const double *slots_in, int N, int flags, int which, double *slots_out, double *ok_out, void *stream) {
    if (!slots_in || !slots_out || !ok_out || N < 1 || N > 63 || which < 0 || which > 1) return MPCRL_E_ARG;
    if (flags & ~(MPCRL_PROBE_MX_PIN | MPCRL_PROBE_MX_WANT_P)) return MPCRL_E_ARG;
    ON_DEVICE_OF(slots_out);
    const hipStream_t st = (hipStream_t)stream;
    SmallSpec sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.N = N;
    const int pin = (flags & MPCRL_PROBE_MX_PIN) ? 1 : 0;
    if (flags & MPCRL_PROBE_MX_WANT_P)
        hipLaunchKernelGGL(mx_factor_probe_kernel<true>, dim3(1), dim3(64), 0, st, sp, slots_in, pin, which, slots_out, ok_out);
    else
        hipLaunchKernelGGL(mx_factor_probe_kernel<false>, dim3(1), dim3(64), 0, st, sp, slots_in, pin, which, slots_out, ok_out);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_probe_chain_ext_version(void) { return MPCRL_PROBE_CHAIN_EXT_VERSION; }

int mpcrl_debug_mx_chain(const double *slots_in, int N, int forward, int which, double *slots_out, void *stream) {
    if (!slots_in || !slots_out || N < 1 || N > 63 || which < 0 || which > 1 || forward < 0 || forward > 1) return MPCRL_E_ARG;
    ON_DEVICE_OF(slots_out);
    const hipStream_t st = (hipStream_t)stream;
    SmallSpec sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.N = N;
    if (forward)
        hipLaunchKernelGGL(mx_chain_probe_kernel<true>, dim3(1), dim3(64), 0, st, sp, slots_in, which, slots_out);
    else
        hipLaunchKernelGGL(mx_chain_probe_kernel<false>, dim3(1), dim3(64), 0, st, sp, slots_in, which, slots_out);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"
