// The deterministic policy gradient with a compatible linear critic (mpc4rl_amd/policy_gradient.py), from what the roll-out solves
// already give: pi(s_t) = u0*, its Jacobian J_t = du0*/dp on the K <= GN_KMAX learned entries, and V(s_t) as the baseline.  With
//     delta_j = (cost_j + gamma V_{j+E}) - V_j,   d_j = a_j - u0*_j (the exploration that was applied),   psi_j = J_j' d_j  [K]
// over the valid terms j, the critic's weights are the least-squares fit  w = (G/n + damping diag(G/n))^-1 (b/n),  G = sum psi psi',
// b = sum delta psi, and the policy gradient is  (M/n) w,  M = sum_j sum_c J_jc J_jc'  (J_jc: row c of J_j, one per control); the natural
// gradient is w itself.
//   cdpg_record_kernel   after a roll-out solve, before the plant's collect launch: row[e] of the tables V, u0*, status and J
//   cdpg_terms_kernel    delta, validity and the message [G | b | M | sum delta | count], summed in a fixed order
//   cdpg_apply_kernel    after the collective: the damped fp64 Cholesky solve for w, the step -lr (M/n) w or -lr w, clipped entrywise
// The reduction is that of qlearning_td_gn_kernel (qlearning_gn_kernel.hpp): X'X of staged rows on v_mfma_f64_16x16x4, upper tiles
// only, the tiles dealt to the two wavefronts, then the fixed-order batch sum of batch_sum.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qlearning_gn_kernel.hpp"

namespace mpcrl {

constexpr int CDPG_NU_MAX = 3;      // the controls of the largest plant (the chain of masses)

__host__ __device__ constexpr int cdpg_msg_len(int K) { return K * (K + 1) + K + 2; }

struct CdpgRecordArgs {
    const double *V;              // [E] the roll-out solve: value
    const double *u0;             // [E][nu]
    const double *du0;            // [E][nu][n_p]
    const int *status;            // [E]
    const int *row;               // [E] the table row the collect launch is about to write
    const int *idx;               // [K] columns of du0 (an entry outside [0, n_p) reads as a zero column)
    int E, T, nu, n_p, K;
    double *Vt;                   // [T][E]
    double *U0;                   // [T][E][nu]
    int *St;                      // [T][E]
    double *Jt;                   // [T][E][nu][K]
};

// One lane per environment and entry (c, a) of its J.  A row outside the table writes nothing.  Exact copies.
__global__ void __launch_bounds__(256) cdpg_record_kernel(const CdpgRecordArgs a) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int W = a.nu * a.K;
    if (g >= (long)a.E * W) return;
    const int e = (int)(g / W), q = (int)(g - (long)e * W);
    const int r = a.row[e];
    if (r < 0 || r >= a.T) return;
    const long k = (long)r * a.E + e;
    const int c = q / a.K;
    const int col = a.idx[q - c * a.K];
    a.Jt[k * W + q] = (col >= 0 && col < a.n_p) ? a.du0[((long)e * a.nu + c) * a.n_p + col] : 0.0;
    if (q == 0) a.Vt[k] = a.V[e], a.St[k] = a.status[e];
    if (q < a.nu) a.U0[k * a.nu + q] = a.u0[(long)e * a.nu + q];
}

struct CdpgTermsArgs {
    const double *Vt;             // [T][E]
    const double *U0;             // [T][E][nu]
    const double *Jt;             // [T][E][nu][K]
    const int *St;                // [T][E]
    const double *act;            // [T][E][nu] the applied controls (the episode table A)
    const double *cost;           // [T][E]
    const uint8_t *live;          // [T][E]
    int T, E, nu, K;
    double gamma;
    double *delta;                // [T-2][E]: delta where valid, else 0
    uint8_t *valid;               // [T-2][E] or nullptr
    double *partial;              // [n_blocks][cdpg_msg_len(K)]
    unsigned int *ticket;         // [1], zero before the first launch (the kernel leaves it zero)
    double *msg;                  // [cdpg_msg_len(K)]
};

// Terms j = i E + e, i < T - 2:  valid_j = live[i][e] && live[i+1][e] && live[i+2][e] (the liveness rule of qlearning_td_grad_kernel)
// && the roll-out solves of rows i and i + 1 returned status 0.  A block of TD_ROWS terms is staged GN_HALF rows at a time, 1 + nu times:
//     pass 0      rows ok_j [psi_j | delta_j]:  [G | b] = X'X into the first set of accumulators (b rides as column K);
//     pass 1 + c  rows ok_j J_jc:               M += X'X into the second set (its column K is zero)
// psi_ja = sum_c nan_to_num(J_jca) d_jc in fp64 with contraction off, c in order, formed while staging; ok_j in {0, 1} is selected, so a
// NaN of an invalid term never enters a product.  Tiles, operand layout and the row stride gn_ld are those of qlearning_td_gn_kernel;
// every entry is summed over the block's terms in one fixed order by one accumulator.  Then the fixed-order batch sum over the blocks.
template <int NC>
__global__ void __launch_bounds__(128) cdpg_terms_kernel(const CdpgTermsArgs a) {
    constexpr int LD = gn_ld(NC), NRMAX = NC < 4 ? NC : 4;
    constexpr int NTILE = NRMAX * NC - NRMAX * (NRMAX - 1) / 2, NQ = (NTILE + 1) / 2;
    __shared__ double X[GN_HALF * LD];
    __shared__ double dlr[TD_ROWS], okr[TD_ROWS], dr[CDPG_NU_MAX][TD_ROWS];
    const int K = a.K, nu = a.nu, KK = K * (K + 1) / 2, P = 2 * KK + K + 2, W = nu * K;
    const long M = (long)(a.T - 2) * a.E;
    const long b0 = (long)blockIdx.x * TD_ROWS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const long j = b0 + tid;
        double tj = 0.0, oj = 0.0, dj[CDPG_NU_MAX] = {0.0, 0.0, 0.0};
        if (j < M) {
#pragma clang fp contract(off)      // cost + gamma V' - V in the Q-learning kernels' order: product, sum, difference
            const long E = a.E;
            const bool ok = a.live[j] && a.live[j + E] && a.live[j + 2 * E] && a.St[j] == 0 && a.St[j + E] == 0;
            double t = a.gamma * a.Vt[j + E];
            t = a.cost[j] + t;
            t = t - a.Vt[j];
            tj = ok ? t : 0.0;
            a.delta[j] = tj;
            if (a.valid) a.valid[j] = ok ? 1 : 0;
            oj = ok ? 1.0 : 0.0;
#pragma unroll
            for (int c = 0; c < CDPG_NU_MAX; ++c)
                if (c < nu) {
                    const double d = a.act[j * nu + c] - a.U0[j * nu + c];
                    dj[c] = ok ? d : 0.0;
                }
        }
        dlr[tid] = tj, okr[tid] = oj;
#pragma unroll
        for (int c = 0; c < CDPG_NU_MAX; ++c) dr[c][tid] = dj[c];
    }
    // this wavefront's tiles (wavefront-uniform)
    const int NR = (K + 15) / 16;
    int ta[NQ], tb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        int ti = 0, rem = 2 * q + wave;
        while (ti < NR && rem >= NC - ti) rem -= NC - ti, ++ti;
        ta[q] = ti < NR ? 16 * ti : -1, tb[q] = 16 * (ti + rem);
    }
    gn_d4 accG[NQ], accM[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) accG[q] = gn_d4{0.0, 0.0, 0.0, 0.0}, accM[q] = gn_d4{0.0, 0.0, 0.0, 0.0};
    // A(i, k) and B(k, j) of v_mfma_f64_16x16x4 sit at lane 16 k + (i | j): both operands are row 4 ks + lane / 16 of X
    const double *xr = X + (lane >> 4) * LD + (lane & 15);
    auto tiles = [&](gn_d4(&acc)[NQ]) {
#pragma unroll 4
        for (int ks = 0; ks < GN_HALF / 4; ++ks) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (ta[q] >= 0) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[ks * 4 * LD + ta[q]], xr[ks * 4 * LD + tb[q]], acc[q], 0, 0, 0);
        }
    };
    const int nr = (int)(M - b0 < TD_ROWS ? M - b0 : TD_ROWS);
    for (int h0 = 0; h0 < nr; h0 += GN_HALF) {
        __syncthreads();                // the rows of the first phase are written / the products of the last pass are done
        for (int e = tid; e < GN_HALF * LD; e += 128) {
            const int r = e / LD, c = e - r * LD, rr = h0 + r;
            double v = 0.0;
            if (rr < nr && okr[rr] != 0.0) {
                if (c < K) {
#pragma clang fp contract(off)
                    const double *J = a.Jt + (b0 + rr) * W + c;
                    v = nan_to_num_d(J[0]) * dr[0][rr];
                    for (int cc = 1; cc < nu; ++cc) v = v + nan_to_num_d(J[cc * K]) * dr[cc][rr];
                } else if (c == K) {
                    v = dlr[rr];
                }
            }
            X[e] = v;
        }
        __syncthreads();
        tiles(accG);
        for (int p = 0; p < nu; ++p) {
            __syncthreads();            // the products of the last pass are done
            for (int e = tid; e < GN_HALF * LD; e += 128) {
                const int r = e / LD, c = e - r * LD, rr = h0 + r;
                double v = 0.0;
                if (rr < nr && c < K && okr[rr] != 0.0) v = nan_to_num_d(a.Jt[(b0 + rr) * W + p * K + c]);
                X[e] = v;
            }
            __syncthreads();
            tiles(accM);
        }
    }
    // register r of a tile holds its rows 4 r + lane / 16, column lane % 16
    double *row = a.partial + (long)blockIdx.x * P;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (ta[q] < 0) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ta[q] + 4 * r + (lane >> 4), c = tb[q] + (lane & 15);
            if (i < K && c >= i && c <= K) {
                const int at = i * K - i * (i - 1) / 2 + (c - i);
                row[c < K ? at : KK + i] = accG[q][r];
                if (c < K) row[KK + K + at] = accM[q][r];
            }
        }
    }
    if (tid == 0) {
        double s = 0.0, n = 0.0;
        for (int r = 0; r < TD_ROWS; ++r) s += dlr[r], n += okr[r];
        row[2 * KK + K] = s, row[2 * KK + K + 1] = n;
    }
    if (!last_workgroup(a.ticket)) return;
    sliced_final_sum<TD_PMAX, TD_ROWS>(a.partial, gridDim.x, P, [&](int p, double s) { a.msg[p] = s; });
}

// After the collective, one workgroup.  n, Gb, bb, d_max, H, the Cholesky solve and the codes -1 and a + 1 are those of
// qlearning_gn_apply_kernel;  w = H^-1 bb;  s = w (natural != 0) or s_a = sum_c (M_ac / n) w_c, c in order, contraction off;
// Delta_a = (-lr) s_a, clipped to [l_a, u_a]:
//     l_a = max(lo_c - theta_c, -radius scale_c),  u_a = min(hi_c - theta_c, +radius scale_c),  c = idx[a]
// (lo, hi, scale may each be null: -inf, +inf, 1; all null and radius = inf: no clip).  l_a <= u_a fails for some a (a NaN included):
// info = -2, checked before the factorisation.  On every code but 0 theta is untouched and step_out, w_out, active are 0.  Else
// theta_c = min(max(theta_c + Delta_a, lo_c), hi_c) with contraction off, step_out[c] = Delta_a (a clipped entry: l_a or u_a bit for bit),
// w_out = w, active[a] = 0 inside / 1 clipped to l_a / 2 clipped to u_a, info = 0.  Fixed order, no atomics.
__global__ void __launch_bounds__(GN_APPLY_NT) cdpg_apply_kernel(const double *msg, int K, const int *idx, int n_theta, double lr, double damping, int natural,
                                                                 const double *lo, const double *hi, const double *scale, double radius, double *theta,
                                                                 double *step_out, double *w_out, uint8_t *active, int *info) {
    __shared__ double H[GN_KMAX * GN_KMAX];     // the lower triangle: H[i][j], j <= i
    __shared__ double y[GN_KMAX], lb[GN_KMAX], ub[GN_KMAX];
    __shared__ double dmax_s;
    __shared__ int bad_s;
    const int tid = threadIdx.x, KK = K * (K + 1) / 2;
    const double count = msg[2 * KK + K + 1];
    const double n = count > 1.0 ? count : 1.0;
    for (int i = tid; i < n_theta; i += GN_APPLY_NT) step_out[i] = 0.0;
    if (tid < K) w_out[tid] = 0.0, active[tid] = 0;
    for (int e = tid; e < K * K; e += GN_APPLY_NT) {
        const int i = e / K, j = e - i * K;
        if (j <= i) H[i * GN_KMAX + j] = msg[j * K - j * (j - 1) / 2 + (i - j)] / n;
    }
    if (tid < K) y[tid] = msg[KK + tid] / n;
    __syncthreads();
    if (tid == 0) {
        double d = H[0];
        for (int i = 1; i < K; ++i) {
            const double v = H[i * GN_KMAX + i];
            d = (v != v || v > d) ? v : d;      // (a NaN stays)
        }
        dmax_s = d;
    }
    __syncthreads();
    const double d_max = dmax_s;
    if (!(count > 0.0) || !isfinite(d_max) || d_max == 0.0) {
        if (tid == 0) *info = -1;
        return;
    }
    const bool clip = lo || hi || scale || radius < INFINITY;
    if (tid < 64) {                             // the first wavefront holds one entry per lane
        bool bad = false;
        if (tid < K) {
#pragma clang fp contract(off)
            const double g = H[tid * GN_KMAX + tid];
            H[tid * GN_KMAX + tid] = g + damping * (g > 0.0 ? g : 1e-12 * d_max);
            const int c = idx[tid];
            double l = 0.0, u = 0.0;            // an entry outside theta cannot move
            if (c >= 0 && c < n_theta) {
                l = -INFINITY, u = INFINITY;
                if (clip) {
                    const double t = radius * (scale ? scale[c] : 1.0);
                    const double p = lo ? lo[c] - theta[c] : -INFINITY, q = hi ? hi[c] - theta[c] : INFINITY;
                    l = (p > -t || p != p) ? p : -t;
                    u = (q < t || q != q) ? q : t;
                }
            }
            bad = !(l <= u);
            lb[tid] = l, ub[tid] = u;
        }
        const unsigned long long any_bad = __ballot(bad);
        if (tid == 0) bad_s = any_bad != 0ull;
    }
    __syncthreads();
    if (bad_s) {
        if (tid == 0) *info = -2;
        return;
    }
    const int fail = gn_chol_solve(H, y, K, tid);
    if (fail >= 0) {
        if (tid == 0) *info = fail + 1;
        return;
    }
    if (tid < K) {
#pragma clang fp contract(off)      // theta + step with the step rounded first, then the clamp
        double s = y[tid];
        if (!natural) {
            const double *Mm = msg + KK + K;
            s = 0.0;
            for (int c = 0; c < K; ++c) {
                const int i = c < tid ? c : tid, j = c < tid ? tid : c;
                const double m = Mm[i * K - i * (i - 1) / 2 + (j - i)] / n;
                s = s + m * y[c];
            }
        }
        double d = (-lr) * s;
        int st = 0;
        if (d < lb[tid]) d = lb[tid], st = 1;
        else if (d > ub[tid]) d = ub[tid], st = 2;
        const int c = idx[tid];
        if (c >= 0 && c < n_theta) {
            double t = theta[c] + d;
            if (lo) t = t < lo[c] ? lo[c] : t;
            if (hi) t = t > hi[c] ? hi[c] : t;
            theta[c] = t, step_out[c] = d;      // (after the barriers above: the zeros are written)
        }
        w_out[tid] = y[tid], active[tid] = (uint8_t)st;
    }
    if (tid == 0) *info = 0;
}

}  // namespace mpcrl
