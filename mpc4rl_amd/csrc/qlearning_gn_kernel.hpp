// The Gauss-Newton (least-squares TD) parameter step of the device Q-learners (mpc4rl_amd/qlearning.py, method="gauss_newton"):
//     Delta = lr (G/n + damping diag(G/n))^-1 (b/n),   G = sum_j ok_j g_j g_j',  b = sum_j ok_j td_j g_j,  g_j = dQ/dp_j[idx]
// over the K <= GN_KMAX learned entries idx of theta — a step that is covariant under a rescaling of the parameters, where the first-order
// step of qlearning_kernel.hpp needs one lr per model.
//   qlearning_td_gn_kernel     the TD errors of the learning sweep, exactly as qlearning_td_grad_kernel computes them, and the message
//                              [G (upper triangle, packed row-major) | b | sum td | count], summed in a fixed order
//   qlearning_gn_apply_kernel  after the collective: the damped fp64 Cholesky solve in LDS, theta[idx] += Delta
//   qlearning_gn_apply_box_kernel  the same step inside bounds on theta and a per-entry trust region: a box QP, solved exactly
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qlearning_kernel.hpp"

namespace mpcrl {

constexpr int GN_KMAX = 64;         // the cap on the learned entries: H [64][64] doubles is 32 KB of LDS, one workgroup factors it
constexpr int GN_HALF = 64;         // rows staged at a time: 64 x 80 doubles = 40 KB (a block of 128 would not fit the 64 KB of a workgroup)

typedef double gn_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int gn_msg_len(int K) { return K * (K + 1) / 2 + K + 2; }
// the row stride of the staged rows, in doubles: the 16 NC columns, made an odd multiple of 16 so that the four rows an operand load
// touches (64 lanes: rows 4 ks + lane / 16, 16 consecutive columns each) fall on different LDS banks
__host__ __device__ constexpr int gn_ld(int NC) { return (16 * NC) | 16; }

struct QlGnArgs {
    const double *Q, *V;          // [T-1][E]
    const double *dQ;             // [T-1][E][n_p]
    const int *sq, *sv;           // [T-1][E]
    const double *cost;           // [T][E]
    const uint8_t *live;          // [T][E]
    const int *idx;               // [K] columns of dQ, strictly increasing (an entry outside [0, n_p) reads as a zero column)
    int T, E, n_p, K;
    double gamma;
    double *td;                   // [T-2][E]: td where valid, else 0
    uint8_t *valid;               // [T-2][E] or nullptr
    double *partial;              // [n_blocks][gn_msg_len(K)]
    unsigned int *ticket;         // [1], zero before the first launch (the kernel leaves it zero)
    double *msg;                  // [gn_msg_len(K)]
};

// Terms, validity and td: those of qlearning_td_grad_kernel (the same expressions: the same bits).  A block of TD_ROWS terms gives
//     [G | b] = X' X  with the rows X_j = ok_j [g_j | td_j]   (ok_j in {0, 1}: selected, a NaN of an invalid term never enters a product)
// as 16 x 16 tiles of v_mfma_f64_16x16x4, the upper ones only; b rides as column K.  NC = ceil((K + 1) / 16) column tiles, NR =
// ceil(K / 16) row tiles; tile t (row tiles in order, the column tiles ti .. NC - 1 of each in order) belongs to wavefront t % 2, which
// keeps its 16 x 16 sums in registers over both half blocks: every entry is summed over the block's terms in term order by one
// accumulator.  Then the fixed-order batch sum of batch_sum.hpp over the blocks.
template <int NC>
__global__ void __launch_bounds__(128) qlearning_td_gn_kernel(const QlGnArgs a) {
    constexpr int LD = gn_ld(NC), NRMAX = NC < 4 ? NC : 4;
    constexpr int NTILE = NRMAX * NC - NRMAX * (NRMAX - 1) / 2, NQ = (NTILE + 1) / 2;
    __shared__ double X[GN_HALF * LD];
    __shared__ double tdr[TD_ROWS], okr[TD_ROWS];
    __shared__ int sidx[GN_KMAX];
    const int K = a.K, KK = K * (K + 1) / 2, P = KK + K + 2;
    const long M = (long)(a.T - 2) * a.E;
    const long b0 = (long)blockIdx.x * TD_ROWS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const long j = b0 + tid;
        double tj = 0.0, oj = 0.0;
        if (j < M) {
            const long E = a.E;
            const bool ok = a.live[j] && a.live[j + E] && a.live[j + 2 * E] && a.sq[j] == 0 && a.sv[j] == 0 && a.sq[j + E] == 0 && a.sv[j + E] == 0;
            double t;
            {
#pragma clang fp contract(off)      // cost + gamma V' - Q as the script writes it: product, sum, difference
                t = a.gamma * a.V[j + E];
                t = a.cost[j] + t;
                t = t - a.Q[j];
            }
            tj = ok ? t : 0.0;
            a.td[j] = tj;
            if (a.valid) a.valid[j] = ok ? 1 : 0;
            oj = ok ? 1.0 : 0.0;
        }
        tdr[tid] = tj, okr[tid] = oj;
        if (tid < GN_KMAX) {
            const int c = tid < K ? a.idx[tid] : -1;
            sidx[tid] = (c >= 0 && c < a.n_p) ? c : -1;
        }
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
    gn_d4 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = gn_d4{0.0, 0.0, 0.0, 0.0};
    const int nr = (int)(M - b0 < TD_ROWS ? M - b0 : TD_ROWS);
    for (int h0 = 0; h0 < nr; h0 += GN_HALF) {
        __syncthreads();                // the rows of the first phase are written / the products of the last half block are done
        for (int e = tid; e < GN_HALF * LD; e += 128) {
            const int r = e / LD, c = e - r * LD, rr = h0 + r;
            double v = 0.0;
            if (rr < nr && okr[rr] != 0.0) {
                if (c < K) {
                    const int col = sidx[c];
                    v = col >= 0 ? nan_to_num_d(a.dQ[(b0 + rr) * a.n_p + col]) : 0.0;
                } else if (c == K) {
                    v = tdr[rr];
                }
            }
            X[e] = v;
        }
        __syncthreads();
        // A(i, k) and B(k, j) of v_mfma_f64_16x16x4 sit at lane 16 k + (i | j): both operands are row 4 ks + lane / 16 of X
        const double *xr = X + (lane >> 4) * LD + (lane & 15);
#pragma unroll 4
        for (int ks = 0; ks < GN_HALF / 4; ++ks) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (ta[q] >= 0) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[ks * 4 * LD + ta[q]], xr[ks * 4 * LD + tb[q]], acc[q], 0, 0, 0);
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
            if (i < K && c >= i && c <= K) row[c < K ? i * K - i * (i - 1) / 2 + (c - i) : KK + i] = acc[q][r];
        }
    }
    if (tid == 0) {
        double s = 0.0, n = 0.0;
        for (int r = 0; r < TD_ROWS; ++r) s += tdr[r], n += okr[r];
        row[KK + K] = s, row[KK + K + 1] = n;
    }
    if (!last_workgroup(a.ticket)) return;
    sliced_final_sum<TD_PMAX, TD_ROWS>(a.partial, gridDim.x, P, [&](int p, double s) { a.msg[p] = s; });
}

// The factor-and-solve both apply kernels share, one workgroup of GN_APPLY_NT lanes: the fp64 Cholesky factorisation H = L L' of the
// leading K x K block (lower triangle, row stride GN_KMAX) in LDS, right-looking, column by column, then y <- H^-1 y.  H and y are written
// and a barrier has passed before the call; y is visible to every lane after it.  Returns -1, or the index of the first pivot that is not
// a finite number > 0 (the same value in every lane; H and y are then left half done).
constexpr int GN_APPLY_NT = 256;

__device__ inline int gn_chol_solve(double *H, double *y, int K, int tid) {
    for (int k = 0; k < K; ++k) {
        const double piv = H[k * GN_KMAX + k];      // every lane reads the same value: the branch is uniform
        if (!(isfinite(piv) && piv > 0.0)) return k;
        const double l = sqrt(piv);
        __syncthreads();                            // every lane has read the pivot
        if (tid == 0) H[k * GN_KMAX + k] = l;
        for (int i = k + 1 + tid; i < K; i += GN_APPLY_NT) H[i * GN_KMAX + k] = H[i * GN_KMAX + k] / l;
        __syncthreads();
        const int m = K - 1 - k;                    // the trailing block: rows k + 1 + i, columns k + 1 + j, j <= i < m
        for (int e = tid; e < m * m; e += GN_APPLY_NT) {
            const int i = e / m, j = e - i * m;
            if (j <= i) H[(k + 1 + i) * GN_KMAX + k + 1 + j] -= H[(k + 1 + i) * GN_KMAX + k] * H[(k + 1 + j) * GN_KMAX + k];
        }
        __syncthreads();
    }
    // L z = bb, then L' x = z, a column at a time
    for (int k = 0; k < K; ++k) {
        const double z = y[k] / H[k * GN_KMAX + k];
        __syncthreads();
        if (tid == 0) y[k] = z;
        if (tid > k && tid < K) y[tid] -= H[tid * GN_KMAX + k] * z;
        __syncthreads();
    }
    for (int k = K - 1; k >= 0; --k) {
        const double x = y[k] / H[k * GN_KMAX + k];
        __syncthreads();
        if (tid == 0) y[k] = x;
        if (tid < k) y[tid] -= H[k * GN_KMAX + tid] * x;
        __syncthreads();
    }
    return -1;
}

// After the collective, one workgroup.  n = max(1, count), Gb = G / n, bb = b / n, d_max = max_a Gb_aa (a NaN diagonal makes it NaN);
//   count == 0, or d_max not finite, or d_max == 0:  info = -1, theta untouched, step_out = 0;
//   H = Gb + damping diag(Gb_aa > 0 ? Gb_aa : 1e-12 d_max)  (Marquardt's scaling: the step stays covariant under a diagonal rescaling of
//   the parameters for any damping; an entry no term is sensitive to has a zero row, column and bb_a, so its floor only keeps H positive
//   definite and its Delta_a is 0 whatever the floor), fp64 Cholesky H = L L' in LDS, right-looking, column by column;
//   pivot a not a finite number > 0:  info = a + 1, theta untouched, step_out = 0;
//   else Delta = lr H^-1 bb, theta[idx[a]] += Delta_a, step_out = Delta scattered (0 elsewhere), info = 0.
__global__ void __launch_bounds__(GN_APPLY_NT) qlearning_gn_apply_kernel(const double *msg, int K, const int *idx, int n_theta, double lr, double damping,
                                                                         double *theta, double *step_out, int *info) {
    __shared__ double H[GN_KMAX * GN_KMAX];     // the lower triangle: H[i][j], j <= i
    __shared__ double y[GN_KMAX];
    __shared__ double dmax_s;
    const int tid = threadIdx.x, KK = K * (K + 1) / 2;
    const double count = msg[KK + K + 1];
    const double n = count > 1.0 ? count : 1.0;
    for (int i = tid; i < n_theta; i += GN_APPLY_NT) step_out[i] = 0.0;
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
    if (tid < K) {
        const double g = H[tid * GN_KMAX + tid];
        H[tid * GN_KMAX + tid] = g + damping * (g > 0.0 ? g : 1e-12 * d_max);
    }
    __syncthreads();
    const int fail = gn_chol_solve(H, y, K, tid);
    if (fail >= 0) {
        if (tid == 0) *info = fail + 1;
        return;
    }
    if (tid < K) {
#pragma clang fp contract(off)      // theta + step with the step rounded first: theta moves by exactly what step_out reports
        const int c = idx[tid];
        const double d = lr * y[tid];
        if (c >= 0 && c < n_theta) theta[c] = theta[c] + d, step_out[c] = d;    // (after the barriers above: the zeros are written)
    }
    if (tid == 0) *info = 0;
}

// The same step inside a box and a per-entry trust region (DeviceQLearning's trust_radius, theta_bounds, theta_scale), one workgroup:
//     Delta = argmin 1/2 D' H D - lr bb' D   subject to  l_a <= D_a <= u_a,
//     l_a = max(lo_c - theta_c, -radius scale_c),  u_a = min(hi_c - theta_c, +radius scale_c),  c = idx[a]
// with H, bb and the codes -1 and a + 1 of qlearning_gn_apply_kernel (H is factored whole first, for those codes).  A strictly convex box
// QP, solved exactly by a primal active-set method (mpc4rl_amd.qlearning.qlearning_gn_box_step states it in torch, step for step):
//   l_a <= u_a fails (or a bound, theta_c or scale_c is NaN) for some a:  info = -2;
//   x = clamp(0, l, u) (theta may start outside [lo, hi]: the step then moves it back); the entries that start on a bound are active;
//   every iteration solves the free block, H_FF z = lr bb_F - H_FB x_B, by gn_chol_solve on the compacted block;
//   some z_a outside [l_a, u_a]: x moves towards z up to the first blocking bound (the lowest entry on a tie), which it takes exactly and
//   which becomes active;
//   else x_F = z and r = H x - lr bb: of the active entries with l_a < u_a whose multiplier has the wrong sign by more than tol_a / 2,
//   tol_a = 4 (3 K + 1) eps (sum_c sqrt(H_aa H_cc) |x_c| + lr |bb_a|) (the backward error of the solve: a multiplier below it is rounding,
//   and releasing on it could cycle), the one with the largest |r_a| / sqrt(H_aa) (the choice is covariant under a rescaling of the
//   parameters, as the ratio test is) is released; none: done.
// A strictly convex QP has finitely many working sets and the objective falls with every move, so this terminates; the count has no
// useful bound in theory.  From x = clamp(0, l, u) an entry typically enters the working set once and some leave it and enter again on
// the other side: on every problem of tests/test_gpu_qlearning_gn_box.py and tests/test_qlearning_gn_box_cpu.py the count stayed below
// 2 K (113 at K = 64 with all 64 bounds active), and the chain run of profiles/qlearning_gn_box_microbench.txt reached 85 at K = 40.
// gn_box_iteration_cap, 8 K + 16, is about four times that; hitting it is info = -3.
// On every code but 0 theta is untouched, step_out = 0 and active = 0.  Else, with contraction off, theta_c = min(max(theta_c + Delta_a,
// lo_c), hi_c) (the clamp: theta_c + (lo_c - theta_c) may round to a neighbour of lo_c), step_out[c] = Delta_a (an active entry: l_a or
// u_a bit for bit), active[a] = 0 free / 1 at l / 2 at u (l_a = u_a: by the sign of r_a), info = {0, iterations}.
// The whole of H stays in LDS beside the working block: the strict upper triangle keeps H, hd its diagonal, and the lower triangle with
// the diagonal is what gn_chol_solve factors.  Fixed order everywhere, no atomics: the same inputs give the same bits.
__host__ __device__ constexpr int gn_box_iteration_cap(int K) { return 8 * K + 16; }

__global__ void __launch_bounds__(GN_APPLY_NT) qlearning_gn_apply_box_kernel(const double *msg, int K, const int *idx, int n_theta, double lr, double damping,
                                                                             const double *lo, const double *hi, const double *scale, double radius,
                                                                             double *theta, double *step_out, uint8_t *active, int *info) {
    __shared__ double H[GN_KMAX * GN_KMAX];
    __shared__ double y[GN_KMAX], hd[GN_KMAX], gs[GN_KMAX], lb[GN_KMAX], ub[GN_KMAX], xs[GN_KMAX];
    __shared__ int st[GN_KMAX], fr[GN_KMAX];
    __shared__ double dmax_s;
    // the free entries' count; whether the step was blocked (before the loop: the box is empty); whether an entry was released.  One
    // flag per decision: a lane may still be reading the first while the first wavefront writes the second
    __shared__ int m_s, blk_s, rel_s;
    const int tid = threadIdx.x, KK = K * (K + 1) / 2;
    const double count = msg[KK + K + 1];
    const double n = count > 1.0 ? count : 1.0;
    for (int i = tid; i < n_theta; i += GN_APPLY_NT) step_out[i] = 0.0;
    if (tid < K) active[tid] = 0;
    for (int e = tid; e < K * K; e += GN_APPLY_NT) {
        const int i = e / K, j = e - i * K;
        if (j <= i) {
            const double v = msg[j * K - j * (j - 1) / 2 + (i - j)] / n;
            H[i * GN_KMAX + j] = v;
            if (j < i) H[j * GN_KMAX + i] = v;
        }
    }
    if (tid < K) gs[tid] = lr * (msg[KK + tid] / n);
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
        if (tid == 0) info[0] = -1, info[1] = 0;
        return;
    }
    if (tid < 64) {                             // the first wavefront holds one entry per lane from here on
        bool bad = false;
        if (tid < K) {
#pragma clang fp contract(off)
            const double g = H[tid * GN_KMAX + tid];
            const double h = g + damping * (g > 0.0 ? g : 1e-12 * d_max);
            H[tid * GN_KMAX + tid] = h, hd[tid] = h;
            y[tid] = gs[tid];
            const int c = idx[tid];
            double l = 0.0, u = 0.0;            // an entry outside theta cannot move
            if (c >= 0 && c < n_theta) {
                const double t = radius * scale[c], a = lo[c] - theta[c], b = hi[c] - theta[c];
                l = (a > -t || a != a) ? a : -t;
                u = (b < t || b != b) ? b : t;
            }
            bad = !(l <= u);
            double x = l > 0.0 ? l : (u < 0.0 ? u : 0.0);
            const int s = x == l ? 1 : (x == u ? 2 : 0);
            x = s == 1 ? l : (s == 2 ? u : x);  // (the bound's own bits: -0.0 stays -0.0)
            lb[tid] = l, ub[tid] = u, xs[tid] = x, st[tid] = s;
        }
        const unsigned long long any_bad = __ballot(bad);
        if (tid == 0) blk_s = any_bad != 0ull;
    }
    __syncthreads();
    if (blk_s) {
        if (tid == 0) info[0] = -2, info[1] = 0;
        return;
    }
    {
        const int fail = gn_chol_solve(H, y, K, tid);
        if (fail >= 0) {
            if (tid == 0) info[0] = fail + 1, info[1] = 0;
            return;
        }
    }
    const double tol_c = 4.0 * (3 * K + 1) * 0x1p-53;
    double r = 0.0;                             // lane a < K: the multiplier of entry a at the last point
    bool first = true;
    int it = 0;
    for (;;) {
        // the free entries, in order: lane a's place among them is the number of free lanes below it
        if (tid < 64) {
            const bool fre = tid < K && st[tid] == 0;
            const unsigned long long mask = __ballot(fre);
            if (fre) fr[__popcll(mask & ((1ull << tid) - 1ull))] = tid;
            if (tid == 0) m_s = __popcll(mask);
        }
        __syncthreads();
        const int m = m_s;
        if (it == gn_box_iteration_cap(K)) {
            if (tid == 0) info[0] = -3, info[1] = it;
            return;
        }
        ++it;
        if (!(first && m == K)) {               // (else the factorisation above is this iteration's)
            for (int e = tid; e < m * m; e += GN_APPLY_NT) {
                const int p = e / m, q = e - p * m;
                if (q < p) H[p * GN_KMAX + q] = H[fr[q] * GN_KMAX + fr[p]];       // fr[q] < fr[p]: the kept upper triangle
                else if (q == p) H[p * GN_KMAX + p] = hd[fr[p]];
            }
            // (the block is written into the lower triangle and read from the strict upper one and hd, as the right-hand side is: no lane
            // reads what another writes)
            if (tid < m) {
                const int a = fr[tid];
                double s = gs[a];
                for (int c = 0; c < K; ++c)
                    if (st[c] != 0) s -= (c < a ? H[c * GN_KMAX + a] : H[a * GN_KMAX + c]) * xs[c];
                y[tid] = s;
            }
            __syncthreads();
            const int fail = gn_chol_solve(H, y, m, tid);
            if (fail >= 0) {                    // (H is positive definite, so every principal block is: not reached in exact arithmetic)
                if (tid == 0) info[0] = fr[fail] + 1, info[1] = it;
                return;
            }
        }
        first = false;
        if (tid < 64) {
            // the ratio test: the first bound the segment from x to z crosses
            double alpha = INFINITY, z = 0.0, xa = 0.0;
            int a = 0, side = 0;
            if (tid < m) {
#pragma clang fp contract(off)
                a = fr[tid], z = y[tid], xa = xs[a];
                if (z > ub[a]) alpha = (ub[a] - xa) / (z - xa), side = 2;
                else if (z < lb[a]) alpha = (lb[a] - xa) / (z - xa), side = 1;
            }
            double am = alpha;
            int pm = tid;
            for (int o = 32; o > 0; o >>= 1) {
                const double ao = __shfl_xor(am, o);
                const int po = __shfl_xor(pm, o);
                if (ao < am || (ao == am && po < pm)) am = ao, pm = po;
            }
            if (am < INFINITY) {                // blocked: move to the bound, which joins the working set
                if (tid < m) {
#pragma clang fp contract(off)
                    if (tid == pm) {
                        xs[a] = side == 2 ? ub[a] : lb[a], st[a] = side;
                    } else {
                        double xn = xa + am * (z - xa);
                        xn = xn < lb[a] ? lb[a] : (xn > ub[a] ? ub[a] : xn);
                        xs[a] = xn;
                    }
                }
                if (tid == 0) blk_s = 1;
            } else {
                if (tid < m) xs[a] = z;
                if (tid == 0) blk_s = 0;
            }
        }
        __syncthreads();
        if (blk_s) continue;
        if (tid < 64) {
            // the multipliers at x, and the active entry to release
            double score = -INFINITY;
            if (tid < K) {
#pragma clang fp contract(off)
                const double ra = sqrt(hd[tid]);
                double s = 0.0, w = 0.0;
                for (int c = 0; c < K; ++c) {
                    const double h = c < tid ? H[c * GN_KMAX + tid] : (c == tid ? hd[tid] : H[tid * GN_KMAX + c]);
                    s += h * xs[c];
                    w += sqrt(hd[c]) * fabs(xs[c]);
                }
                r = s - gs[tid];
                const double tol = tol_c * (ra * w + fabs(gs[tid]));
                const double v = st[tid] == 1 ? -r : r;
                if (st[tid] != 0 && lb[tid] < ub[tid] && v > 0.5 * tol) score = v / ra;
            }
            double sm = score;
            int pm = tid;
            for (int o = 32; o > 0; o >>= 1) {
                const double so = __shfl_xor(sm, o);
                const int po = __shfl_xor(pm, o);
                if (so > sm || (so == sm && po < pm)) sm = so, pm = po;
            }
            if (sm > -INFINITY) {
                if (tid == pm) st[tid] = 0;
                if (tid == 0) rel_s = 1;
            } else if (tid == 0) rel_s = 0;
        }
        __syncthreads();
        if (!rel_s) break;
    }
    if (tid < K) {
#pragma clang fp contract(off)      // theta + step with the step rounded first, then the clamp
        const int c = idx[tid];
        const double d = xs[tid];
        if (c >= 0 && c < n_theta) {
            double t = theta[c] + d;
            t = t < lo[c] ? lo[c] : (t > hi[c] ? hi[c] : t);
            theta[c] = t, step_out[c] = d;      // (after the barriers above: the zeros are written)
        }
        active[tid] = (uint8_t)(lb[tid] == ub[tid] ? (r >= 0.0 ? 1 : 2) : st[tid]);
    }
    if (tid == 0) info[0] = 0, info[1] = it;
}

}  // namespace mpcrl
