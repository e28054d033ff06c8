// PPO's value function as library kernels (round 8): what mpc4rl_amd/ppo.py asks of its 4 -> 64 -> 64 -> 1 tanh MLP —
//     predict_values:   V(obs_b)                                                 (a cast, three products of [n x 64], two tanh launches, a cast back)
//     the value step:   valid_b = idx[b] inside the table and OBS[idx[b]], RET[idx[b]] finite   (an invalid row is SELECTED out)
//                       e_b     = valid_b ? V(OBS[idx[b]]) - (float)RET[idx[b]] : 0
//                       loss    = vf_coef sum_b e_b^2 / max(1, sum_b valid_b),     grad = d loss / d (parameters of V)
//                       (two index_selects, two casts, the forward pass, the MSE and autograd's backward pass)
// — as value_forward_kernel (one launch) and value_mse_partial_kernel + value_mse_reduce_kernel (two).  critic_kernel.hpp is the model:
// one workgroup per VALUE_S = 16 rows, lane j = hidden unit j, row j of W2 in registers for the forward pass and column j for the
// backward pass (one coalesced read of the matrix by the whole workgroup, transposed through LDS), the workgroup's rows and activations in
// LDS, read as broadcasts.  fp32 FMAs on the vector ALU for the network (inputs are PPO's float64 tables, rounded to float on load as
// `.to(torch.float32)` does); every sum over rows — the weight and bias gradients, the loss, the count — is accumulated in fp64 in a fixed
// order: within a workgroup over its rows 0 .. 15, then over the workgroups' partials in block order.  No floating-point atomics, no
// ticket: the workspace is written in full before it is read, so it needs no initialisation.
//
// Four wavefronts per workgroup, one per SIMD (a lone wavefront per SIMD is bound by its own issue rate).  The passes
// that run along a row (forward, and backward to the first layer's pre-activation) give each wavefront four of the 16 rows; the weight
// gradients, which sum over rows, give each wavefront a quarter of the OUTPUT instead — 16 of lane j's 64 entries of dW2 (fp64
// accumulators: 32 registers) and every fourth column of dW1 — so that no sum is split between wavefronts and nothing has to be added
// through LDS afterwards.  tanh' = 1 - h^2 from the stored activation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcrl {

constexpr int VALUE_H = 64;        // hidden width (both layers): the lane count of a wavefront
constexpr int VALUE_S = 16;        // rows per workgroup
constexpr int VALUE_DMAX = 16;     // inputs of the first layer (nx)
constexpr int VALUE_NT = 256;      // lanes per workgroup: four wavefronts
constexpr int VALUE_SW = VALUE_S / 4;      // rows per wavefront in the row-wise passes

__host__ __device__ inline int value_n_params(int D) { return VALUE_H * D + VALUE_H + VALUE_H * VALUE_H + VALUE_H + VALUE_H + 1; }

// LDS of one workgroup's forward pass
struct ValueTile {
    float w2[VALUE_H][VALUE_H + 1];                                  // W2 (read by rows, later by columns)
    __attribute__((aligned(16))) float x[VALUE_S][VALUE_DMAX];       // the rows' inputs, zero beyond nx
    __attribute__((aligned(16))) float h1[VALUE_S][VALUE_H];         // first-layer activations
    float h2[VALUE_S][VALUE_H];                                      // second-layer activations
    float ps[VALUE_S][VALUE_H + 1];                                  // per-lane pieces of the output sum
};

// W2 to LDS, 16 coalesced loads per lane (a wavefront writes one row of the LDS image per load: consecutive banks)
__device__ inline void value_stage_w2(ValueTile &t, const float *params, int D) {
    const float *W2 = params + VALUE_H * D + VALUE_H;
#pragma unroll
    for (int k = 0; k < VALUE_H * VALUE_H / VALUE_NT; ++k) {
        const int e = k * VALUE_NT + threadIdx.x;
        t.w2[e >> 6][e & 63] = W2[e];
    }
}

// Forward pass of the workgroup's 16 rows (t.x and t.w2 written by the caller, no barrier yet): h1, h2 to LDS; returns V of row lane / 4
// (every wavefront computes all 16, four lanes per row hold the same value).  w3 is handed back for the backward pass.
__device__ inline float value_tile_forward(ValueTile &t, const float *params, int D, float &w3) {
    constexpr int H = VALUE_H;
    const int w = threadIdx.x >> 6, j = threadIdx.x & 63, s0 = w * VALUE_SW, s1 = s0 + VALUE_SW;
    const float *W1 = params, *B1 = W1 + H * D, *B2 = B1 + H + H * H, *W3 = B2 + H, *B3 = W3 + H;
    float w1r[VALUE_DMAX];
#pragma unroll
    for (int d = 0; d < VALUE_DMAX; ++d) w1r[d] = d < D ? W1[j * D + d] : 0.0f;
    const float b1 = B1[j], b2 = B2[j], b3 = B3[0];
    w3 = W3[j];
    __syncthreads();
    float w2r[H];
#pragma unroll
    for (int i = 0; i < H; ++i) w2r[i] = t.w2[j][i];
    // (the loops over the rows stay rolled: straight-line code that runs once is paid in instruction fetches)
#pragma unroll 2
    for (int s = s0; s < s1; ++s) {
        float z = b1;
#pragma unroll
        for (int d = 0; d < VALUE_DMAX; d += 4) {
            if (d >= D) break;      // (uniform)
            const float4 v = *(const float4 *)&t.x[s][d];
            z = fmaf(w1r[d], v.x, z), z = fmaf(w1r[d + 1], v.y, z), z = fmaf(w1r[d + 2], v.z, z), z = fmaf(w1r[d + 3], v.w, z);
        }
        t.h1[s][j] = tanhf(z);
    }
    __syncthreads();
#pragma unroll 2
    for (int s = s0; s < s1; ++s) {
        float z0 = b2, z1 = 0.0f;
#pragma unroll
        for (int i = 0; i < H; i += 8) {
            const float4 h = *(const float4 *)&t.h1[s][i], k = *(const float4 *)&t.h1[s][i + 4];
            z0 = fmaf(w2r[i], h.x, z0), z0 = fmaf(w2r[i + 1], h.y, z0), z0 = fmaf(w2r[i + 2], h.z, z0), z0 = fmaf(w2r[i + 3], h.w, z0);
            z1 = fmaf(w2r[i + 4], k.x, z1), z1 = fmaf(w2r[i + 5], k.y, z1), z1 = fmaf(w2r[i + 6], k.z, z1), z1 = fmaf(w2r[i + 7], k.w, z1);
        }
        const float h2 = tanhf(z0 + z1);
        t.h2[s][j] = h2;
        t.ps[s][j] = w3 * h2;
    }
    __syncthreads();
    // V[s] for s = lane / 4: the four lanes of a quad sum a quarter of the pieces each
    const int s = j >> 2, k = j & 3;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) q += t.ps[s][k * 16 + i];
    q += __shfl_xor(q, 1, 64);
    q += __shfl_xor(q, 2, 64);
    return q + b3;
}

// values[b] = V(obs[b]).  No masking: a row that is not finite gives a value that is not finite, in that row only.
__global__ void __launch_bounds__(VALUE_NT) value_forward_kernel(const double *obs, long n, int nx, const float *params, double *values) {
    __shared__ ValueTile t;
    const long b0 = (long)blockIdx.x * VALUE_S;
    {
        const int s = threadIdx.x >> 4, i = threadIdx.x & 15;      // 16 x 16 entries = the 256 lanes
        const long b = b0 + s;
        t.x[s][i] = (b < n && i < nx) ? (float)obs[b * nx + i] : 0.0f;
    }
    value_stage_w2(t, params, nx);
    float w3;
    const float q = value_tile_forward(t, params, nx, w3);
    const long b = b0 + (threadIdx.x >> 2);
    if (threadIdx.x < 64 && (threadIdx.x & 3) == 0 && b < n) values[b] = (double)q;
}

struct ValueMseArgs {
    const double *OBS, *RET;      // [n_rows][nx], [n_rows]
    const int64_t *idx;           // [M]
    int M, nx;
    long n_rows;
    const float *params;          // W1 [64][nx] | b1 [64] | W2 [64][64] | b2 [64] | W3 [64] | b3 [1]
    double *partial;              // [n_blocks][n_params + 2]   (per block: the gradient partial, then sum e^2, then the valid count)
};

__global__ void __launch_bounds__(VALUE_NT) value_mse_partial_kernel(const ValueMseArgs a) {
    constexpr int H = VALUE_H, S = VALUE_S;
    const int D = a.nx, w = threadIdx.x >> 6, j = threadIdx.x & 63, b0 = blockIdx.x * S, n_params = value_n_params(D);
    __shared__ ValueTile t;
    __shared__ float ret[S], okf[S];
    __shared__ __attribute__((aligned(16))) float g2s[S][H];      // the second layer's pre-activation gradient
    __shared__ float g1s[S][H];                                    // the first layer's
    // ---- the workgroup's rows: lane = (row, entry), every load in flight at once; entry 0 also fetches the return.  A row is valid
    // when its index is inside the table and its 16 lanes (a quarter of the wavefront) all saw finite numbers
    {
        const int s = threadIdx.x >> 4, i = threadIdx.x & 15, b = b0 + s;
        const long r = b < a.M ? (long)a.idx[b] : -1;
        const bool inr = r >= 0 && r < a.n_rows;
        const double v = (inr && i < D) ? a.OBS[r * D + i] : 0.0, rv = (inr && i == 0) ? a.RET[r] : 0.0;
        const unsigned long long fin = __ballot(isfinite(v) && isfinite(rv));
        const bool ok = inr && ((fin >> (16 * (j >> 4))) & 0xFFFFull) == 0xFFFFull;
        t.x[s][i] = ok ? (float)v : 0.0f;
        if (i == 0) ret[s] = ok ? (float)rv : 0.0f, okf[s] = ok ? 1.0f : 0.0f;
    }
    value_stage_w2(t, a.params, D);
    float w3;
    const float q = value_tile_forward(t, a.params, D, w3);
    // ---- error of row lane / 4 (the same in every wavefront), dV of the unscaled loss (vf_coef and the count multiply in the reduction)
    const float e = okf[j >> 2] != 0.0f ? q - ret[j >> 2] : 0.0f, dq = 2.0f * e;
    // ---- backward along the wavefront's rows: g2 = dq w3 (1 - h2^2), g1 = (W2^T g2) (1 - h1^2)
    const int s0 = w * VALUE_SW, s1 = s0 + VALUE_SW;
    float w2c[H];
#pragma unroll
    for (int i = 0; i < H; ++i) w2c[i] = t.w2[i][j];
#pragma unroll 1
    for (int s = s0; s < s1; ++s) {
        const float h2 = t.h2[s][j];
        g2s[s][j] = __shfl(dq, 4 * s, 64) * w3 * fmaf(-h2, h2, 1.0f);
    }
    __syncthreads();
#pragma unroll 2
    for (int s = s0; s < s1; ++s) {
        float g1a = 0.0f, g1b = 0.0f;
#pragma unroll
        for (int i = 0; i < H; i += 4) {
            const float4 g = *(const float4 *)&g2s[s][i];
            g1a = fmaf(w2c[i], g.x, g1a), g1b = fmaf(w2c[i + 1], g.y, g1b), g1a = fmaf(w2c[i + 2], g.z, g1a), g1b = fmaf(w2c[i + 3], g.w, g1b);
        }
        const float h1 = t.h1[s][j];
        g1s[s][j] = (g1a + g1b) * fmaf(-h1, h1, 1.0f);
    }
    __syncthreads();
    // ---- the sums over the 16 rows, fp64, rows in order.  This wavefront's share of the output: d W2[j][16 w .. 16 w + 15] and
    // d W1[j][w], [w + 4], [w + 8], [w + 12]; the bias and output-layer sums are cheap enough that every wavefront forms them and
    // the first writes them
    double dw2[16], dw1[4];
#pragma unroll
    for (int i = 0; i < 16; ++i) dw2[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) dw1[k] = 0.0;
    double db1 = 0.0, db2 = 0.0, dw3 = 0.0, db3 = 0.0;
#pragma unroll 2
    for (int s = 0; s < S; ++s) {
        const double g2 = (double)g2s[s][j], g1 = (double)g1s[s][j], dqs = (double)__shfl(dq, 4 * s, 64);
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
            const float4 h = *(const float4 *)&t.h1[s][16 * w + i];
            dw2[i] = fma(g2, (double)h.x, dw2[i]), dw2[i + 1] = fma(g2, (double)h.y, dw2[i + 1]);
            dw2[i + 2] = fma(g2, (double)h.z, dw2[i + 2]), dw2[i + 3] = fma(g2, (double)h.w, dw2[i + 3]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w + 4 * k < D) dw1[k] = fma(g1, (double)t.x[s][w + 4 * k], dw1[k]);      // (uniform)
        db1 += g1, db2 += g2, db3 += dqs;
        dw3 = fma(dqs, (double)t.h2[s][j], dw3);
    }
    // ---- the workgroup's partial: the parameters in order, EXCEPT that the 64 x 64 block is stored transposed (lane j writes
    // d W2[j][i] to [i][j]: coalesced; value_mse_reduce_kernel puts it back)
    double *o = a.partial + (long)blockIdx.x * (n_params + 2);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (w + 4 * k < D) o[j * D + w + 4 * k] = dw1[k];
    o += H * D;
    if (w == 0) o[j] = db1;
    o += H;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[(16 * w + i) * H + j] = dw2[i];
    o += H * H;
    if (w == 0) o[j] = db2, o[H + j] = dw3;
    o += 2 * H;
    if (w == 0) {
        // sum of e^2 over the rows: lane 4 s holds row s; a butterfly in a fixed order
        double l = (j & 3) == 0 ? (double)e * (double)e : 0.0;
#pragma unroll
        for (int m = 32; m >= 4; m >>= 1) l += __shfl_xor(l, m, 64);
        if (j == 0) {
            double n = 0.0;
            for (int s = 0; s < S; ++s) n += (double)okf[s];
            o[0] = db3, o[1] = l, o[2] = n;
        }
    }
}

// out[t] = out_scale vf_coef / max(1, n) * sum_blocks partial[block][t] for the gradient (fp64), out[n_params] = vf_coef sum e^2 / max(1, n),
// out[n_params + 1] = n.  A workgroup takes 64 entries; its four wavefronts take a quarter of the blocks each (16 loads in flight per
// lane) and are added in a fixed order.
__global__ void __launch_bounds__(256) value_mse_reduce_kernel(const double *partial, int n_blocks, int D, double vf_coef, double out_scale, double *out) {
    __shared__ double red[256];
    const int n_params = value_n_params(D), stride = n_params + 2;
    double n = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) n += partial[(long)b * stride + n_params + 1];
    red[threadIdx.x] = n;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    const double count = red[0], cnt = count > 1.0 ? count : 1.0;
    __syncthreads();
    const int p = threadIdx.x & 63, sl = threadIdx.x >> 6, t = blockIdx.x * 64 + p;
    const int per = (n_blocks + 3) / 4, lo = sl * per, hi = lo + per < n_blocks ? lo + per : n_blocks;
    double acc = 0.0;
    if (t <= n_params) {
        int b = lo;
        for (; b + 16 <= hi; b += 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = partial[(long)(b + k) * stride + t];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc += v[k];
        }
        for (; b < hi; ++b) acc += partial[(long)b * stride + t];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (sl == 0 && t <= n_params) {
        acc = ((red[p] + red[64 + p]) + red[128 + p]) + red[192 + p];
        if (t < n_params) {
            // where the entry lives in torch's order: the 64 x 64 block comes in transposed
            const int w2 = VALUE_H * D + VALUE_H;
            int dst = t;
            if (t >= w2 && t < w2 + VALUE_H * VALUE_H) dst = w2 + ((t - w2) & 63) * VALUE_H + ((t - w2) >> 6);
            out[dst] = acc * (out_scale * vf_coef) / cnt;
        } else {
            out[n_params] = vf_coef * acc / cnt;
            out[n_params + 1] = count;
        }
    }
}

}  // namespace mpcrl
