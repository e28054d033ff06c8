// The fixed-order batch sum of the learners' gradient kernels (dpg_grad_kernel, qlearning_td_grad_kernel, ppo_surrogate_kernel): a
// weighted sum of sensitivity rows over a batch, in ONE launch and without floating-point atomics — the same inputs give the same bits
// whatever the scheduling.
//   1. every workgroup sums its block of rows into its row of `partial` (block_weighted_colsum);
//   2. the LAST workgroup to finish (last_workgroup: a ticket counter) adds the partials (sliced_final_sum): four slices of the blocks
//      per entry, each slice in block order, the slices added in order.
// Non-finite sensitivities are read as nan_to_num does.
#pragma once
#include <hip/hip_runtime.h>

namespace mpcrl {

__device__ inline double nan_to_num_d(double v) {
    return v != v ? 0.0 : (v > 1.7976931348623157e308 ? 1.7976931348623157e308 : (v < -1.7976931348623157e308 ? -1.7976931348623157e308 : v));
}

// partial_row[p] = sum_{k < nr} w[k] nan_to_num(base[k n_p + p]) for p < n_p: one lane per column (stride NT, the block size), the rows in
// order, eight loads in flight per lane.  (A row that is left out has weight 0 and is read all the same — nan_to_num makes every entry
// finite, 0 x finite = 0: no branch.)  Sensitivities of nu components per batch row, base [.][nu][n_p] with w [.][nu], are nr x nu rows
// here: the batch rows in order, the components 0 .. nu-1 in order inside a row.
template <int NT>
__device__ __forceinline__ void block_weighted_colsum(const double *w, const double *base, int nr, int n_p, double *partial_row) {
    for (int p = threadIdx.x; p < n_p; p += NT) {
        double acc = 0.0;
        int k = 0;
        for (; k + 8 <= nr; k += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = base[(long)(k + q) * n_p + p];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = fma(w[k + q], nan_to_num_d(v[q]), acc);
        }
        for (; k < nr; ++k) acc = fma(w[k], nan_to_num_d(base[(long)k * n_p + p]), acc);
        partial_row[p] = acc;
    }
}

// The hand-off: true, to every lane, in the last workgroup of the grid to get here — what the others wrote to global memory before the
// call is visible to it after.  *ticket is zero before the first launch and is left zero.
__device__ __forceinline__ bool last_workgroup(unsigned int *ticket) {
    __shared__ bool last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
        if (last) *ticket = 0u;      // (every workgroup has taken its ticket)
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    return true;
}

// emit(p, sum_{k < nb} partial[k P + p]) for p < P, by one workgroup of NT lanes, PMAX entries at a time.  (A dependent chain of loads over
// the blocks would cost their latency each: four slices of the blocks per entry, eight loads in flight, the slices added in order.)
template <int PMAX, int NT, class Emit>
__device__ __forceinline__ void sliced_final_sum(const double *partial, int nb, int P, Emit emit) {
    __shared__ double fin[4][PMAX];
    const int per = (nb + 3) / 4;
    for (int p0 = 0; p0 < P; p0 += PMAX) {
        const int np = P - p0 < PMAX ? P - p0 : PMAX;
        for (int e = threadIdx.x; e < 4 * np; e += NT) {
            const int sl = e / np, p = p0 + e - sl * np;
            const int lo = sl * per, hi = lo + per < nb ? lo + per : nb;
            double acc = 0.0;
            int k = lo;
            for (; k + 8 <= hi; k += 8) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = partial[(long)(k + q) * P + p];
#pragma unroll
                for (int q = 0; q < 8; ++q) acc += v[q];
            }
            for (; k < hi; ++k) acc += partial[(long)k * P + p];
            fin[sl][e - sl * np] = acc;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < np; e += NT) emit(p0 + e, ((fin[0][e] + fin[1][e]) + fin[2][e]) + fin[3][e]);
        __syncthreads();
    }
}

}  // namespace mpcrl
