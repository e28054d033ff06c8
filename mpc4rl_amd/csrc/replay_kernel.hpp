// Replay-side glue of the TD3 loop (round 6): what DeviceReplayBuffer.sample + iterates_of_last_sample (mpc4rl_amd/td3.py — the batched
// form of stable_baselines3's ReplayBuffer.sample as scripts/cartpole_mpc_as_td3_agent_closed_loop.py:47-58 uses it) do with ~22 framework
// launches (gather, integer index arithmetic, masks, float64 copies of the states for the two replay solves), in one launch, one lane per
// sampled transition.  Nothing is computed in floating point: every output is a copy, a widening or an integer expression.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_sum.hpp"

namespace mpcrl {

struct ReplaySampleArgs {
    const float *table;       // [cap * E][row_len]: obs (nx) | next obs (nx) | action (nu) | reward | done
    int row_len, nx, B, E, cap, steps;
    const int64_t *idx;       // [B] sampled rows (step * E + env)
    const int64_t *pos_t;     // [1] the slot the roll-out writes next
    int exclude;              // != 0: that slot is being written WHILE this batch is drawn (pipelined loop): idx counts the rows of the other cap - 1 slots
    const uint8_t *iter_ok;   // [cap * E] or nullptr: the roll-out solve stored with the transition converged
    float *rows;              // [B][row_len]
    double *obs64, *nxt64;    // [B][nx]
    int64_t *row_s, *row_n;   // [B] rows of the iterate tables to start the solves at obs / next obs from
    int32_t *cold_s, *cold_n; // [B] 1 = that stored iterate is not a starting point
};

__global__ void __launch_bounds__(256) replay_sample_kernel(const ReplaySampleArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    int64_t i = a.idx[b];
    if (a.exclude) {      // row of the k-th slot after the excluded one
        const int64_t st = i / a.E;
        i = ((a.pos_t[0] + 1 + st) % a.cap) * a.E + (i - st * a.E);
    }
    const float *r = a.table + i * a.row_len;
    int64_t n = i;
    if (a.iter_ok) {
        // the iterate for next obs: the roll-out solution of the NEXT step of the same environment where that exists and IS that state —
        // the slot is neither the one about to be overwritten (or being written: exclude) nor one not yet written, the episode did not
        // terminate, and the obs stored there equals this row's next obs entry for entry — else the one at obs.  The done column
        // holds `terminated` alone (the TD target's flag): an episode cut off at the time limit resets its environment with the flag at
        // 0, and only the comparison tells that row's obs (the reset state) from next obs.  Both are the same double rounded to float
        // by the same cast where the episode went on; a NaN never compares equal (the safe side).  The next row is read only after
        // the two slot tests passed: a slot that is being written or was never written is not touched.  (Ahead of the copies below
        // and without a short circuit: these loads wait for nothing but the index.)
        const int64_t step = i / a.E, env = i - step * a.E, nstep = (step + 1) % a.cap;
        if (nstep != a.pos_t[0] && nstep < a.steps) {
            const float *q = a.table + (nstep * a.E + env) * a.row_len;
            bool cont = r[a.row_len - 1] == 0.0f;
#pragma unroll 4
            for (int k = 0; k < a.nx; ++k) cont &= q[k] == r[a.nx + k];
            if (cont) n = nstep * a.E + env;
        }
    }
    float *o = a.rows + (long)b * a.row_len;
    for (int k = 0; k < a.row_len; ++k) o[k] = r[k];
    for (int k = 0; k < a.nx; ++k) a.obs64[(long)b * a.nx + k] = (double)r[k], a.nxt64[(long)b * a.nx + k] = (double)r[a.nx + k];
    if (a.iter_ok) {
        a.row_s[b] = i, a.row_n[b] = n;
        a.cold_s[b] = a.iter_ok[i] ? 0 : 1, a.cold_n[b] = a.iter_ok[n] ? 0 : 1;
    }
}

// The deterministic policy gradient's contraction (round 6): out[p] = sum_b ok_b sum_u dq_da[b][u] chain_u dpi_dp[b][u][p], out[n_p] = sum_b ok_b
// with chain_u = 2 / (hi_u - lo_u) (the derivative of MPC.scale_action, rlmpc/mpc/common/mpc.py:290-301; 1 without scaling) — the step
// the reference leaves as a stub (rlmpc/td3/policies.py:332).  ~14 framework launches, the batch sum of [4096 x 83] doubles alone 48 us,
// in ONE: the fixed-order batch sum of batch_sum.hpp over blocks of DPG_ROWS rows, a (row, control) pair k = r nu + u being one term.
constexpr int DPG_ROWS = 32, DPG_PMAX = 256;

struct DpgArgs {
    const float *dq_da;      // [B][nu]
    const uint8_t *ok;       // [B] or nullptr
    const double *dpi_dp;    // [B][nu][n_p]
    int B, nu, n_p, scale;
    const double *lo, *hi;   // [nu]
    double *partial;         // [n_blocks][n_p + 1]
    unsigned int *ticket;    // [1], zero before the first launch (the kernel leaves it zero)
    double *out;             // [n_p + 1]
};

__global__ void __launch_bounds__(128) dpg_grad_kernel(const DpgArgs a) {
    __shared__ double w[DPG_ROWS * 8];      // the terms' weights (nu <= 8), 0 for a row that is left out
    __shared__ double cnt;
    const int b0 = blockIdx.x * DPG_ROWS, P1 = a.n_p + 1;
    for (int e = threadIdx.x; e < DPG_ROWS * a.nu; e += 128) {
        const int r = e / a.nu, u = e - r * a.nu, b = b0 + r;
        const bool ok = b < a.B && (!a.ok || a.ok[b]);
        const double chain = a.scale ? 2.0 / (a.hi[u] - a.lo[u]) : 1.0;
        w[e] = ok ? (double)a.dq_da[(long)b * a.nu + u] * chain : 0.0;
    }
    if (threadIdx.x == 0) {
        double n = 0.0;
        for (int r = 0; r < DPG_ROWS; ++r) n += (b0 + r < a.B && (!a.ok || a.ok[b0 + r])) ? 1.0 : 0.0;
        cnt = n;
    }
    __syncthreads();
    const int nr = (a.B - b0 < DPG_ROWS ? a.B - b0 : DPG_ROWS) * a.nu;      // terms of this workgroup
    double *row = a.partial + (long)blockIdx.x * P1;
    block_weighted_colsum<128>(w, a.dpi_dp + (long)b0 * a.nu * a.n_p, nr, a.n_p, row);
    if (threadIdx.x == 0) row[a.n_p] = cnt;
    if (!last_workgroup(a.ticket)) return;
    sliced_final_sum<DPG_PMAX, 128>(a.partial, gridDim.x, P1, [&](int p, double s) { a.out[p] = s; });
}

}  // namespace mpcrl
