// mpcrl_api.hip — the handle's half of the C ABI of libmpcrl_hip.so (include/mpcrl.h): handle management, bounds, packing order,
// iterate access, the launch-shape tuner, and mpcrl_solve with the cartpole / linear-system solve kernels (small_kernel.hpp,
// linear_kernel.hpp), which this unit instantiates: launch_plan.hpp decides which of them a solve launches (choose_shape, dispatch).
// The chain of masses: the table of mpcrl_host.hpp (chain_inst.hip); the handle-less library kernels of the RL loops: mpcrl_loops.hip.
#include "mpcrl_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "small_kernel.hpp"
#include "linear_kernel.hpp"
#include "order_kernel.hpp"
#include "iterate_kernel.hpp"

using namespace mpcrl;

namespace {

template <class T>
int dev_alloc(T **p, size_t n, int64_t &bytes) {
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) return MPCRL_E_NOMEM;
    bytes += (int64_t)(n * sizeof(T));
    return 0;
}

void copy_or_fill(double *dst, const double *src, int n, int cap, double fill) {
    for (int i = 0; i < cap; ++i) dst[i] = (src && i < n) ? src[i] : fill;
}

int fill_small_spec(const MpcrlProblemSpec &s, SmallSpec &d) {
    const int nw = s.nx + s.nu;
    if (nw > SMALL_MAXNW || s.n_consts > SMALL_MAXC || s.N + 1 > 64 || s.N < 2) return MPCRL_E_ARG;
    std::memset(&d, 0, sizeof(d));
    d.N = s.N, d.np = s.np, d.cost_kind = s.cost_kind, d.rk_steps = s.rk_steps, d.max_iter = s.max_iter;
    d.dT = s.dT, d.gamma = s.gamma, d.h = s.h, d.tol = s.tol;
    copy_or_fill(d.lb0, s.lb0, s.nu, SMALL_MAXNW, -MPCRL_NO_BOUND);
    copy_or_fill(d.ub0, s.ub0, s.nu, SMALL_MAXNW, MPCRL_NO_BOUND);
    copy_or_fill(d.lb, s.lb, nw, SMALL_MAXNW, -MPCRL_NO_BOUND);
    copy_or_fill(d.ub, s.ub, nw, SMALL_MAXNW, MPCRL_NO_BOUND);
    copy_or_fill(d.lbe, s.lbe, s.nx, SMALL_MAXNW, -MPCRL_NO_BOUND);
    copy_or_fill(d.ube, s.ube, s.nx, SMALL_MAXNW, MPCRL_NO_BOUND);
    copy_or_fill(d.zl, s.zl, nw, SMALL_MAXNW, 0.0);
    copy_or_fill(d.zu, s.zu, nw, SMALL_MAXNW, 0.0);
    for (int i = 0; i < SMALL_MAXNW; ++i) d.soft[i] = (s.soft && i < nw) ? s.soft[i] : 0;
    copy_or_fill(d.consts, s.consts, s.n_consts, SMALL_MAXC, 0.0);
    return 0;
}

int fill_large_spec(const MpcrlProblemSpec &s, LargeSpec &d) {
    const int nw = s.nx + s.nu;
    if (nw > LARGE_MAXNW || s.nu > 4 || s.N + 1 > 64 || s.N < 1 || s.rk_steps < 1 || s.rk_steps > 2) return MPCRL_E_ARG;
    if (s.soft)
        for (int i = 0; i < nw; ++i)
            if (s.soft[i]) return MPCRL_E_ARG;   // hard bounds only in the large kernel
    std::memset(&d, 0, sizeof(d));
    d.N = s.N, d.np = s.np, d.cost_kind = s.cost_kind, d.rk_steps = s.rk_steps, d.max_iter = s.max_iter;
    d.dT = s.dT, d.gamma = s.gamma, d.h = s.h, d.tol = s.tol;
    copy_or_fill(d.lb0, s.lb0, s.nu, 4, -MPCRL_NO_BOUND);
    copy_or_fill(d.ub0, s.ub0, s.nu, 4, MPCRL_NO_BOUND);
    copy_or_fill(d.lb, s.lb, nw, LARGE_MAXNW, -MPCRL_NO_BOUND);
    copy_or_fill(d.ub, s.ub, nw, LARGE_MAXNW, MPCRL_NO_BOUND);
    copy_or_fill(d.lbe, s.lbe, s.nx, LARGE_MAXNW, -MPCRL_NO_BOUND);
    copy_or_fill(d.ube, s.ube, s.nx, LARGE_MAXNW, MPCRL_NO_BOUND);
    return 0;
}

inline void tuner_harvest(MpcrlSolver::Tuner &t) {   // probes that have finished since the last look (never waits)
    for (int m = 0; m < 2; ++m)
        if (t.pending[m] && hipEventQuery(t.ev[m][1]) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, t.ev[m][0], t.ev[m][1]) == hipSuccess && ms > 0.f) t.ms[m] = ms;
            t.pending[m] = false;
        }
}

// The cartpole solve kernels exist in a third form, BOX (small_kernel.hpp): the full-box bound pattern compiled in.  It is the same
// iteration bit for bit, taken when the handle's bounds are that pattern (box_rows_spec) and MPCRL_GENERIC_ROWS=1 did not switch it off;
// any other bounds run the generic kernels.  The linear system has soft rows and the generic form only.
// every interior bound present, u_0's bounds the interior control bounds and the terminal bounds the interior state bounds, bitwise
inline bool box_rows_spec(const SmallSpec &sp, int nx, int nu) {
    for (int i = 0; i < nx + nu; ++i)
        if (!(std::fabs(sp.lb[i]) < NO_BOUND) || !(std::fabs(sp.ub[i]) < NO_BOUND)) return false;
    return std::memcmp(sp.lb0, sp.lb, nu * sizeof(double)) == 0 && std::memcmp(sp.ub0, sp.ub, nu * sizeof(double)) == 0 &&
           std::memcmp(sp.lbe, sp.lb + nu, nx * sizeof(double)) == 0 && std::memcmp(sp.ube, sp.ub + nu, nx * sizeof(double)) == 0;
}
inline void refresh_box_rows(MpcrlSolver *h) {
    h->box_rows = !h->is_large && !h->generic_rows && h->model == MPCRL_MODEL_CARTPOLE && box_rows_spec(h->small, h->nx, h->nu);
}

// The launch plan (launch_plan.hpp) of the handle's next solve with these flags on stream `st`, for the query (commit = false: the
// shape it answers with becomes the promise the next solve keeps) and for the solve itself (commit = true: harvests the probes, keeps
// the promise, counts the call; *probe = the shape to time with the tuner's events, -1 = this call is not a probe).  In automatic
// mode a candidate that passes the rule takes the tuner's shape; every other input has one plan.
SmallPlan choose_shape(MpcrlSolver *h, int flags, hipStream_t st, bool commit, int *probe = nullptr) {
    const SmallTraits tr = h->model == MPCRL_MODEL_LINEAR ? small_traits<LinearDev>() : small_traits<CartpoleDev>();
    auto plan = [&](int shape) { return plan_small(tr, h->N, h->B, h->n_simd, flags, h->slice_mode, h->box_rows, h->linear_spl, shape); };
    SmallPlan p = plan(TUNE_SLICED);
    int promise = -1;
    if (h->slice_mode == 0 && p.candidate && p.by_rule) {
        // No event calls while the stream is being captured into a graph (they would end the capture): nothing is timed, counted or
        // promised, and the graph gets the shape preferred so far.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        const bool query_failed = hipStreamIsCapturing(st, &cap) != hipSuccess;
        if (query_failed) (void)hipGetLastError();   // (not sticky for the caller's next HIP call)
        MpcrlSolver::Tuner &t = h->tune[(flags & MPCRL_COLD) ? 0 : 1];
        int shape = tuned_best(t);
        if (!query_failed && cap == hipStreamCaptureStatusNone) {
            if (commit) tuner_harvest(t);
            bool timed = false;
            const int by_count = tuned_shape(t, &timed);
            shape = (commit && h->planned >= 0) ? h->planned : by_count;   // a promise made before the harvest above stands
            if (!commit) promise = shape;
            if (commit && timed && shape == by_count && !t.pending[shape]) *probe = shape;
            if (commit) t.calls++;
        }
        if (shape == TUNE_PLAIN) p = plan(TUNE_PLAIN);
    }
    h->planned = promise;
    return p;
}

// calls f with std::true_type if `on`, else with std::false_type; CAN = the instantiations of the true side exist for this model
template <bool CAN, class F>
void with_switch(bool on, F &&f) {
    if constexpr (CAN)
        if (on) return f(std::true_type());
    f(std::false_type());
}

// Launches what the plan says: the one place a plan's fields become template arguments, one table per family.  Only the
// instantiations a plan of model M can name exist: SHORT without seg_skip, BOX for cartpole, the time-sliced kernel without soft
// bounds, LDS parking of a full-tree instance where the cap has room (lds_park_reachable).  probe_end (may be null) is recorded
// behind the solve launch, before the sensitivity launch.
template <class M>
int dispatch(const SmallPlan &p, const SmallSpec &sp, const SmallArgs &a, hipStream_t st, hipEvent_t probe_end) {
    constexpr SmallTraits T = small_traits<M>();
    const dim3 grid(p.grid), wave(64);
    with_switch<!T.seg_skip>(p.seg_short, [&](auto s) {
        with_switch<T.box_rows>(p.box, [&](auto b) {
            constexpr bool SHORT = decltype(s)::value, BOX = decltype(b)::value;
            if (p.family == SmallPlan::PLAIN) hipLaunchKernelGGL((small_solve_kernel<M, SHORT, BOX>), grid, wave, 0, st, sp, a);
            if constexpr (!T.has_soft)
                if (p.family == SmallPlan::SLICED)
                    with_switch<lds_park_reachable(T, SHORT)>(p.lds_park, [&](auto l) {
                        with_switch<true>(p.warm, [&](auto w) {
                            hipLaunchKernelGGL((small_solve_sliced_kernel<M, decltype(l)::value, decltype(w)::value, SHORT, BOX>), grid, wave, 0, st, sp, a);
                        });
                    });
        });
    });
    if constexpr (T.lq)
        if (p.family == SmallPlan::LQ) {
            if (p.lq_spl == 4) hipLaunchKernelGGL((lq_solve_kernel<4, 16>), grid, wave, 0, st, sp, a);
            if (p.lq_spl == 3 && p.lq_rl == 16) hipLaunchKernelGGL((lq_solve_kernel<3, 16>), grid, wave, 0, st, sp, a);
            if (p.lq_spl == 3 && p.lq_rl == 8) hipLaunchKernelGGL((lq_solve_kernel<3, 8>), grid, wave, 0, st, sp, a);
        }
    if constexpr (std::is_same<M, CartpoleDev>::value)
        if (p.family == SmallPlan::EXACT) hipLaunchKernelGGL(small_solve_kernel<CartpoleDevExact>, grid, wave, 0, st, sp, a);
    HIP_OK(hipGetLastError());
    if (probe_end) HIP_OK(hipEventRecord(probe_end, st));
    if (p.sens_grid) {
        with_switch<!T.seg_skip>(p.seg_short, [&](auto s) {
            hipLaunchKernelGGL((small_sens_kernel<M, decltype(s)::value>), dim3(p.sens_grid), wave, 0, st, sp, a);
        });
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int launch_small(MpcrlSolver *h, const SmallArgs &a, hipStream_t st) {
    int probe = -1;
    const SmallPlan p = choose_shape(h, a.flags, st, true, &probe);
    MpcrlSolver::Tuner &t = h->tune[(a.flags & MPCRL_COLD) ? 0 : 1];
    if (probe >= 0) {
        if (!t.ev[0][0])
            for (auto &pair : t.ev)
                for (auto &e : pair) HIP_OK(hipEventCreate(&e));
        HIP_OK(hipEventRecord(t.ev[probe][0], st));
    }
    const hipEvent_t probe_end = probe >= 0 ? t.ev[probe][1] : nullptr;
    const int rc = h->model == MPCRL_MODEL_LINEAR ? dispatch<LinearDev>(p, h->small, a, st, probe_end) : dispatch<CartpoleDev>(p, h->small, a, st, probe_end);
    if (!rc && probe >= 0) t.pending[probe] = true;
    return rc;
}

// writes the cold iterate (MPC.reset) into the stored-iterate arrays; x0 may be null (x_k = 0)
int fill_cold_iterate(MpcrlSolver *h, const double *x0, bool primal, hipStream_t st) {
    const long n = (long)h->B * 10 * (h->N + 1) * (h->nx + h->nu);
    hipLaunchKernelGGL(cold_iterate_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 4096)), dim3(256), 0, st, x0, h->B, h->N, h->nx, h->nu,
                       primal ? h->X : nullptr, primal ? h->U : nullptr, primal ? h->PI : nullptr, h->BND);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

#ifdef MPCRL_PROFILE_PHASES
int mpcrl_debug_phases(unsigned long long *out, int reset) {   // summed over the translation units (each has its own counters)
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_ticks), sizeof(unsigned long long) * 16));
    if (reset) {
        unsigned long long z[16] = {0};
        HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_ticks), z, sizeof(z)));
    }
    for (int n = 3; n <= 7; ++n) {
        unsigned long long t[16];
        if (!chain_entry(n)->debug_phases) continue;
        const int rc = chain_entry(n)->debug_phases(t, reset);
        if (rc) return rc;
        for (int i = 0; i < 16; ++i) out[i] += t[i];
    }
    return 0;
}
#endif

int mpcrl_version(void) { return MPCRL_ABI_VERSION; }

int mpcrl_debug_seg_reduce(const double *in, int lpi, int n_max, int n_sum, int which, double *out, void *stream) {
    if (!in || !out || lpi < 1 || lpi > 64 || which < 0 || which > 2) return MPCRL_E_ARG;
    ON_DEVICE_OF(out);
    const hipStream_t st = (hipStream_t)stream;
#define MPCRL_SEG_PROBE(NM, NS) \
    if (n_max == NM && n_sum == NS) { \
        hipLaunchKernelGGL((seg_probe_kernel<NM, NS>), dim3(1), dim3(64), 0, st, in, lpi, which, out); \
        HIP_OK(hipGetLastError()); \
        return 0; \
    }
    // the shapes the kernels reduce (small_kernel.hpp): single sums and maxima, the interior point's three passes, the SQP round's
    MPCRL_SEG_PROBE(0, 1) MPCRL_SEG_PROBE(1, 0) MPCRL_SEG_PROBE(1, 1) MPCRL_SEG_PROBE(2, 2) MPCRL_SEG_PROBE(1, 2) MPCRL_SEG_PROBE(4, 1)
#undef MPCRL_SEG_PROBE
    return MPCRL_E_ARG;
}

int mpcrl_debug_launch_plan(int model, int N, int B, int n_simd, int flags, int slice_mode, int box_rows, int linear_spl, int shape, int32_t out[12]) {
    if ((model != MPCRL_MODEL_CARTPOLE && model != MPCRL_MODEL_LINEAR) || N < 2 || N > 63 || B < 1 || n_simd < 1 || !out) return MPCRL_E_ARG;
    if (slice_mode < -1 || slice_mode > 1 || (shape != TUNE_SLICED && shape != TUNE_PLAIN)) return MPCRL_E_ARG;
    const SmallTraits tr = model == MPCRL_MODEL_LINEAR ? small_traits<LinearDev>() : small_traits<CartpoleDev>();
    const SmallPlan p = plan_small(tr, N, B, n_simd, flags, slice_mode, box_rows != 0, linear_spl, shape);
    const int32_t fields[12] = {(int32_t)p.family, p.seg_short, p.box, p.lds_park, p.warm, p.lq_spl, p.lq_rl, (int32_t)p.grid, (int32_t)p.sens_grid,
                                p.candidate, p.by_rule, 0};
    std::memcpy(out, fields, sizeof(fields));
    return 0;
}

int mpcrl_create(const MpcrlProblemSpec *spec, int batch, int device, mpcrl_handle *out) {
    if (!spec || !out || batch <= 0) return MPCRL_E_ARG;
    ON_DEVICE(device);
    MpcrlSolver *h = new (std::nothrow) MpcrlSolver();
    if (!h) return MPCRL_E_NOMEM;
    h->model = spec->model, h->B = batch, h->device = device, h->nx = spec->nx, h->nu = spec->nu, h->np = spec->np, h->N = spec->N;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_simd = 4 * cus;
        const char *e = std::getenv("MPCRL_TIME_SLICE");   // tests, profiling: same as mpcrl_set_launch_mode
        if (e && *e) h->slice_mode = (*e == '0') ? -1 : 1;
        const char *l = std::getenv("MPCRL_LINEAR_SPL");   // stages per lane of the linear-system solve kernel: 3 (default) or 1
        if (l && *l == '1') h->linear_spl = 1;
        const char *g = std::getenv("MPCRL_GENERIC_ROWS");   // tests, A/B runs: the generic cartpole solve kernels whatever the bounds are
        if (g && *g == '1') h->generic_rows = true;
    }
    int rc = 0;
    switch (spec->model) {
        case MPCRL_MODEL_CARTPOLE:
            if (spec->nx != CartpoleDev::NX || spec->nu != CartpoleDev::NU || spec->np != CartpoleDev::NP) rc = MPCRL_E_MODEL;
            break;
        case MPCRL_MODEL_LINEAR:
            if (spec->nx != LinearDev::NX || spec->nu != LinearDev::NU || spec->np != LinearDev::NP) rc = MPCRL_E_MODEL;
            break;
        case MPCRL_MODEL_CHAIN:
            h->is_large = true;
            h->n_mass = (spec->nx / 3 - 1) / 2 + 2;
            if (spec->nu != 3 || h->n_mass < 3 || h->n_mass > 7 || spec->nx != (2 * (h->n_mass - 2) + 1) * 3 || spec->n_consts != spec->nx)
                rc = MPCRL_E_MODEL;
            else if (spec->np != chain_entry(h->n_mass)->np)
                rc = MPCRL_E_MODEL;
            else if (spec->N >= 1 && spec->N < 64 && !chain_entry(h->n_mass)->fits(spec->N))
                rc = MPCRL_E_ARG;   // the horizon's trajectories / tables do not fit the LDS of one workgroup at this chain size
            break;
        default: rc = MPCRL_E_MODEL;
    }
    if (!rc) rc = h->is_large ? fill_large_spec(*spec, h->large) : fill_small_spec(*spec, h->small);
    if (!rc && !h->is_large)   // L1-soft bounds only where the model's kernel carries slack state (models_dev.hpp soft_coord)
        for (int i = 0; i < spec->nx + spec->nu; ++i)
            if (h->small.soft[i] && !(spec->model == MPCRL_MODEL_LINEAR ? LinearDev::soft_coord(i) : CartpoleDev::soft_coord(i))) rc = MPCRL_E_MODEL;
    if (rc) {
        delete h;
        return rc;
    }
    refresh_box_rows(h);
    const size_t B = batch, N = spec->N, nx = spec->nx, nu = spec->nu, nw = nx + nu;
    rc = dev_alloc(&h->X, B * (N + 1) * nx, h->bytes);
    if (!rc) rc = dev_alloc(&h->U, B * N * nu, h->bytes);
    if (!rc) rc = dev_alloc(&h->PI, B * N * nx, h->bytes);
    if (!rc) rc = dev_alloc(&h->BND, B * 10 * (N + 1) * nw, h->bytes);
    if (!rc) rc = dev_alloc(&h->RES, B * 4, h->bytes);
    if (!rc) rc = dev_alloc(&h->LAG, B, h->bytes);
    if (!rc) rc = dev_alloc(&h->theta, B * (size_t)spec->np, h->bytes);
    if (!rc) rc = dev_alloc(&h->perm, B, h->bytes);
    if (!rc) rc = dev_alloc(&h->cold_mask, B, h->bytes);
    if (!rc) rc = dev_alloc(&h->order_state, 4, h->bytes);
    if (!rc && h->is_large) {
        h->ws_stride = chain_entry(h->n_mass)->ws_doubles(spec->N);
        rc = dev_alloc(&h->ws, B * h->ws_stride, h->bytes);
        if (!rc) rc = dev_alloc(&h->consts_dev, (size_t)spec->n_consts, h->bytes);
        if (!rc) {
            if (hipMemcpy(h->consts_dev, spec->consts, spec->n_consts * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = MPCRL_E_HIP;
            h->large.consts = h->consts_dev;
        }
    }
    // parameters 0, residuals 0, and the stored iterate = the cold iterate with x_k = 0: nothing the handle owns is ever read
    // uninitialised (get_iterate / set_iterate before the first solve)
    if (!rc && hipMemset(h->theta, 0, B * (size_t)spec->np * sizeof(double)) != hipSuccess) rc = MPCRL_E_HIP;
    if (!rc && hipMemset(h->RES, 0, B * 4 * sizeof(double)) != hipSuccess) rc = MPCRL_E_HIP;
    if (!rc && hipMemset(h->LAG, 0, B * sizeof(double)) != hipSuccess) rc = MPCRL_E_HIP;
    if (!rc) {   // "no spread known": a cheap-form order launch that runs before any refresh (a captured first call that was never
                 // replayed) then finds one crowded bucket = the identity order, never garbage
        const double os0[4] = {-1.0, 0.0, 0.0, 0.0};
        if (hipMemcpy(h->order_state, os0, sizeof(os0), hipMemcpyHostToDevice) != hipSuccess) rc = MPCRL_E_HIP;
    }
    if (!rc) rc = fill_cold_iterate(h, nullptr, true, nullptr);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = MPCRL_E_HIP;
    if (rc) {
        mpcrl_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int mpcrl_destroy(mpcrl_handle h) {
    if (!h) return MPCRL_E_ARG;
    DeviceGuard guard_(h->device);
    for (double *p : {h->X, h->U, h->PI, h->BND, h->RES, h->LAG, h->theta, h->ws, h->consts_dev})
        if (p) (void)hipFree(p);
    if (h->perm) (void)hipFree(h->perm);
    if (h->cold_mask) (void)hipFree(h->cold_mask);
    if (h->order_state) (void)hipFree(h->order_state);
    for (auto &t : h->tune)
        for (auto &pair : t.ev)
            for (auto &e : pair)
                if (e) (void)hipEventDestroy(e);
    delete h;
    return 0;
}

int64_t mpcrl_workspace_bytes(mpcrl_handle h) { return h ? h->bytes : 0; }

int mpcrl_set_theta(mpcrl_handle h, const double *theta, int n_theta, int per_instance, void *stream) {
    if (!h || !theta || n_theta != h->np) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    const size_t n = (size_t)h->np * (per_instance ? h->B : 1);
    HIP_OK(hipMemcpyAsync(h->theta, theta, n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->chain_ws_current = h->chain_adjoint_current = false;   // (mpcrl_chain_ext.h: the workspace no longer describes the handle's state)
    h->theta_stride = per_instance ? h->np : 0;
    return 0;
}

int mpcrl_set_gamma(mpcrl_handle h, double gamma) {
    if (!h) return MPCRL_E_ARG;
    h->chain_ws_current = h->chain_adjoint_current = false;   // (mpcrl_chain_ext.h: the workspace no longer describes the handle's state)
    h->small.gamma = gamma, h->large.gamma = gamma;
    return 0;
}

int mpcrl_set_options(mpcrl_handle h, double tol, int max_iter) {
    if (!h) return MPCRL_E_ARG;
    if (tol > 0) h->small.tol = tol, h->large.tol = tol;
    if (max_iter >= 0) h->small.max_iter = max_iter, h->large.max_iter = max_iter;
    return 0;
}

int mpcrl_set_exit_rule(mpcrl_handle h, int window, double factor) {
    if (!h || window < 0 || window > 255 || !(factor > 0.0 && factor <= 1.0)) return MPCRL_E_ARG;
    h->small.exit_window = window, h->small.exit_factor = factor;
    h->large.exit_window = window, h->large.exit_factor = factor;
    return 0;
}

int mpcrl_set_order(mpcrl_handle h, const int32_t *perm, void *stream) {
    if (!h) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    if (perm) HIP_OK(hipMemcpyAsync(h->perm, perm, (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->have_perm = perm != nullptr;
    return 0;
}

int mpcrl_set_cold_mask(mpcrl_handle h, const int32_t *mask, void *stream) {
    if (!h) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    if (mask) HIP_OK(hipMemcpyAsync(h->cold_mask, mask, (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->have_cold_mask = mask != nullptr;
    return 0;
}

int mpcrl_query_time_sliced(mpcrl_handle h, int flags, void *stream) {
    if (!h) return MPCRL_E_ARG;
    if (h->is_large) return 0;
    ON_DEVICE(h->device);
    if (!h->have_iterate) flags |= MPCRL_COLD;
    // the plan the next mpcrl_solve computes (launch_small), from the same function; where the tuner has a say, that solve keeps the promise
    return choose_shape(h, flags, (hipStream_t)stream, false).family == SmallPlan::SLICED ? 1 : 0;
}

int mpcrl_set_launch_mode(mpcrl_handle h, int mode) {
    if (!h || mode < -1 || mode > 1) return MPCRL_E_ARG;
    h->slice_mode = mode, h->planned = -1;
    return 0;
}

int mpcrl_get_launch_times(mpcrl_handle h, int warm, double *sliced_ms, double *plain_ms) {
    if (!h || !sliced_ms || !plain_ms) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    MpcrlSolver::Tuner &t = h->tune[warm ? 1 : 0];
    tuner_harvest(t);
    *sliced_ms = t.ms[TUNE_SLICED], *plain_ms = t.ms[TUNE_PLAIN];
    return tuned_best(t);
}

int mpcrl_auto_order(mpcrl_handle h, const double *x0, void *stream) {
    if (!h || !x0) return MPCRL_E_ARG;
    if (h->B > ORDER_MAX) return MPCRL_E_ARG;   // larger batches: build the permutation outside and pass it to mpcrl_set_order
    if (h->is_large || 64 / (h->N + 1) < 2) {   // one instance per wavefront (chain; N + 1 > 32 stages): nothing shares a lock step
        h->have_perm = false;
        return 0;
    }
    ON_DEVICE(h->device);
    // the coordinate and range the batch is bucketed along are found from scratch on the first call and every 32nd one (never inside a
    // stream capture once they exist: a graph replays the cheap form)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    // (a first call inside a capture refreshes as well — the graph then always does — but does not count: the state is only known to
    // be valid once a refresh launch was issued for real)
    const int refresh = (h->order_calls == 0 || (!capturing && h->order_calls % 32 == 0)) ? 1 : 0;
    if (!(capturing && h->order_calls == 0)) h->order_calls++;
    hipLaunchKernelGGL(order_kernel, dim3(1), dim3(ORDER_NT), 0, (hipStream_t)stream, x0, h->B, h->nx, h->perm, h->order_state, refresh);
    HIP_OK(hipGetLastError());
    h->have_perm = true;
    return 0;
}

int mpcrl_debug_get_order(mpcrl_handle h, int32_t *perm_out, double *state_out, void *stream) {
    if (!h) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    const hipStream_t st = (hipStream_t)stream;
    if (perm_out && h->have_perm) HIP_OK(hipMemcpyAsync(perm_out, h->perm, (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (state_out) HIP_OK(hipMemcpyAsync(state_out, h->order_state, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return h->have_perm ? 1 : 0;
}

int mpcrl_set_bounds(mpcrl_handle h, int which, const double *lb, const double *ub) {
    if (!h || !lb || !ub || which < MPCRL_BOUNDS_U0 || which > MPCRL_BOUNDS_TERMINAL) return MPCRL_E_ARG;
    const int nw = h->nx + h->nu;
    const int n = which == MPCRL_BOUNDS_U0 ? h->nu : (which == MPCRL_BOUNDS_STAGE ? nw : h->nx);
    for (int i = 0; i < n; ++i)
        if (!(lb[i] <= ub[i])) return MPCRL_E_ARG;
    double *dl, *du;
    if (h->is_large)
        dl = which == MPCRL_BOUNDS_U0 ? h->large.lb0 : (which == MPCRL_BOUNDS_STAGE ? h->large.lb : h->large.lbe),
        du = which == MPCRL_BOUNDS_U0 ? h->large.ub0 : (which == MPCRL_BOUNDS_STAGE ? h->large.ub : h->large.ube);
    else
        dl = which == MPCRL_BOUNDS_U0 ? h->small.lb0 : (which == MPCRL_BOUNDS_STAGE ? h->small.lb : h->small.lbe),
        du = which == MPCRL_BOUNDS_U0 ? h->small.ub0 : (which == MPCRL_BOUNDS_STAGE ? h->small.ub : h->small.ube);
    if (which == MPCRL_BOUNDS_STAGE && !h->is_large)   // a soft bound must stay a two-sided bound (its slack rows exist for both sides)
        for (int i = 0; i < n; ++i)
            if (h->small.soft[i] && (lb[i] <= -MPCRL_NO_BOUND * 0.1 || ub[i] >= MPCRL_NO_BOUND * 0.1)) return MPCRL_E_ARG;
    h->chain_ws_current = h->chain_adjoint_current = false;   // (mpcrl_chain_ext.h: the workspace no longer describes the handle's state)
    for (int i = 0; i < n; ++i) dl[i] = lb[i], du[i] = ub[i];
    refresh_box_rows(h);
    return 0;
}

int mpcrl_query_box_rows(mpcrl_handle h) {
    if (!h) return MPCRL_E_ARG;
    return h->box_rows ? 1 : 0;
}

int mpcrl_reset(mpcrl_handle h, const double *x0, void *stream) {
    if (!h) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    // the next solve builds the cold iterate itself from ITS x0 (MPCRL_COLD); the stored arrays are set to the same state so
    // that get_iterate / set_iterate after a reset see the cold iterate and not the previous solution
    int rc = fill_cold_iterate(h, x0, true, (hipStream_t)stream);
    h->chain_ws_current = h->chain_adjoint_current = false;   // (mpcrl_chain_ext.h: the workspace no longer describes the handle's state)
    h->have_iterate = false, h->dual_cold = false;
    return rc;
}

int mpcrl_solve(mpcrl_handle h, const double *x0, const double *u0_fixed, int flags, double *u0_out, double *V, double *dV_dp,
                double *dpi_dp, int32_t *status, int32_t *iters, void *stream) {
    if (!h || !x0 || !u0_out || !V || !status) return MPCRL_E_ARG;
    if ((flags & MPCRL_SENS_V) && !dV_dp) return MPCRL_E_ARG;
    if ((flags & MPCRL_SENS_PI) && !dpi_dp) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    // (test-only flag: cartpole through its own kernel instantiation, chain and lq_solve_kernel through a wave-uniform switch; not for RTI calls,
    // not for the one-stage linear kernels)
    if ((flags & MPCRL_EXACT_QP) && ((flags & MPCRL_RTI) || (h->model == MPCRL_MODEL_LINEAR && h->linear_spl == 1))) return MPCRL_E_ARG;
    if (!h->have_iterate) flags |= MPCRL_COLD;
    if (h->dual_cold) flags |= MPCRL_COLD_DUAL;
    SmallArgs a;
    a.B = h->B, a.flags = flags, a.theta_stride = h->theta_stride, a.perm = h->have_perm ? h->perm : nullptr;
    a.cold = (h->have_cold_mask && h->have_iterate) ? h->cold_mask : nullptr;   // one-shot: consumed by this solve
    h->have_cold_mask = false;
    a.x0 = x0, a.u0fix = u0_fixed, a.theta = h->theta;
    a.X = h->X, a.U = h->U, a.PI = h->PI, a.BND = h->BND, a.RES = h->RES, a.LAG = h->LAG;
    a.u0_out = u0_out, a.V = V, a.dV = (flags & MPCRL_SENS_V) ? dV_dp : nullptr, a.dpi = (flags & MPCRL_SENS_PI) ? dpi_dp : nullptr;
    a.status = status, a.iters = iters;
    // chain: sens_out stores only the entries of solved instances that have a gradient; the small models' sensitivity kernel writes its rows in full
    if (h->is_large && a.dV) HIP_OK(hipMemsetAsync(dV_dp, 0, (size_t)h->B * h->np * sizeof(double), st));
    if (h->is_large && a.dpi) HIP_OK(hipMemsetAsync(dpi_dp, 0, (size_t)h->B * h->nu * h->np * sizeof(double), st));
    int rc;
    if (h->is_large) {
        LargeArgs la;
        la.B = a.B, la.flags = a.flags, la.theta_stride = a.theta_stride, la.perm = a.perm, la.cold = a.cold, la.x0 = a.x0, la.u0fix = a.u0fix, la.theta = a.theta;
        la.X = a.X, la.U = a.U, la.PI = a.PI, la.BND = a.BND, la.RES = a.RES, la.LAG = a.LAG, la.ws = nullptr, la.ws_stride = 0;
        la.u0_out = a.u0_out, la.V = a.V, la.dV = a.dV, la.dpi = a.dpi, la.status = a.status, la.iters = a.iters;
        rc = chain_entry(h->n_mass)->launch(h, la, st);
    } else
        rc = launch_small(h, a, st);   // (mpcrl_create admits no other model: cartpole or the linear system)
    // (a solve that left the bound planes alone: the next one must not start its interior point from them)
    if (!rc) h->have_iterate = true, h->dual_cold = (flags & MPCRL_NO_BND_STORE) != 0;
    if (!rc && h->is_large) h->chain_ws_current = true, h->chain_adjoint_current = a.dpi && !a.u0fix;
    return rc;
}

int mpcrl_get_iterate(mpcrl_handle h, double *x, double *u, double *pi, double *bnd, double *res, void *stream) {
    if (!h) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = h->B, N = h->N, nx = h->nx, nu = h->nu, nw = nx + nu;
    if (x) HIP_OK(hipMemcpyAsync(x, h->X, B * (N + 1) * nx * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (u) HIP_OK(hipMemcpyAsync(u, h->U, B * N * nu * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (pi) HIP_OK(hipMemcpyAsync(pi, h->PI, B * N * nx * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (bnd) HIP_OK(hipMemcpyAsync(bnd, h->BND, B * 10 * (N + 1) * nw * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (res) HIP_OK(hipMemcpyAsync(res, h->RES, B * 4 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}

int mpcrl_get_lagrangian(mpcrl_handle h, double *L, void *stream) {
    if (!h || !L) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    HIP_OK(hipMemcpyAsync(L, h->LAG, (size_t)h->B * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int mpcrl_set_iterate(mpcrl_handle h, const double *x, const double *u, const double *pi, const double *bnd, void *stream) {
    if (!h || !x || !u || !pi) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = h->B, N = h->N, nx = h->nx, nu = h->nu, nw = nx + nu;
    HIP_OK(hipMemcpyAsync(h->X, x, B * (N + 1) * nx * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(h->U, u, B * N * nu * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(h->PI, pi, B * N * nx * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (bnd)
        HIP_OK(hipMemcpyAsync(h->BND, bnd, B * 10 * (N + 1) * nw * sizeof(double), hipMemcpyDeviceToDevice, st));
    else {   // multipliers 0, slacks t = 1: the state MPCRL_COLD would build
        int rc = fill_cold_iterate(h, nullptr, false, st);
        if (rc) return rc;
    }
    h->chain_ws_current = h->chain_adjoint_current = false;   // (mpcrl_chain_ext.h: the workspace no longer describes the handle's state)
    h->have_iterate = true, h->dual_cold = bnd == nullptr;
    return 0;
}

int mpcrl_get_iterate_rows(mpcrl_handle h, double *x, double *u, double *pi, double *bnd, const int64_t *index, void *stream) {
    if (!h || !(x || u || pi || bnd)) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    const int N = h->N, nx = h->nx, nu = h->nu, nw = nx + nu;
    hipLaunchKernelGGL(iterate_rows_kernel<false>, dim3((unsigned)h->B), dim3(256), 0, (hipStream_t)stream, h->X, h->U, h->PI, h->BND, x, u, pi, bnd,
                       (const long *)index, (N + 1) * nx, N * nu, N * nx, 10 * (N + 1) * nw);
    HIP_OK(hipGetLastError());
    return 0;
}

int mpcrl_set_iterate_rows(mpcrl_handle h, const double *x, const double *u, const double *pi, const double *bnd, const int64_t *index, void *stream) {
    if (!h || !x || !u || !pi) return MPCRL_E_ARG;
    ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int N = h->N, nx = h->nx, nu = h->nu, nw = nx + nu;
    if (!bnd) {   // multipliers 0, slacks t = 1: the state MPCRL_COLD would build
        int rc = fill_cold_iterate(h, nullptr, false, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(iterate_rows_kernel<true>, dim3((unsigned)h->B), dim3(256), 0, st, h->X, h->U, h->PI, h->BND, (double *)x, (double *)u, (double *)pi,
                       (double *)bnd, (const long *)index, (N + 1) * nx, N * nu, N * nx, 10 * (N + 1) * nw);
    HIP_OK(hipGetLastError());
    h->chain_ws_current = h->chain_adjoint_current = false;   // (mpcrl_chain_ext.h: the workspace no longer describes the handle's state)
    h->have_iterate = true, h->dual_cold = bnd == nullptr;
    return 0;
}

}  // extern "C"
