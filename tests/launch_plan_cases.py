"""The launch plan of the cartpole / linear-system solves (csrc/launch_plan.hpp, plan_small) restated in Python, independently of the
header: which kernel family one mpcrl_solve launches, with which template switches and in which grids.  `expected` returns the twelve
numbers mpcrl_debug_launch_plan writes (include/mpcrl.h states the order); tests/test_launch_plan_cpu.py sweeps the two against each
other and pins the cases below by literal, tests/test_gpu_small_modes.py holds mpcrl_query_time_sliced of real handles to it.

The rules, as the kernels' lane layouts state them (one lane per stage, lpi = N + 1 lanes per instance, 64 lanes per wavefront):
  * plain kernel: min(64 // lpi, MAX_IPW) instances per wavefront (cartpole MAX_IPW 4, linear system 21), one workgroup per wavefront;
  * time-sliced kernel (models without soft bounds: cartpole): q = min(64 // lpi, MAX_IPW - 1) + 1 instances per wavefront, one of
    them parked; legal when at least one lane is left beside the resident slots and the call is not an RTI call; favoured by the
    wave-count rule when 1.62 x (rounds of q-instance wavefronts on the SIMDs) <= rounds of plain wavefronts; forced modes override
    the rule, never the legality; in automatic mode the tuner's shape decides among the favoured;
  * the parked instance takes 2 nx + nu + 4 (nx + nu) doubles per stage and lives in LDS up to 21 stages (cartpole);
  * SHORT reductions for lpi <= 32 unless the model skips tree levels at run time (linear system);
  * BOX rows: cartpole, when the handle's bounds are the full-box pattern; not for the exact-QP instantiation;
  * linear system: lq_solve_kernel with 3 stages per lane in rows of 8 (16) lanes, 4 stages per lane beyond 16 lanes, when that packs
    more instances into a wavefront than one stage per lane and MPCRL_LINEAR_SPL is not 1; it runs its own sensitivity pass;
  * MPCRL_EXACT_QP on cartpole: the exact-QP instantiation in the plain grid, then the shipped sensitivity pass."""
import itertools

SENS_V, SENS_PI, RTI, COLD, EXACT_QP = 1, 2, 4, 8, 64
PLAIN, SLICED, LQ, EXACT = 0, 1, 2, 3
TUNE_SLICED, TUNE_PLAIN = 0, 1
FIELDS = ("family", "seg_short", "box", "lds_park", "warm", "lq_spl", "lq_rl", "grid", "sens_grid", "candidate", "by_rule", "reserved")

MODELS = {       # id (MPCRL_MODEL_*), nx, nu, MAX_IPW, soft bounds, run-time level skipping
    "cartpole": dict(id=0, nx=4, nu=1, max_ipw=4, soft=False, skip=False),
    "linear": dict(id=1, nx=2, nu=1, max_ipw=21, soft=True, skip=True),
}
LDS_PARK_STAGES = {"cartpole": 21, "linear": 64}

# the sweep of the issue
SWEEP_N = range(2, 64)
SWEEP_B = (1, 3, 4, 96, 4096, 4097, 32768)
SWEEP_SIMD = (1024, 1)
SWEEP_FLAGS = [sum(s) for k in range(5) for s in itertools.combinations((COLD, RTI, SENS_PI, EXACT_QP), k)]
SWEEP_MODE = (-1, 0, 1)


def ceil_div(a, b):
    return -(-a // b)


def expected(model, N, B, n_simd, flags, slice_mode, box_rows, linear_spl, shape):
    m = MODELS[model]
    lpi = N + 1
    per_wave = min(64 // lpi, m["max_ipw"])
    plain_grid = ceil_div(B, per_wave)
    wants_sens = bool(flags & (SENS_V | SENS_PI))
    exact = model == "cartpole" and bool(flags & EXACT_QP)
    out = dict.fromkeys(FIELDS, 0)
    out["seg_short"] = int(lpi <= 32 and not m["skip"])
    out["warm"] = int(not flags & COLD)
    # --- may the launch be time-sliced, and does the wave count favour it
    if not m["soft"] and not exact:
        resident = min(64 // lpi, m["max_ipw"] - 1)
        sliced_grid = ceil_div(B, resident + 1)
        out["candidate"] = int(resident >= 1 and resident * lpi < 64 and not flags & RTI)
        out["by_rule"] = int(162 * ceil_div(sliced_grid, n_simd) <= 100 * ceil_div(plain_grid, n_simd))      # (1.62, in integers)
    if exact:
        family, grid = EXACT, plain_grid
    elif out["candidate"] and (slice_mode == 1 or (slice_mode == 0 and out["by_rule"] and shape == TUNE_SLICED)):
        family, grid = SLICED, sliced_grid
        out["lds_park"] = int(lpi <= LDS_PARK_STAGES[model])
    else:
        family, grid = PLAIN, plain_grid
        if model == "linear" and linear_spl != 1:
            lanes3 = ceil_div(lpi, 3)
            row = 8 if lanes3 <= 8 else 16
            if 64 // row > per_wave:
                family, grid = LQ, ceil_div(B, 64 // row)
                out["lq_spl"], out["lq_rl"] = (4 if lanes3 > 16 else 3), row
    out["family"], out["grid"] = family, grid
    out["box"] = int(model == "cartpole" and bool(box_rows) and family in (PLAIN, SLICED))
    out["sens_grid"] = plain_grid if wants_sens and family != LQ else 0
    return [out[f] for f in FIELDS]


def tuner(calls, ms_sliced, ms_plain):
    """(shape of call number `calls`, whether it is a timed probe, the shape the times prefer): calls 1 and 2 of every 64 probe the
    time-sliced and the plain shape; plain is preferred only when both are timed and plain < 0.80 x time-sliced."""
    best = TUNE_PLAIN if (ms_sliced > 0 and ms_plain > 0 and ms_plain < 0.80 * ms_sliced) else TUNE_SLICED
    phase = calls % 64
    return {1: TUNE_SLICED, 2: TUNE_PLAIN}.get(phase, best), int(phase in (1, 2)), best
