"""What tests/test_small_modes_cpu.py and tests/test_gpu_small_modes.py share (no test of its own): the inputs of the cartpole and
linear-system kernels at every horizon where their lane layout or their kernel changes, the references of the C++ CPU port (oracle/cpu)
on those inputs, computed once per (model, N), and the comparison helpers (used by tests/test_gpu_chain_modes.py as well).

Lane layouts (csrc/launch_plan.hpp: plan_small, sliced_parks_in_lds):
  cartpole   min(64 / (N + 1), 4) instances per wavefront: 4 up to N = 15, 3 up to N = 20, 2 up to N = 31, 1 from N = 32.  The
             time-sliced launch holds one instance fewer per round (at most 3) plus a parked one, in LDS up to N = 20 and in HBM from
             N = 21; it needs a spare lane, so it is illegal at N = 31 (two 32-lane slots) and N = 63 (64 stages).
  linear     one stage per lane up to N = 7 (small_solve_kernel, 64 / (N + 1) instances per wavefront); lq_solve_kernel<3, 8> for
             N = 8 .. 23 (8 instances), <3, 16> for N = 24 .. 47 (4 instances), <4, 16> for N = 48 .. 63 (4 instances).

Comparison rule (the project's own): statuses equal the port's, SQP iteration counts within one, the largest error over u0, V, dV, dpi,
X, U, PI (every instance's row scaled by max(|reference row|, 1)) below RTOL = 1e-6, the bar of BASELINE.json.  On the lq_solve_kernel
horizons an instance whose interior-point count differs from the port's by one stopped one iteration apart and shares only the QP
tolerance with it: 1e-4, and 1e-3 for dpi (the bars of test_linear_kernel_three_stages_per_lane_vs_one); at most one instance of a
case may need them."""
import dataclasses
import functools

import numpy as np
import torch

RTOL = 1e-6
LOOSE, LOOSE_DPI = 1e-4, 1e-3
FIELDS = ("u0", "V", "dV", "dpi", "X", "U", "PI")
Q_FIELDS = ("V", "dV", "X", "U", "PI")      # Q mode: u0 and dpi are checked exactly (the pinned value, zeros)

CP_B, LIN_B = 13, 25
CP_N = (2, 3, 15, 16, 20, 21, 31, 32, 62, 63)
LIN_N = (2, 7, 8, 9, 22, 23, 24, 47, 48, 63)
CP_WARM_N, LIN_WARM_N = (3, 16, 21, 32, 63), (7, 8, 24, 48)
CP_BOUNDS_N, LIN_BOUNDS_N = (3, 21, 32, 63), (7, 8, 24, 48)
CP_MAXITER_N = (16, 32, 63)
LIN_GAMMA_N = (8, 24)
CP_TOL_N, LIN_TOL_N = 32, 24
CP_NAN_N, LIN_NAN_N = (3, 16, 21), (2, 8, 24, 48)
CP_U_BOUND, LIN_U_BOUND = 20.0, 0.5
LIN_STAGE_LB, LIN_TERMINAL_LB = -0.3, -0.05
ACTIVE = 1e-3      # a bound row counts as active when its multiplier is above this


# ---------------------------------------------------------------------------------------------------------------------------------
# device side and comparison (moved here from tests/test_gpu_chain_modes.py and tests/test_gpu_small_modes.py, which import them back)
# ---------------------------------------------------------------------------------------------------------------------------------
def raw_solve(mpc, x0, u0=None, flags=None):
    """mpcrl_solve through ctypes with every output buffer poisoned (NaN / -1) before the call, as
    test_sensitivity_rows_are_written_in_full calls it: what comes back was written by this call."""
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import SolveResult, _ptr
    B = mpc.B
    flags = (_lib.SENS_V | _lib.SENS_PI | _lib.COLD) if flags is None else flags
    kw = dict(dtype=torch.float64, device=mpc.device)
    xd = torch.as_tensor(x0, **kw).reshape(B, mpc.nx).contiguous()
    ud = None if u0 is None else torch.as_tensor(u0, **kw).reshape(B, mpc.nu).contiguous()
    u0o, V = torch.full((B, mpc.nu), np.nan, **kw), torch.full((B,), np.nan, **kw)
    dV, dpi = torch.full((B, mpc.n_p), np.nan, **kw), torch.full((B, mpc.nu, mpc.n_p), np.nan, **kw)
    st = torch.full((B,), -1, dtype=torch.int32, device=mpc.device)
    it = torch.full((B, 2), -1, dtype=torch.int32, device=mpc.device)
    with torch.cuda.device(mpc.device):
        rc = mpc.lib.mpcrl_solve(mpc._h, _ptr(xd), _ptr(ud), flags, _ptr(u0o), _ptr(V), _ptr(dV), _ptr(dpi), _ptr(st), _ptr(it), mpc._stream())
    torch.cuda.synchronize()
    assert rc == 0
    mpc.has_iterate = mpc.duals_valid = True
    return SolveResult(u0o, V, st, it, dV, dpi)


def outputs(mpc, r):
    """What a call returned and left behind, as numpy arrays under the names of the port's result."""
    x, u, pi, bnd, _ = mpc.get_iterate()
    o = {"status": r.status, "iters": r.iters, "u0": r.u0, "V": r.V, "dV": r.dV_dp, "dpi": r.dpi_dp, "X": x, "U": u, "PI": pi, "BND": bnd}
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def row_errors(got, ref, fields=FIELDS, rows=None):
    """{field: |got - ref| of every compared instance, its row scaled by max(|reference row|, 1)} (a NaN on the device side is inf).
    ref: a PortResult (or a dict of arrays under the same names); rows: the instances to compare (default: all of them)."""
    per = {}
    for f in fields:
        a = got[f]
        b = ref[f] if isinstance(ref, dict) else {"u0": ref.u0, "V": ref.V, "dV": ref.dV, "dpi": ref.dpi, "X": ref.X, "U": ref.U, "PI": ref.PI}[f]
        B = len(b)
        a, b = np.asarray(a, float).reshape(B, -1), np.asarray(b, float).reshape(B, -1)
        if rows is not None:
            a, b = a[rows], b[rows]
        assert a.shape == b.shape and np.all(np.isfinite(b)), f
        if a.shape[1] == 0:
            continue
        e = np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)
        per[f] = np.nan_to_num(e, nan=np.inf)
    return per


def largest_error(got, ref, fields=FIELDS, rows=None):
    """THE comparison: the largest |got - ref| over the named fields, every instance's row scaled by max(|reference row|, 1).
    ref: a PortResult (or a dict of arrays under the same names); rows: the instances to compare (default: all of them)."""
    per = {f: float(e.max()) for f, e in row_errors(got, ref, fields, rows).items()}
    largest_error.last = per
    return max(per.values(), default=0.0)


def same_statuses(got, ref, expect=0):
    """Statuses equal on both sides and, unless the case is about a status, all zero; SQP iteration counts within one."""
    assert np.array_equal(got["status"], ref.status), (got["status"], ref.status)
    if expect is not None:
        assert np.all(ref.status == expect), ref.status
    assert np.abs(got["iters"][:, 0] - ref.sqp_iter).max() <= 1, (got["iters"][:, 0], ref.sqp_iter)


def report(tag, err, suite="chain modes"):
    print(f"[{suite}] {tag}: largest error {err:.3e}  {largest_error.last}")


def bit_equal(ra, rb, rows=None):
    for f in ("u0", "V", "status", "iters", "dV_dp", "dpi_dp"):
        a, b = getattr(ra, f), getattr(rb, f)
        assert (a is None) == (b is None), f
        if a is not None:
            if rows is not None:
                a, b = a[rows], b[rows]
            assert torch.equal(a, b), f


def snapshot(mpc, r):
    """Everything a call returned and left in the handle."""
    return r, mpc.get_iterate(), mpc.get_lagrangian()


def same_bits(a, b, rows=None, reverse=False, lagrangian=True):
    """Two snapshots bit for bit (b in reversed batch order if reverse), on the given instances."""
    from mpc4rl_amd.batch import SolveResult
    (ra, ia, la), (rb, ib, lb) = a, b
    if reverse:
        rb = SolveResult(*[None if t is None else t.flip(0) for t in (rb.u0, rb.V, rb.status, rb.iters, rb.dV_dp, rb.dpi_dp)])
        ib, lb = [t.flip(0) for t in ib], lb.flip(0)
    bit_equal(ra, rb, rows)
    sel = slice(None) if rows is None else rows
    for name, t1, t2 in zip(("x", "u", "pi", "bnd", "res"), ia, ib):
        assert torch.equal(t1[sel], t2[sel]), name
    if lagrangian:
        assert torch.equal(la[sel], lb[sel]), "lagrangian"


def uses_lq_kernel(model, N):
    """launch_small's choice for the linear system: lq_solve_kernel from N = 8 (more instances per wavefront than one stage per lane)."""
    return model == "linear" and N >= 8


def compare(got, ref, lq, fields=FIELDS, tag="", suite="small modes"):
    """The comparison rule of the module's docstring.  Returns (largest error at the RTOL bar, instances that needed the looser bars);
    asserts everything but the statuses (same_statuses)."""
    per = row_errors(got, ref, fields)
    worst = np.max([per[f] for f in per], axis=0)
    loose = np.zeros(len(worst), bool)
    if lq:
        one_apart = np.abs(got["iters"][:, 1] - ref.ipm_iter) == 1
        loose = one_apart & (worst >= RTOL)
        for f in per:
            assert np.all(per[f][loose] < (LOOSE_DPI if f == "dpi" else LOOSE)), (tag, f, per[f])
    err = float(worst[~loose].max())
    largest_error.last = {f: float(e[~loose].max()) for f, e in per.items()}
    print(f"[{suite}] {tag}: largest error {err:.3e}  {largest_error.last}  looser bar on {int(loose.sum())} instances")
    assert err < RTOL, (tag, largest_error.last)
    assert loose.sum() <= 1, (tag, np.flatnonzero(loose))
    compare.loose_total += int(loose.sum())
    return err, int(loose.sum())


compare.loose_total = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU only; computed once per (model, N) and shared, never written to)
# ---------------------------------------------------------------------------------------------------------------------------------
def problem(model, N, gamma=0.99):
    """(the library's description, the port's) of one model at horizon N."""
    from mpc4rl_amd import cartpole_ocp, linear_system_ocp
    from oracle.problems import make_cartpole, make_linear_system
    if model == "cartpole":
        return cartpole_ocp(N=N, tf=0.1 * N), make_cartpole(N=N, tf=0.1 * N)
    return linear_system_ocp(discount_factor=gamma, N=N), make_linear_system(gamma=gamma, N=N)


@functools.lru_cache(maxsize=None)
def inputs(model):
    """(x0 [B, nx], the pinned u0 of the Q-mode calls before row 0 is replaced [B, 1], the step to the warm calls' x1 [B, nx])."""
    rng = np.random.default_rng(41)
    if model == "cartpole":
        x0 = rng.uniform(-1, 1, (CP_B, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
        u0 = rng.uniform(-15, 15, (CP_B, 1))
    else:
        x0 = np.column_stack([rng.uniform(0.15, 0.85, LIN_B), rng.uniform(-0.2, 0.5, LIN_B)])
        u0 = rng.uniform(-0.9, 0.9, (LIN_B, 1))
    step = rng.normal(0.0, 0.02, x0.shape)
    return x0, u0, step


@dataclasses.dataclass
class Case:
    model: str
    N: int
    ocp: object
    P: object
    x0: np.ndarray
    u0: np.ndarray          # pinned u_0 of the Q-mode calls; row 0 = that instance's own V-mode u0*
    ref_v: object           # port, V mode, cold
    ref_q: object           # port, Q mode, cold
    lq: bool                # the device runs lq_solve_kernel at this horizon

    @property
    def B(self):
        return len(self.x0)


@functools.lru_cache(maxsize=None)
def case(port, model, N):
    ocp, P = problem(model, N)
    x0, u0, _ = inputs(model)
    ref_v = port.solve(P, x0)
    u0 = u0.copy()
    u0[0] = ref_v.u0[0]
    return Case(model, N, ocp, P, x0, u0, ref_v, port.solve(P, x0, u0fix=u0), uses_lq_kernel(model, N))


@dataclasses.dataclass
class WarmCase:
    x1: np.ndarray
    ref_w: object           # port, V mode at x1, warm from Case.ref_v
    ref_wq: object          # port, Q mode at x1, warm from ref_w
    ref_wv: object          # port, V mode at x1, warm from ref_wq
    ref_cold: object        # port, V mode at x1, cold


@functools.lru_cache(maxsize=None)
def warm_case(port, model, N):
    c = case(port, model, N)
    x1 = c.x0 + inputs(model)[2]
    ref_w = port.solve(c.P, x1, warm=c.ref_v)
    ref_wq = port.solve(c.P, x1, u0fix=c.u0, warm=ref_w)
    return WarmCase(x1, ref_w, ref_wq, port.solve(c.P, x1, warm=ref_wq), port.solve(c.P, x1))


@dataclasses.dataclass
class BoundsCase:
    lb0: np.ndarray         # what mpcrl_set_bounds takes: BOUNDS_U0
    ub0: np.ndarray
    lb: np.ndarray          # BOUNDS_STAGE, v = [u; x]
    ub: np.ndarray
    lbe: np.ndarray         # BOUNDS_TERMINAL
    ube: np.ndarray
    P: object               # the port's problem with those bounds from the start
    ref: object             # port, V mode, cold, on P
    b0: float               # the level of the BOUNDS_U0-only call: half the free solution's largest |u_k|, k >= 1


def original_bounds(ocp):
    """(lb0, ub0, lb, ub, lbe, ube) a handle is created with."""
    lb, ub, lbe, ube, _, _, _ = ocp.stage_bounds()
    return lb[: ocp.nu].copy(), ub[: ocp.nu].copy(), lb, ub, lbe, ube


def cartpole_velocity_level(c):
    """Halfway between -max |x0[:, 1]| and the median over instances of the free solution's smallest cart velocity (stages 1 .. N)."""
    return 0.5 * (-np.abs(c.x0[:, 1]).max() + np.median(c.ref_v.X[:, 1:, 1].min(1)))


@functools.lru_cache(maxsize=None)
def bounds_case(port, model, N):
    """The bounds of the issue's section 3.  Cartpole: controls +-20; the cart velocity (state 1) bounded from below only, on the
    stages and at the terminal stage.  Linear: controls +-0.5; x[1] >= -0.3 (no upper bound) on the stages, x_N[1] >= -0.05, the soft
    row x[0] in [0, 1] as it is."""
    c = case(port, model, N)
    nu = c.ocp.nu
    _, _, lb, ub, lbe, ube = [a.copy() for a in original_bounds(c.ocp)]
    if model == "cartpole":
        bu, lvl = CP_U_BOUND, cartpole_velocity_level(c)
        lb[nu + 1], ub[nu + 1], lbe[1], ube[1] = lvl, 1e30, lvl, 1e30
        P = dataclasses.replace(c.P, lbu=np.array([-bu]), ubu=np.array([bu]), lbx=lb[nu:].copy(), ubx=ub[nu:].copy(),
                                lbx_e=lbe.copy(), ubx_e=ube.copy())
    else:
        bu = LIN_U_BOUND
        lb[nu + 1], ub[nu + 1], lbe[1], ube[1] = LIN_STAGE_LB, 1e30, LIN_TERMINAL_LB, 1e30
        one = lambda v, dt=float: np.array([v], dt)
        P = dataclasses.replace(c.P, lbu=one(-bu), ubu=one(bu), lbx=lb[nu:].copy(), ubx=ub[nu:].copy(),
                                idxbx_e=one(1, int), lbx_e=one(LIN_TERMINAL_LB), ubx_e=one(1e30))
    lb[:nu], ub[:nu] = -bu, bu
    b0 = 0.5 * float(np.abs(c.ref_v.U[:, 1:]).max())
    return BoundsCase(np.full(nu, -bu), np.full(nu, bu), lb, ub, lbe, ube, P, port.solve(P, c.x0), b0)


def active_rows(BND, N, nu):
    """Per instance, from the bound planes [B, 10, N + 1, nu + nx]: (a control row on its bound, the lower row of state 1 at a stage
    1 .. N - 1, that row at the terminal stage), by the multipliers lam_l (plane 0) and lam_u (plane 1)."""
    lam = np.maximum(BND[:, 0], BND[:, 1])
    control = lam[:, :N, :nu].reshape(len(BND), -1).max(1) > ACTIVE
    stage = BND[:, 0, 1:N, nu + 1].max(1) > ACTIVE
    return control, stage, BND[:, 0, N, nu + 1] > ACTIVE
