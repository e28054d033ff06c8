"""mpcrl_bound_vjp and mpcrl_bound_value_grad (include/mpcrl_bound_ext.h) on the device, cartpole and linear system: the derivatives
of the planned trajectory and of the value with respect to the box bounds from small_bound_vjp_kernel / bound_value_grad_kernel
against the mirror fixture G13 (tests/golden/make_bound_vjp.py), the known answer du_k/db_k = 1 on an active control row, the
calls' contract, the same bits under every launch shape, and MPCLayer with ``bounds`` on top.

Bars.  Against the fixture: max(1e-6, 4 x the error of that solve's own du0*/dp against the fixture's mirror du0*/dp on the same
instances) — another right-hand side of the same factorisation, the bar of tests/test_gpu_traj_vjp.py; 1e-6 is RTOL of
tests/small_mode_cases.py.  A row is an instance's whole [N + 1, nu + nx] gradient, scaled by max(|reference|, 1).  Asserted on the
firm instances (no positive slack: with one the mirror holds the slacks constant and is the definition, not a yardstick); the
instances with an active hard state row are asserted on their own and printed on their own line.  The layer against central
differences of its own forward pass at h = 1e-5: 1e-5, the bar of the existing layer tests.  Q mode against differences of Q at
h = 1e-4 (solves at tol 1e-10: 1e-10 / 1e-4 = 1e-6 of noise at worst, Q itself second order in the residual): 1e-6.

Measured on an MI355X: MEASURED at the end of this file (every line the tests print).
"""
import itertools
import os

import numpy as np
import pytest
import torch

import small_mode_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
RTOL = C.RTOL


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLD, "g13_bound_vjp.npz"))


def scaled(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    if not len(ref):
        return 0.0
    got, ref = got.reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)).max())


def same(a, b):
    """bit-identical, NaN included"""
    return all((x is None and y is None) or torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def set_bounds(mpc, lb0, ub0, lb, ub, lbe, ube):
    from mpc4rl_amd import _lib
    mpc.set_bounds(_lib.BOUNDS_U0, lb0, ub0)
    mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, lbe, ube)


def handle(ocp, B, bounds=None, tol=1e-9):
    from mpc4rl_amd import MPCBatch
    mpc = MPCBatch(ocp, B)
    mpc.set_options(tol=tol)
    if bounds is not None:
        set_bounds(mpc, *bounds)
    return mpc


def fixture_bounds(g13, key):
    return tuple(g13[key + k] for k in ("lb0", "ub0", "lb", "ub", "lbe", "ube"))


def split(mpc, G):
    """(gX [B, N+1, nx], gU [B, N, nu]) of cotangents [B, nw] in the mirror's order w = [u_0 .. u_{N-1}; x_0 .. x_N]."""
    G = torch.as_tensor(G, dtype=torch.float64, device=mpc.device)
    n = mpc.N * mpc.nu
    return G[:, n:].reshape(mpc.B, mpc.N + 1, mpc.nx).contiguous(), G[:, :n].reshape(mpc.B, mpc.N, mpc.nu).contiguous()


def shapes(mpc):
    nb = (mpc.B, mpc.N + 1, mpc.nu + mpc.nx)
    return (mpc.B, mpc.nx), (mpc.B, mpc.n_p), nb, nb


def raw_vjp(mpc, gX, gU, want=(True, True, True, True), flags=0, fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    bufs = [torch.full(sh, fill, **kw) if w else None for sh, w in zip(shapes(mpc), want)]
    mpc._call("mpcrl_bound_vjp", flags, gX, gU, *bufs)
    torch.cuda.synchronize()
    return bufs


def raw_traj_vjp(mpc, gX, gU, want=(True, True)):
    kw = dict(dtype=torch.float64, device=mpc.device)
    bufs = [torch.full(sh, float("nan"), **kw) if w else None for sh, w in zip(shapes(mpc)[:2], want)]
    mpc._call("mpcrl_traj_vjp", 0, gX, gU, *bufs)
    torch.cuda.synchronize()
    return bufs


def raw_value(mpc, want=(True, True), flags=0):
    kw = dict(dtype=torch.float64, device=mpc.device)
    bufs = [torch.full(shapes(mpc)[2], float("nan"), **kw) if w else None for w in want]
    mpc._call("mpcrl_bound_value_grad", flags, *bufs)
    torch.cuda.synchronize()
    return bufs


def row_mask(mpc, bounds):
    """[2, N + 1, nu + nx]: the bound rows the OCP has."""
    lb0, ub0, lb, ub, lbe, ube = (np.asarray(b, float) for b in bounds)
    N, nu = mpc.N, mpc.nu
    m = np.zeros((2, N + 1, mpc.nu + mpc.nx), bool)
    m[0, 0, :nu], m[1, 0, :nu] = lb0 > -1e29, ub0 < 1e29
    m[0, 1:N], m[1, 1:N] = lb > -1e29, ub < 1e29
    m[0, N, nu:], m[1, N, nu:] = lbe > -1e29, ube < 1e29
    return m


# ---------------------------------------------------------------------- 1. against the fixture
def fixture_case(g13, key, ocp, rows):
    """The bounds of the fixture, a cold solve at tol 1e-9 on its x0, one bound_vjp per cotangent and bound_value_grad.  Returns (bar,
    error of the solve's own du0*/dp, errors over the firm instances per cotangent, over those with an active hard state row, of
    dV/db, counts)."""
    x0 = g13[key + "x0"][rows]
    bounds = fixture_bounds(g13, key)
    mpc = handle(ocp, len(x0), bounds)
    r = mpc.solve(x0, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
    firm, act_x = ~g13[key + "soft"][rows], g13[key + "act_x"][rows] & ~g13[key + "soft"][rows]
    ref_dp = g13[key + "dpi_dp"][rows].copy()
    ref_dp[g13[key + "act_u0"][rows]] = 0.0      # u_0 on its bound: the exact zero, as tests/test_gpu_state_sens.py takes it
    err_dp = scaled(r.dpi_dp.cpu().numpy()[firm], ref_dp[firm])
    e_firm, e_x = [], []
    for c in range(3):
        gX, gU = split(mpc, g13[key + "G"][rows][:, c])
        _, _, g_lb, g_ub = mpc.bound_vjp(gX, gU, x0=False, theta=False)
        got = np.stack([g_lb.cpu().numpy(), g_ub.cpu().numpy()], 1)
        ref = np.stack([g13[key + "g_lb"][rows][:, c], g13[key + "g_ub"][rows][:, c]], 1)
        m = row_mask(mpc, bounds)
        assert np.all(got[:, ~m] == 0)                       # the structural zeros are exact
        e_firm.append(scaled(got[firm], ref[firm])), e_x.append(scaled(got[act_x], ref[act_x]))
    dlb, dub = mpc.bound_value_grad()
    bnd = mpc.get_iterate()[3]
    m = torch.tensor(row_mask(mpc, bounds), device=mpc.device)
    assert torch.equal(dlb, torch.where(m[0], bnd[:, 0], torch.zeros_like(dlb))) and torch.equal(dub, torch.where(m[1], -bnd[:, 1], torch.zeros_like(dub)))
    got_V = np.stack([dlb.cpu().numpy(), dub.cpu().numpy()], 1)
    e_V = scaled(got_V[firm], np.stack([g13[key + "dV_dlb"][rows], g13[key + "dV_dub"][rows]], 1)[firm])
    return max(RTOL, 4.0 * err_dp), err_dp, e_firm, e_x, e_V, int(firm.sum()), int(act_x.sum())


def fmt(e):
    return " ".join(f"{v:.1e}" for v in e)


@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]])
def test_bound_vjp_against_the_mirror(g13, model, N):
    """Every instance of the fixture, then its first instance alone (B = 1); three cotangents each (two random over all of w, the
    unit vector on u_0).  MEASURED on an MI355X at the end of this file."""
    ocp, _ = C.problem(model, N)
    key = f"{model}_N{N}_"
    for rows in (slice(None), slice(0, 1)):
        bar, err_dp, e_firm, e_x, e_V, n, nx = fixture_case(g13, key, ocp, rows)
        print(f"bound vjp {model} N {N} B {len(g13[key + 'x0'][rows])}: firm ({n}): du0*/dp {err_dp:.1e} -> bar {bar:.1e}; g_lb, g_ub {fmt(e_firm)}; "
              f"dV/dlb, dV/dub {e_V:.1e}")
        if nx:
            print(f"bound vjp {model} N {N} B {len(g13[key + 'x0'][rows])}: active hard state row ({nx}): g_lb, g_ub {fmt(e_x)}")
        assert max(e_firm) <= bar and e_V <= bar, (model, N, bar, e_firm, e_V)
        assert max(e_x) <= bar, (model, N, bar, e_x)


# ---------------------------------------------------------------------- 2. the known answer, no fixture value
@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]])
def test_unit_cotangent_on_an_active_control_row_gives_one(g13, model, N):
    """A unit cotangent on a control the fixture marks as sitting on its bound, at a stage >= 1 and at stage 0: the control moves with
    that bound one to one (the gradient with respect to that row's active side is 1) and not with the other side (0), within the bar
    of the fixture test.  Negative control: an instance's gradient for its own random cotangent is farther than 100 x the bar from
    the reference of the next instance with an active row."""
    ocp, _ = C.problem(model, N)
    key = f"{model}_N{N}_"
    firm = ~g13[key + "soft"]
    x0 = g13[key + "x0"][firm]
    act = np.stack([g13[key + "act_lb"][firm][:, :, 0], g13[key + "act_ub"][firm][:, :, 0]], 1)      # [B, side, stage] of the one control
    mpc = handle(ocp, len(x0), fixture_bounds(g13, key))
    r = mpc.solve(x0, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * len(x0)
    ref_dp = g13[key + "dpi_dp"][firm].copy()
    ref_dp[g13[key + "act_u0"][firm]] = 0.0
    bar = max(RTOL, 4.0 * scaled(r.dpi_dp.cpu().numpy(), ref_dp))
    worst, seen = {}, {}
    for name, stages in (("stage >= 1", range(1, N)), ("stage 0", range(0, 1))):
        pick = [next(((k, sd) for k in stages for sd in (0, 1) if act[i, sd, k]), None) for i in range(len(x0))]
        gU = torch.zeros((mpc.B, mpc.N, mpc.nu), dtype=torch.float64, device=mpc.device)
        for i, p in enumerate(pick):
            if p is not None:
                gU[i, p[0], 0] = 1.0
        g = torch.stack(mpc.bound_vjp(None, gU, x0=False, theta=False)[2:], 1).cpu().numpy()      # [B, side, stage, coordinate]
        on = [abs(g[i, p[1], p[0], 0] - 1.0) for i, p in enumerate(pick) if p is not None]
        off = [abs(g[i, 1 - p[1], p[0], 0]) for i, p in enumerate(pick) if p is not None]
        worst[name], seen[name] = max(on + off), len(on)
    print(f"bound vjp {model} N {N} known answer: |g - 1| on the active side, |g| on the other: stage >= 1 ({seen['stage >= 1']}) "
          f"{worst['stage >= 1']:.1e}; stage 0 ({seen['stage 0']}) {worst['stage 0']:.1e}; bar {bar:.1e}")
    assert seen["stage >= 1"] >= 3 and seen["stage 0"] >= 1 and max(worst.values()) <= bar
    has = np.where(act.any((1, 2)))[0]
    gX, gU = split(mpc, g13[key + "G"][firm][:, 0])
    got = torch.stack(mpc.bound_vjp(gX, gU, x0=False, theta=False)[2:], 1).cpu().numpy()
    ref = np.stack([g13[key + "g_lb"][firm][:, 0], g13[key + "g_ub"][firm][:, 0]], 1)
    far = min(scaled(got[i:i + 1], ref[j:j + 1]) for i, j in zip(has, np.roll(has, -1)))
    print(f"bound vjp {model} N {N} negative control: nearest neighbour's reference at {far:.1e}")
    assert far > 100.0 * bar


# ---------------------------------------------------------------------- 3. contract
CP_BOUNDS = ([-8.0], [8.0], [-8.0, -0.6, -1.0, -0.4, -1.5], [8.0, 0.6, 1.0, 0.4, 1.5], [-0.6, -1.0, -0.4, -1.5], [0.6, 1.0, 0.4, 1.5])
LIN_BOUNDS = ([-0.3], [0.3], [-0.3, -1.0, -1.0], [0.3, 1.0, 1.0], [-1.0, -1.0], [1.0, 1.0])


@pytest.fixture(scope="module")
def cp16():
    """cartpole N 20, B 16 with the bounds of the fixture: the x0 distribution of tests/test_gpu_traj_vjp.py (a seed at which every
    instance is feasible inside the tightened box) with instance 5 made NaN, and one cotangent over all of w."""
    ocp, _ = C.problem("cartpole", 20)
    rng = np.random.default_rng(43)
    x0 = rng.uniform(-1, 1, (16, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    x0[5, 2] = float("nan")
    return ocp, x0, rng.standard_normal((16, 20 * 1 + 21 * 4))


def test_every_requested_row_is_written_for_every_output_combination(cp16):
    ocp, x0, G = cp16
    mpc = handle(ocp, 16, CP_BOUNDS)
    r = mpc.solve(x0, cold=True)
    gX, gU = split(mpc, G)
    before = [t.clone() for t in (r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian())]
    full = raw_vjp(mpc, gX, gU)
    st = r.status.cpu().numpy()
    assert st[5] == 1 and np.all(np.delete(st, 5) == 0)
    assert all(torch.isfinite(t).all() for t in full)
    assert all(torch.all(t[5] == 0) for t in full) and torch.all(full[0][4].abs() > 0)      # a NaN-x0 instance gives zero rows
    assert float(full[2].abs().max()) > 1e-3 or float(full[3].abs().max()) > 1e-3            # some control row is active in this batch
    for want in itertools.product((False, True), repeat=4):      # the 15 non-empty combinations, NaN-poisoned buffers
        if any(want):
            got = raw_vjp(mpc, gX, gU, want)
            assert all((g is None) == (not w) for g, w in zip(got, want)) and same(got, [f if w else None for f, w in zip(full, want)]), want
    # with the bound outputs NULL: the bits of mpcrl_traj_vjp; with them requested g_x0 and g_theta keep those bits
    traj = raw_traj_vjp(mpc, gX, gU)
    assert same(raw_vjp(mpc, gX, gU, (True, True, False, False))[:2], traj) and same(full[:2], traj)
    for a, b in ((gX, None), (None, gU)):      # a NULL cotangent counts as zeros
        za, zb = (torch.zeros_like(gX) if a is None else a), (torch.zeros_like(gU) if b is None else b)
        assert same(raw_vjp(mpc, a, b), raw_vjp(mpc, za, zb))
    m = torch.tensor(row_mask(mpc, CP_BOUNDS), device=mpc.device)
    assert torch.all(full[2][:, ~m[0]] == 0) and torch.all(full[3][:, ~m[1]] == 0)
    p = mpc.bound_vjp(gX, gU)      # the Python surface: the same numbers, rows selected by the status it holds
    assert same(p, full)
    dlb, dub = raw_value(mpc)
    assert torch.isfinite(dlb).all() and torch.all(dlb[5] == 0) and torch.all(dub[5] == 0) and torch.all(dlb >= 0) and torch.all(dub <= 0)
    assert same(raw_value(mpc, (True, False)), (dlb, None)) and same(raw_value(mpc, (False, True)), (None, dub))
    after = [r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian()]
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, after))      # (bytes: instance 5 holds NaN)


def test_an_absent_bound_gives_exact_zeros(cp16):
    """set_bounds with 1e30 on the upper bound of the pole angle (stages and terminal) and on the lower bound of the control."""
    ocp, x0, G = cp16
    lb0, ub0, lb, ub, lbe, ube = (list(b) for b in CP_BOUNDS)
    lb0[0], lb[0], ub[3], ube[2] = -1e30, -1e30, 1e30, 1e30
    mpc = handle(ocp, 16, (lb0, ub0, lb, ub, lbe, ube))
    r = mpc.solve(np.nan_to_num(x0, nan=0.1), cold=True)
    assert r.status.tolist() == [0] * 16
    gX, gU = split(mpc, G)
    _, _, g_lb, g_ub = raw_vjp(mpc, gX, gU)
    dlb, dub = raw_value(mpc)
    for lo, up in ((g_lb, g_ub), (dlb, dub)):
        assert torch.all(lo[:, :, 0] == 0) and torch.all(up[:, 1:20, 3] == 0) and torch.all(up[:, 20, 3] == 0)
        assert torch.all(lo[:, 0, 1:] == 0) and torch.all(up[:, 0, 1:] == 0) and torch.all(lo[:, 20, 0] == 0) and torch.all(up[:, 20, 0] == 0)
    assert torch.all(g_ub[:, 0, 0].abs() > 0) and torch.all(g_lb[:, 1:20, 3].abs() > 0) and torch.all(dlb[:, 1:, 3] > 0)


def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, chain_mass_ocp, linear_system_ocp
    lin = MPCBatch(linear_system_ocp(N=7), 3)
    x0 = np.array([[0.5, 0.1], [0.3, 0.2], [0.6, -0.1]])
    gX, gU = split(lin, np.ones((3, 7 + 8 * 2)))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU)                                        # before any solve
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(lin)
    with pytest.raises(RuntimeError):
        lin.bound_vjp(gX, gU)
    with pytest.raises(RuntimeError):
        lin.bound_value_grad()
    lin.solve(x0, cold=True, store_bounds=False)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU)                                        # the bound planes are placeholders
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(lin)
    with pytest.raises(RuntimeError):
        lin.bound_vjp(gX, gU)
    lin.solve(x0, cold=True)
    assert all(torch.isfinite(t).all() for t in raw_vjp(lin, gX, gU)) and all(torch.isfinite(t).all() for t in raw_value(lin))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, None, None)                                    # both cotangents NULL
    with pytest.raises(ValueError):
        lin.bound_vjp(None, None)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU, (False, False, False, False))          # all outputs NULL
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(lin, (False, False))
    with pytest.raises(ValueError):
        lin.bound_vjp(gX, gU, x0=False, theta=False, bounds=False)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU, flags=_lib.STATE_Q_MODE)               # Q mode is not offered on the VJP
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(lin, flags=4)                                     # an unknown flag
    x, u, pi, _, _ = lin.get_iterate()
    lin.set_iterate(x, u, pi)                                       # without bnd
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(lin)
    lin.solve(x0, np.full((3, 1), 0.1), cold=True)                  # a solve with u0 fixed
    with pytest.raises(RuntimeError, match="Q mode"):
        lin.bound_vjp(gX, gU)
    chain = MPCBatch(chain_mass_ocp(n_mass=3, N=10), 2)
    chain.solve(np.tile(chain.ocp.x0, (2, 1)), cold=True)
    cX, cU = split(chain, np.ones((2, 10 * chain.nu + 11 * chain.nx)))
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        raw_vjp(chain, cX, cU)
    st = torch.zeros(3, dtype=torch.int32, device=lin.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):        # the chain's call on a small model
        lin._call("mpcrl_chain_bound_vjp", 0, st, gX, gU, *raw_vjp_buffers(lin))


def raw_vjp_buffers(mpc):
    return [torch.zeros(sh, dtype=torch.float64, device=mpc.device) for sh in shapes(mpc)]


def test_bound_value_grad_in_q_mode_against_differences_of_q():
    """u_0 pinned: the control entries of stage 0 are exactly zero (the pin's gradient is dQ/du0), the rest is lam_l / -lam_u; summed
    over the stages 1 .. N-1 that share it, the control's upper bound against central differences of Q."""
    from mpc4rl_amd import _lib
    ocp, _ = C.problem("linear", 8)
    x0 = np.array([[0.7, 0.3], [0.8, 0.35], [0.3, -0.1]])
    u0 = np.array([[0.1], [-0.2], [0.0]])
    mpc = handle(ocp, 3, LIN_BOUNDS, tol=1e-10)
    r = mpc.solve(x0, u0, cold=True)
    assert r.status.tolist() == [0] * 3
    dlb, dub = mpc.bound_value_grad(q_mode=True)
    assert torch.all(dlb[:, 0] == 0) and torch.all(dub[:, 0] == 0) and torch.all(dlb[:, 8, 0] == 0) and torch.all(dub[:, 8, 0] == 0)
    bnd = mpc.get_iterate()[3]
    assert torch.equal(dlb[:, 1:8], bnd[:, 0, 1:8]) and torch.equal(dub[:, 1:8], -bnd[:, 1, 1:8])
    got = torch.stack([dlb[:, 1:8, 0].sum(1), dub[:, 1:8, 0].sum(1)], 1).cpu().numpy()      # d Q / d lbu, d Q / d ubu of the stages
    Q, h = {}, 1e-4
    for side in (0, 1):
        for sgn in (1.0, -1.0):
            lb, ub = list(LIN_BOUNDS[2]), list(LIN_BOUNDS[3])
            (ub if side else lb)[0] += sgn * h
            mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
            rr = mpc.solve(x0, u0, cold=True)
            assert rr.status.tolist() == [0] * 3
            Q[side, sgn] = rr.V.cpu().numpy()
    ref = np.stack([(Q[s, 1.0] - Q[s, -1.0]) / (2 * h) for s in (0, 1)], 1)
    err = scaled(got, ref)
    print(f"bound value grad linear N 8 Q mode: d Q / d (lbu, ubu) of the stages against differences {err:.1e}; largest {np.abs(ref).max():.2e}")
    assert np.abs(ref).max() > 1e-3 and err <= 1e-6


# ---------------------------------------------------------------------- 4. the same bits
def test_same_bits_whatever_the_order_and_the_launch_shape(cp16):
    """An explicit reversed packing order, the time-sliced against the plain solve launch, and a second call: the same bits."""
    ocp, x0, G = cp16
    x0 = np.nan_to_num(x0, nan=0.1)
    ref = None
    for mode, perm in ((-1, None), (1, None), (-1, torch.arange(15, -1, -1))):
        mpc = handle(ocp, 16, CP_BOUNDS)
        mpc.set_launch_mode(mode)
        mpc.set_order(perm)
        mpc.solve(x0, cold=True, reorder=False)
        gX, gU = split(mpc, G)
        a, b = raw_vjp(mpc, gX, gU) + raw_value(mpc), raw_vjp(mpc, gX, gU) + raw_value(mpc)
        assert same(a, b)
        ref = a if ref is None else ref
        assert same(a, ref), (mode, perm is not None)
    assert all(torch.isfinite(t).all() for t in ref) and float(ref[2].abs().max()) > 0


# ---------------------------------------------------------------------- 5. inside a graph
def test_replays_inside_a_graph(cp16):
    ocp, x0, G = cp16
    mpc = handle(ocp, 16, CP_BOUNDS)
    mpc.solve(np.nan_to_num(x0, nan=0.1), cold=True)
    gX, gU = split(mpc, G)
    want = raw_vjp(mpc, gX, gU) + raw_value(mpc)
    bufs = raw_vjp_buffers(mpc) + [torch.zeros(shapes(mpc)[2], dtype=torch.float64, device=mpc.device) for _ in range(2)]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream: a chain of two nodes, no parallel branches
        mpc._call("mpcrl_bound_vjp", 0, gX, gU, *bufs[:4])
        mpc._call("mpcrl_bound_value_grad", 0, *bufs[4:])
    torch.cuda.synchronize()
    assert all(torch.all(t == 0) for t in bufs)      # captured, not run
    for _ in range(2):
        for t in bufs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same(bufs, want)


# ---------------------------------------------------------------------- 6. the layer
def layer_differences(f, z, h=1e-5):
    """d f(z) / d z of a scalar f by central differences, entry by entry (z a float64 tensor)."""
    g = torch.zeros_like(z)
    flat, gf = z.reshape(-1), g.reshape(-1)
    for j in range(flat.numel()):
        keep = flat[j].item()
        flat[j] = keep + h
        fp = f(z)
        flat[j] = keep - h
        fm = f(z)
        flat[j] = keep
        gf[j] = (fp - fm) / (2 * h)
    return g


LAYER_CASES = {"linear": (8, 3, LIN_BOUNDS, np.array([[0.7, 0.3], [0.45, -0.25], [0.8, 0.1]])),
               "cartpole": (6, 2, ([-1.0], [1.0], [-1.0, -0.6, -1.0, -0.4, -1.5], [1.0, 0.6, 1.0, 0.4, 1.5], [-0.6, -1.0, -0.4, -1.5], [0.6, 1.0, 0.4, 1.5]),
                            np.array([[0.2, 0.1, 0.15, -0.2], [-0.3, 0.2, -0.2, 0.1]]))}


def layer_case(model):
    from mpc4rl_amd import BoxBounds, MPCLayer
    N, B, bounds, x0 = LAYER_CASES[model]
    ocp, _ = C.problem(model, N)
    rng = np.random.default_rng(61)
    Wx = torch.tensor(rng.uniform(-1, 1, (B, N + 1, ocp.nx)), device="cuda")
    Wu = torch.tensor(rng.uniform(-1, 1, (B, N, ocp.nu)), device="cuda")
    wu, wV = torch.tensor(rng.uniform(-1, 1, (B, ocp.nu)), device="cuda"), torch.tensor(rng.uniform(-1, 1, B), device="cuda")
    layer = MPCLayer(handle(ocp, B, tol=1e-10), cold=True)

    def box(grad=True):
        return BoxBounds(*(torch.tensor(b, dtype=torch.float64, requires_grad=grad) for b in bounds))

    def traj_loss(x, th, b):
        X, U = layer.trajectory(x, th, b)
        return (Wx * X).sum() + (Wu * U).sum()

    def fwd_loss(x, th, b):
        u0, V = layer(x, th, b)
        return (wu * u0).sum() + (wV * V).sum()

    return ocp, layer, torch.tensor(x0, device="cuda"), box, traj_loss, fwd_loss


@pytest.mark.parametrize("model", ["linear", "cartpole"])
def test_layer_bound_gradients_against_differences_of_its_forward_pass(model):
    """d loss / d bounds of ``trajectory`` and of ``forward`` over all six members of the BoxBounds (the bounds tightened so that a
    control row is active), against central differences of the layer's own forward pass; x0.grad and theta.grad of the same backward
    pass are those of the layer without ``bounds``, bit for bit."""
    ocp, layer, x0, box, traj_loss, fwd_loss = layer_case(model)
    B = len(x0)
    for name, loss in (("trajectory", traj_loss), ("forward", fwd_loss)):
        x, theta, b = x0.clone().requires_grad_(True), torch.tensor(ocp.p0, device="cuda", requires_grad=True), box()
        loss(x, theta, b).backward()
        assert layer.last_status.tolist() == [0] * B
        bnd = layer.batch.get_iterate()[3]
        assert float(bnd[:, 2:4, :-1, 0].min()) < 1e-8      # a control row is active
        x2, theta2 = x0.clone().requires_grad_(True), torch.tensor(ocp.p0, device="cuda", requires_grad=True)
        loss(x2, theta2, None).backward()                   # the batch keeps the bounds the pass before set
        assert same((x.grad, theta.grad), (x2.grad, theta2.grad))
        errs = []
        with torch.no_grad():
            for i, member in enumerate(b):
                def f(z, i=i):
                    return float(loss(x0, theta.detach(), box(False)._replace(**{b._fields[i]: z})))
                fd = layer_differences(f, member.detach().clone())
                errs.append(scaled(member.grad[None], fd.numpy()[None]))
        print(f"layer.{name} {model} N {layer.batch.N} with bounds: d loss/d (lb0 ub0 lb ub lbe ube) {fmt(errs)}; "
              f"largest |gradient| {max(float(m.grad.abs().max()) for m in b):.2e}")
        assert max(float(m.grad.abs().max()) for m in b) > 1e-2 and max(errs) <= 1e-5


def test_layer_bounds_staleness_and_failed_instance():
    from mpc4rl_amd import BoxBounds, MPCLayer
    ocp, layer, x0, box, traj_loss, fwd_loss = layer_case("cartpole")
    theta = torch.tensor(ocp.p0, device="cuda")
    for loss in (traj_loss, fwd_loss):
        out = loss(x0, theta, box())
        layer(x0, theta)                                              # the handle now holds another pass's iterate
        with pytest.raises(RuntimeError, match="one backward per forward"):
            out.backward()
    # an instance whose solve failed contributes exactly zero: the gradients are those of the other instance alone
    bounds = LAYER_CASES["cartpole"][2]
    grads = []
    for xs in (x0[:1], torch.cat([x0[:1], torch.tensor([[0.1, 0.0, float("nan"), 0.0]], device="cuda")])):
        lay = MPCLayer(handle(ocp, len(xs), tol=1e-10), cold=True)
        b = BoxBounds(*(torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in bounds))
        X, U = lay.trajectory(xs, theta, b)
        (torch.nan_to_num(X)[:1].sum() + 2.0 * torch.nan_to_num(U)[:1].sum()).backward()
        assert lay.last_status.tolist() == [0, 1][:len(xs)]
        grads.append([m.grad.clone() for m in b])
        u0, V = lay(xs, theta, b)
        (torch.nan_to_num(u0).sum() + torch.nan_to_num(V).sum()).backward()
        grads[-1] += [m.grad.clone() for m in b]
    assert all(torch.isfinite(g).all() for g in grads[1]) and same(grads[0], grads[1])


MEASURED = """\
bound vjp cartpole N 2 B 5: firm (5): du0*/dp 3.7e-08 -> bar 1.0e-06; g_lb, g_ub 7.0e-08 1.6e-08 3.6e-08; dV/dlb, dV/dub 2.4e-11
bound vjp cartpole N 2 B 1: firm (1): du0*/dp 3.7e-08 -> bar 1.0e-06; g_lb, g_ub 7.0e-08 1.6e-08 3.6e-08; dV/dlb, dV/dub 1.5e-11
bound vjp cartpole N 15 B 7: firm (7): du0*/dp 9.0e-08 -> bar 1.0e-06; g_lb, g_ub 9.2e-08 5.7e-08 4.4e-08; dV/dlb, dV/dub 1.3e-09
bound vjp cartpole N 15 B 7: active hard state row (2): g_lb, g_ub 9.2e-08 5.7e-08 4.4e-08
bound vjp cartpole N 15 B 1: firm (1): du0*/dp 1.5e-11 -> bar 1.0e-06; g_lb, g_ub 5.2e-09 3.1e-09 2.1e-11; dV/dlb, dV/dub 7.6e-12
bound vjp cartpole N 20 B 6: firm (6): du0*/dp 4.6e-09 -> bar 1.0e-06; g_lb, g_ub 2.5e-09 9.3e-09 1.2e-10; dV/dlb, dV/dub 6.8e-11
bound vjp cartpole N 20 B 6: active hard state row (1): g_lb, g_ub 2.2e-09 1.3e-09 7.1e-12
bound vjp cartpole N 20 B 1: firm (1): du0*/dp 4.6e-09 -> bar 1.0e-06; g_lb, g_ub 3.4e-10 3.7e-10 1.2e-10; dV/dlb, dV/dub 1.7e-11
bound vjp cartpole N 31 B 5: firm (5): du0*/dp 2.3e-07 -> bar 1.0e-06; g_lb, g_ub 9.8e-09 4.7e-09 1.6e-10; dV/dlb, dV/dub 7.1e-10
bound vjp cartpole N 31 B 5: active hard state row (2): g_lb, g_ub 9.8e-09 4.7e-09 4.3e-12
bound vjp cartpole N 31 B 1: firm (1): du0*/dp 2.3e-07 -> bar 1.0e-06; g_lb, g_ub 2.1e-10 2.4e-10 7.3e-11; dV/dlb, dV/dub 1.1e-11
bound vjp cartpole N 32 B 6: firm (6): du0*/dp 3.6e-08 -> bar 1.0e-06; g_lb, g_ub 7.0e-09 8.8e-09 9.6e-09; dV/dlb, dV/dub 1.4e-10
bound vjp cartpole N 32 B 6: active hard state row (1): g_lb, g_ub 1.3e-09 4.3e-10 9.6e-12
bound vjp cartpole N 32 B 1: firm (1): du0*/dp 2.4e-08 -> bar 1.0e-06; g_lb, g_ub 7.0e-09 8.8e-09 9.6e-09; dV/dlb, dV/dub 2.4e-11
bound vjp cartpole N 63 B 7: firm (7): du0*/dp 5.6e-08 -> bar 1.0e-06; g_lb, g_ub 9.0e-08 5.3e-08 1.9e-09; dV/dlb, dV/dub 1.2e-08
bound vjp cartpole N 63 B 7: active hard state row (2): g_lb, g_ub 9.0e-08 7.3e-09 1.9e-09
bound vjp cartpole N 63 B 1: firm (1): du0*/dp 5.2e-08 -> bar 1.0e-06; g_lb, g_ub 8.4e-10 9.2e-10 1.2e-10; dV/dlb, dV/dub 2.0e-11
bound vjp linear N 2 B 5: firm (5): du0*/dp 2.2e-08 -> bar 1.0e-06; g_lb, g_ub 1.6e-09 4.0e-09 1.8e-09; dV/dlb, dV/dub 1.9e-13
bound vjp linear N 2 B 1: firm (1): du0*/dp 5.1e-09 -> bar 1.0e-06; g_lb, g_ub 1.4e-09 2.1e-09 1.8e-09; dV/dlb, dV/dub 1.2e-15
bound vjp linear N 7 B 6: firm (5): du0*/dp 3.8e-08 -> bar 1.0e-06; g_lb, g_ub 4.4e-09 5.9e-09 3.4e-09; dV/dlb, dV/dub 2.1e-15
bound vjp linear N 7 B 1: firm (1): du0*/dp 3.2e-08 -> bar 1.0e-06; g_lb, g_ub 6.7e-15 1.4e-15 5.2e-15; dV/dlb, dV/dub 9.1e-18
bound vjp linear N 20 B 6: firm (5): du0*/dp 5.2e-08 -> bar 1.0e-06; g_lb, g_ub 5.3e-09 3.4e-09 3.9e-09; dV/dlb, dV/dub 2.9e-13
bound vjp linear N 20 B 1: firm (1): du0*/dp 4.2e-08 -> bar 1.0e-06; g_lb, g_ub 1.8e-15 1.4e-15 2.1e-16; dV/dlb, dV/dub 2.9e-24
bound vjp linear N 31 B 5: firm (5): du0*/dp 8.9e-08 -> bar 1.0e-06; g_lb, g_ub 5.1e-09 8.8e-09 5.3e-09; dV/dlb, dV/dub 5.9e-14
bound vjp linear N 31 B 1: firm (1): du0*/dp 1.3e-08 -> bar 1.0e-06; g_lb, g_ub 4.7e-09 6.4e-09 1.7e-09; dV/dlb, dV/dub 5.6e-16
bound vjp linear N 32 B 5: firm (5): du0*/dp 3.0e-08 -> bar 1.0e-06; g_lb, g_ub 3.4e-08 4.7e-08 2.8e-09; dV/dlb, dV/dub 5.2e-09
bound vjp linear N 32 B 1: firm (1): du0*/dp 2.3e-08 -> bar 1.0e-06; g_lb, g_ub 1.5e-09 3.7e-09 2.4e-09; dV/dlb, dV/dub 1.5e-14
bound vjp linear N 63 B 5: firm (5): du0*/dp 3.9e-08 -> bar 1.0e-06; g_lb, g_ub 2.7e-09 2.5e-09 3.3e-09; dV/dlb, dV/dub 3.7e-15
bound vjp linear N 63 B 1: firm (1): du0*/dp 3.0e-08 -> bar 1.0e-06; g_lb, g_ub 2.7e-14 2.2e-14 1.1e-15; dV/dlb, dV/dub 4.0e-25
bound vjp cartpole N 2 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 1.2e-12; stage 0 (3) 1.3e-12; bar 1.0e-06
bound vjp cartpole N 2 negative control: nearest neighbour's reference at 6.3e-01
bound vjp cartpole N 15 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (4) 1.8e-12; stage 0 (4) 2.0e-12; bar 1.0e-06
bound vjp cartpole N 15 negative control: nearest neighbour's reference at 1.0e+00
bound vjp cartpole N 20 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (4) 1.7e-12; stage 0 (4) 1.9e-12; bar 1.0e-06
bound vjp cartpole N 20 negative control: nearest neighbour's reference at 9.6e-01
bound vjp cartpole N 31 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 1.5e-12; stage 0 (3) 1.8e-12; bar 1.0e-06
bound vjp cartpole N 31 negative control: nearest neighbour's reference at 1.0e+00
bound vjp cartpole N 32 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (4) 1.5e-12; stage 0 (4) 1.8e-12; bar 1.0e-06
bound vjp cartpole N 32 negative control: nearest neighbour's reference at 1.0e+00
bound vjp cartpole N 63 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (5) 1.9e-12; stage 0 (5) 2.3e-12; bar 1.0e-06
bound vjp cartpole N 63 negative control: nearest neighbour's reference at 9.6e-01
bound vjp linear N 2 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 1.5e-09; stage 0 (3) 1.8e-09; bar 1.0e-06
bound vjp linear N 2 negative control: nearest neighbour's reference at 4.9e-01
bound vjp linear N 7 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 8.5e-09; stage 0 (3) 3.4e-09; bar 1.0e-06
bound vjp linear N 7 negative control: nearest neighbour's reference at 1.4e+00
bound vjp linear N 20 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 3.3e-09; stage 0 (3) 3.9e-09; bar 1.0e-06
bound vjp linear N 20 negative control: nearest neighbour's reference at 1.2e+00
bound vjp linear N 31 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 4.5e-09; stage 0 (3) 5.3e-09; bar 1.0e-06
bound vjp linear N 31 negative control: nearest neighbour's reference at 6.2e-01
bound vjp linear N 32 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 4.4e-08; stage 0 (3) 2.8e-09; bar 1.0e-06
bound vjp linear N 32 negative control: nearest neighbour's reference at 7.9e-01
bound vjp linear N 63 known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (3) 2.8e-09; stage 0 (3) 3.3e-09; bar 1.0e-06
bound vjp linear N 63 negative control: nearest neighbour's reference at 1.2e+00
bound value grad linear N 8 Q mode: d Q / d (lbu, ubu) of the stages against differences 5.8e-10; largest 1.61e+02
layer.trajectory linear N 8 with bounds: d loss/d (lb0 ub0 lb ub lbe ube) 5.7e-07 3.1e-08 1.1e-06 3.8e-08 9.1e-10 9.9e-08; largest |gradient| 2.34e+00
layer.forward linear N 8 with bounds: d loss/d (lb0 ub0 lb ub lbe ube) 5.3e-11 7.8e-10 6.2e-10 3.6e-09 4.5e-11 2.0e-10; largest |gradient| 4.90e+00
layer.trajectory cartpole N 6 with bounds: d loss/d (lb0 ub0 lb ub lbe ube) 1.4e-10 1.1e-11 8.3e-11 4.9e-10 1.8e-10 1.7e-10; largest |gradient| 1.25e+00
layer.forward cartpole N 6 with bounds: d loss/d (lb0 ub0 lb ub lbe ube) 2.4e-10 1.9e-10 1.4e-10 3.1e-10 9.4e-11 1.1e-10; largest |gradient| 5.03e-01
"""
