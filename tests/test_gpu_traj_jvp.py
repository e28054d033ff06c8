"""mpcrl_traj_jvp (include/mpcrl_traj_jvp_ext.h) on the device: the Jacobian-vector product of the whole planned trajectory from
small_traj_jvp_kernel against the mirror fixture G15 (tests/golden/make_traj_jvp.py), against the library's own trajectory VJP by the
adjoint identity <G, J v> = <J' G, v>, against du0*/dp and du0*/dx0 for the unit directions, the same bits under every layout, and
the call's contract.

Bars.  Against the fixture: the bar of tests/test_gpu_traj_vjp.py, max(1e-6, 4 x the error of the solve's own du0*/dp against G9's
mirror du0*/dp on the same instances), asserted on the instances without a positive slack (with one the mirror holds the slacks
constant and is the definition, not a yardstick).  Rows are scaled by max(|reference row|, 1).  Inside the library (the adjoint
identity, unit directions against sens_pi / state_sens): 1e-6, relative to max(|either side|, 1) for the identity.

Measured on an MI355X: MEASURED at the end of this file (every line the tests print).
"""
import functools
import os

import numpy as np
import pytest
import torch

import small_mode_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
CASES = [(m, N) for m in HORIZONS for N in HORIZONS[m]]
RTOL = C.RTOL
R = 3


@pytest.fixture(scope="module")
def g9():
    return np.load(os.path.join(GOLD, "g9_state_sens.npz"))


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(GOLD, "g11_traj_vjp.npz"))


@functools.lru_cache(maxsize=None)
def g15():
    return np.load(os.path.join(GOLD, "g15_traj_jvp.npz"))


def scaled(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    got, ref = got.reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)).max())


def handle(ocp, B, tol=1e-9):
    from mpc4rl_amd import MPCBatch
    mpc = MPCBatch(ocp, B)
    mpc.set_options(tol=tol)
    return mpc


def same(a, b):
    """bit-identical, NaN included"""
    return all((x is None and y is None) or torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))
               for x, y in zip(a, b))


def dev(mpc, a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=mpc.device)


def raw_jvp(mpc, ndir, dx0, dth, want=(True, True), flags=0, fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    shapes = ((mpc.B, max(ndir, 1), mpc.N + 1, mpc.nx), (mpc.B, max(ndir, 1), mpc.N, mpc.nu))
    bufs = [torch.full(sh, fill, **kw) if w else None for sh, w in zip(shapes, want)]
    mpc._call("mpcrl_traj_jvp", flags, ndir, dx0, dth, *bufs)
    torch.cuda.synchronize()
    return bufs


@functools.lru_cache(maxsize=None)
def solved(model, N):
    """One cold solve at tol 1e-9 on every instance of G15 at (model, N), with du0*/dp, and the state sensitivities of it: shared by
    the tests below, which leave the handle as it is (the calls under test do not change it)."""
    ocp, _ = C.problem(model, N)
    x0 = g15()[f"{model}_N{N}_x0"]
    mpc = handle(ocp, len(x0))
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * len(x0), (model, N, r.status.tolist())
    return mpc, r, mpc.state_sens(value=False)


def fmt(e):
    return " ".join(f"{v:.1e}" for v in e)


# ---------------------------------------------------------------------- 1. against the fixture
def fixture_case(g9, g11, key, ocp, rows, theta=None, share=None):
    """Cold solve at tol 1e-9 on the fixture's x0, then one trajectory_jvp with R = 3.  Returns (bar, error of the solve's own
    du0*/dp, errors of dX and dU per direction, number of asserted instances)."""
    fx = g15()
    idx9 = g11[key + "idx"][fx[key + "idx"]][rows]      # row of G15 -> row of G11 -> row of G9
    x0 = fx[key + "x0"][rows]
    if share is not None:
        mpc, r = share
    else:
        mpc = handle(ocp, len(x0))
        if theta is not None:
            mpc.set_theta(theta[rows])
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
    firm = ~fx[key + "soft"][rows] if key + "soft" in fx.files else np.ones(len(x0), bool)
    dX, dU = mpc.trajectory_jvp(dev(mpc, fx[key + "vx"][rows]), dev(mpc, fx[key + "vp"][rows]))
    assert dX.shape == (len(x0), R, mpc.N + 1, mpc.nx) and dU.shape == (len(x0), R, mpc.N, mpc.nu)
    if not firm.any():
        return RTOL, 0.0, [0.0] * R, [0.0] * R, 0
    ref_dp = g9[key + "dpi_dp"][idx9].copy()
    if key + "cls" in g9.files:
        ref_dp[g9[key + "cls"][idx9] == 2] = 0.0      # u_0 on its bound: the exact zero, as tests/test_gpu_state_sens.py takes it
    err_dp = scaled(r.dpi_dp.cpu().numpy()[firm], ref_dp[firm])
    dX, dU = dX.cpu().numpy(), dU.cpu().numpy()
    e_X = [scaled(dX[firm, c], fx[key + "dX"][rows][firm, c]) for c in range(R)]
    e_U = [scaled(dU[firm, c], fx[key + "dU"][rows][firm, c]) for c in range(R)]
    return max(RTOL, 4.0 * err_dp), err_dp, e_X, e_U, int(firm.sum())


@pytest.mark.parametrize("model,N", CASES)
def test_trajectory_jvp_against_the_mirror(g9, g11, model, N):
    """Every instance of the fixture, then its first instance alone (B = 1); three directions each (x0 and theta, theta only, x0
    only).  Asserted on the instances without a positive slack; at linear N 31, 32 and 63 the fixture has none
    (tests/golden/make_traj_vjp.py says why) and the case only runs the call: those lane layouts are held to numbers by the adjoint
    identity and the unit directions below.  MEASURED on an MI355X at the end of this file."""
    ocp, _ = C.problem(model, N)
    key = f"{model}_N{N}_"
    for rows, share in ((slice(None), solved(model, N)[:2]), (slice(0, 1), None)):
        bar, err_dp, e_X, e_U, n = fixture_case(g9, g11, key, ocp, rows, share=share)
        print(f"traj jvp {model} N {N} B {len(g15()[key + 'idx'][rows])}: no positive slack ({n}): du0*/dp {err_dp:.1e} -> bar {bar:.1e}; "
              f"dX {fmt(e_X)}; dU {fmt(e_U)}")
        assert max(e_X) <= bar and max(e_U) <= bar, (model, N, bar, e_X, e_U)


@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_per_instance_theta_against_the_mirror(g9, g11, model):
    ocp, _ = C.problem(model, 20)
    key = f"{model}_th_"
    bar, err_dp, e_X, e_U, n = fixture_case(g9, g11, key, ocp, slice(None), theta=g15()[key + "theta"])
    print(f"traj jvp {model} per-instance theta ({n}): du0*/dp {err_dp:.1e} -> bar {bar:.1e}; dX {fmt(e_X)}; dU {fmt(e_U)}")
    assert n == 2 and max(e_X) <= bar and max(e_U) <= bar


# ---------------------------------------------------------------------- 2. the adjoint identity inside the library
@pytest.mark.parametrize("model,N", CASES)
def test_adjoint_identity_with_the_trajectory_vjp(g11, model, N):
    """<gX, dX> + <gU, dU> from trajectory_jvp against <g_x0, vx> + <g_theta, vp> from trajectory_vjp, on one handle and one solve:
    G11's three cotangents times G15's three directions, every instance of the fixture, positive slacks included.  Two kernels, one
    linearised system: a wrong sign or a missing term of the right-hand side is an error of order one."""
    fx = g15()
    key = f"{model}_N{N}_"
    mpc, _, _ = solved(model, N)
    vx, vp = dev(mpc, fx[key + "vx"]), dev(mpc, fx[key + "vp"])
    dX, dU = mpc.trajectory_jvp(vx, vp)
    G = dev(mpc, g11[key + "G"][fx[key + "idx"]])      # [B, 3, nw], the mirror's order w = [U; X]
    n = mpc.N * mpc.nu
    worst, size = 0.0, 0.0
    for c in range(3):
        gX, gU = G[:, c, n:].reshape(mpc.B, mpc.N + 1, mpc.nx).contiguous(), G[:, c, :n].reshape(mpc.B, mpc.N, mpc.nu).contiguous()
        g_x0, g_th = mpc.trajectory_vjp(gX, gU)
        lhs = (gX[:, None] * dX).sum((2, 3)) + (gU[:, None] * dU).sum((2, 3))      # [B, R]
        rhs = (g_x0[:, None] * vx).sum(2) + (g_th[:, None] * vp).sum(2)
        rel = (lhs - rhs).abs() / torch.maximum(torch.maximum(lhs.abs(), rhs.abs()), torch.ones_like(lhs))
        worst, size = max(worst, float(rel.max())), max(size, float(lhs.abs().max()))
    print(f"traj jvp {model} N {N} adjoint identity: {worst:.1e} (largest product {size:.1e})")
    assert size > 1e-3 and worst <= RTOL


# ---------------------------------------------------------------------- 3. unit directions against the existing sensitivities
@pytest.mark.parametrize("model,N", CASES)
def test_jacobian_rows_of_u0_are_the_first_move_jacobians(model, N):
    mpc, r, s = solved(model, N)
    J = mpc.trajectory_jacobian()
    nd = mpc.n_diff()
    assert nd == (3 if model == "cartpole" else 12)
    assert J.dX_dx0.shape == (mpc.B, N + 1, mpc.nx, mpc.nx) and J.dU_dx0.shape == (mpc.B, N, mpc.nu, mpc.nx)
    assert J.dX_dtheta.shape == (mpc.B, N + 1, mpc.nx, mpc.n_p) and J.dU_dtheta.shape == (mpc.B, N, mpc.nu, mpc.n_p)
    e_t, e_x = scaled(J.dU_dtheta[:, 0], r.dpi_dp.cpu().numpy()), scaled(J.dU_dx0[:, 0], s.dpi_dx0.cpu().numpy())
    print(f"traj jvp {model} N {N} unit directions inside the library: dU_dtheta[0] against du0*/dp {e_t:.1e}; "
          f"dU_dx0[0] against du0*/dx0 {e_x:.1e}")
    assert e_t <= RTOL and e_x <= RTOL
    assert torch.equal(J.dX_dx0[:, 0], torch.eye(mpc.nx, dtype=torch.float64, device=mpc.device).expand(mpc.B, -1, -1))
    assert torch.all(J.dX_dtheta[:, 0] == 0)      # x_0 = x0 does not move with theta
    assert torch.all(J.dX_dtheta[..., nd:] == 0) and torch.all(J.dU_dtheta[..., nd:] == 0)
    assert float(J.dX_dtheta[..., :nd].abs().max()) > 0 and float(J.dU_dx0.abs().max()) > 0


# ---------------------------------------------------------------------- 4. layout
@pytest.mark.parametrize("model,N", CASES)
def test_same_bits_whatever_the_number_of_directions_the_batch_and_the_order(model, N):
    """R = 3 against three R = 1 calls; the batch against B = 1 handles on its first, a middle and its last instance; an explicit
    reversed packing order against none."""
    fx = g15()
    key = f"{model}_N{N}_"
    mpc, _, _ = solved(model, N)
    vx, vp = dev(mpc, fx[key + "vx"]), dev(mpc, fx[key + "vp"])
    ref = raw_jvp(mpc, R, vx, vp)
    assert all(torch.isfinite(t).all() for t in ref)
    for c in range(R):
        one = raw_jvp(mpc, 1, vx[:, c].contiguous(), vp[:, c].contiguous())
        assert same([t[:, 0] for t in one], [t[:, c] for t in ref]), c
    perm, _ = mpc.get_order()
    mpc.set_order(torch.arange(mpc.B - 1, -1, -1))
    try:
        assert same(raw_jvp(mpc, R, vx, vp), ref)
    finally:
        mpc.set_order(perm)
    ocp, _ = C.problem(model, N)
    for i in sorted({0, mpc.B // 2, mpc.B - 1}):
        m1 = handle(ocp, 1)
        assert m1.solve(fx[key + "x0"][i:i + 1], cold=True).status.tolist() == [0]
        assert same(raw_jvp(m1, R, vx[i:i + 1].contiguous(), vp[i:i + 1].contiguous()), [t[i:i + 1] for t in ref]), i


# ---------------------------------------------------------------------- 5. contract
@pytest.fixture(scope="module")
def cp16():
    """cartpole N 20, B 16: x0 of tests/test_gpu_traj_vjp.py with instance 5 made NaN (status 1), and three directions."""
    ocp, _ = C.problem("cartpole", 20)
    rng = np.random.default_rng(41)
    x0 = rng.uniform(-1, 1, (16, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    x0[5, 2] = float("nan")
    vp = np.zeros((16, R, 83))
    vp[..., :3] = rng.standard_normal((16, R, 3))
    return ocp, x0, rng.standard_normal((16, R, 4)), vp


def test_every_requested_row_is_written_and_failed_instances_are_zero(cp16):
    ocp, x0, vx, vp = cp16
    mpc = handle(ocp, 16)
    r = mpc.solve(x0, cold=True)
    vx, vp = dev(mpc, vx), dev(mpc, vp)
    before = [t.clone() for t in (r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian())]
    dX, dU = raw_jvp(mpc, R, vx, vp)
    st = r.status.cpu().numpy()
    assert st[5] == 1 and np.all(np.delete(st, 5) == 0)
    assert torch.isfinite(dX).all() and torch.isfinite(dU).all()
    assert torch.all(dX[5] == 0) and torch.all(dU[5] == 0) and torch.all(dX[4].abs() > 0) and torch.all(dU[4].abs() > 0)
    ok = torch.as_tensor(st == 0, device=mpc.device)
    assert same((dX[ok][:, :, 0],), (vx[ok],))      # x_0 = x0: the row of stage 0 of a solved instance is the direction itself
    only_X, only_U = raw_jvp(mpc, R, vx, vp, (True, False)), raw_jvp(mpc, R, vx, vp, (False, True))
    assert only_X[1] is None and only_U[0] is None and same((only_X[0], only_U[1]), (dX, dU))
    for a, b in ((vx, None), (None, vp)):      # a NULL direction counts as zeros
        za, zb = (torch.zeros_like(vx) if a is None else a), (torch.zeros_like(vp) if b is None else b)
        assert same(raw_jvp(mpc, R, a, b), raw_jvp(mpc, R, za, zb))
    junk = vp.clone()
    junk[..., 3:] = 7.0                        # the cartpole's cost block of a direction is not read
    assert same(raw_jvp(mpc, R, vx, junk), (dX, dU))
    p = mpc.trajectory_jvp(vx, vp)             # the Python surface: the same numbers, rows selected by the status it holds
    assert same(p, (dX, dU))
    p1 = mpc.trajectory_jvp(vx[:, 1], vp[:, 1])                    # [B, nx] / [B, np]: outputs without the direction axis
    assert p1[0].shape == (16, 21, 4) and p1[1].shape == (16, 20, 1) and same(p1, (dX[:, 1], dU[:, 1]))
    pb = mpc.trajectory_jvp(None, vp[3, 0])                        # a 1-D dtheta broadcasts over the batch
    assert same(pb, mpc.trajectory_jvp(None, vp[3, 0].expand(16, 83)))
    assert mpc.trajectory_jvp(vx, vp, U=False)[1] is None and mpc.trajectory_jvp(vx, vp, X=False)[0] is None
    after = [r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian()]
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, after))      # (bytes: instance 5 holds NaN)


def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, chain_mass_ocp, linear_system_ocp
    lin = MPCBatch(linear_system_ocp(N=7), 3)
    x0 = np.array([[0.5, 0.1], [0.3, 0.2], [0.6, -0.1]])
    vx, vp = dev(lin, np.ones((3, 2, 2))), dev(lin, np.ones((3, 2, 12)))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, vx, vp)                                     # before any solve
    with pytest.raises(RuntimeError):
        lin.trajectory_jvp(vx, vp)
    lin.solve(x0, cold=True, store_bounds=False)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, vx, vp)                                     # the bound planes are placeholders
    with pytest.raises(RuntimeError):
        lin.trajectory_jvp(vx, vp)
    lin.solve(x0, cold=True)
    assert all(torch.isfinite(t).all() for t in raw_jvp(lin, 2, vx, vp))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, None, None)                                 # both directions NULL
    with pytest.raises(ValueError):
        lin.trajectory_jvp(None, None)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, vx, vp, (False, False))                     # both outputs NULL
    with pytest.raises(ValueError):
        lin.trajectory_jvp(vx, vp, X=False, U=False)
    for ndir in (0, -1):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw_jvp(lin, ndir, vx, vp)                              # fewer than one direction
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, vx, vp, flags=_lib.STATE_Q_MODE)            # Q mode is not offered
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, vx, vp, flags=1 << 20)                      # unknown flags
    x, u, pi, _, _ = lin.get_iterate()
    lin.set_iterate(x, u, pi)                                       # without bnd
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_jvp(lin, 2, vx, vp)
    lin.solve(x0, np.full((3, 1), 0.1), cold=True)                  # a solve with u0 fixed
    with pytest.raises(RuntimeError, match="Q mode"):
        lin.trajectory_jvp(vx, vp)
    chain = MPCBatch(chain_mass_ocp(n_mass=3, N=10), 2)
    chain.solve(np.tile(chain.ocp.x0, (2, 1)), cold=True)
    cx, cp = dev(chain, np.ones((2, 1, chain.nx))), dev(chain, np.ones((2, 1, chain.n_p)))
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        raw_jvp(chain, 1, cx, cp)
    with pytest.raises(RuntimeError, match="chain"):
        chain.trajectory_jvp(cx, cp)
    with pytest.raises(RuntimeError, match="chain"):
        chain.trajectory_jacobian()


def test_replays_inside_a_graph(cp16):
    ocp, x0, vx, vp = cp16
    mpc = handle(ocp, 16)
    mpc.solve(np.nan_to_num(x0, nan=0.1), cold=True)
    vx, vp = dev(mpc, vx), dev(mpc, vp)
    want = raw_jvp(mpc, R, vx, vp)
    dX = torch.zeros((16, R, 21, 4), dtype=torch.float64, device=mpc.device)
    dU = torch.zeros((16, R, 20, 1), dtype=torch.float64, device=mpc.device)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node: no parallel branches
        mpc._call("mpcrl_traj_jvp", 0, R, vx, vp, dX, dU)
    torch.cuda.synchronize()
    assert torch.all(dX == 0) and torch.all(dU == 0)      # captured, not run
    for _ in range(2):
        dX.fill_(float("nan")), dU.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same((dX, dU), want)


MEASURED = """\
traj jvp cartpole N 2 B 13: no positive slack (13): du0*/dp 2.9e-09 -> bar 1.0e-06; dX 9.4e-09 4.7e-09 1.5e-08; dU 2.9e-08 9.7e-09 3.0e-08
traj jvp cartpole N 2 B 1: no positive slack (1): du0*/dp 1.9e-10 -> bar 1.0e-06; dX 1.1e-09 5.2e-10 6.0e-10; dU 1.7e-10 3.3e-10 1.6e-10
traj jvp cartpole N 15 B 11: no positive slack (11): du0*/dp 2.4e-08 -> bar 1.0e-06; dX 6.0e-08 2.0e-08 6.6e-08; dU 6.1e-08 1.8e-08 5.6e-08
traj jvp cartpole N 15 B 1: no positive slack (1): du0*/dp 4.0e-10 -> bar 1.0e-06; dX 1.4e-09 8.1e-10 1.5e-09; dU 8.5e-10 3.6e-10 7.6e-10
traj jvp cartpole N 20 B 13: no positive slack (13): du0*/dp 1.9e-08 -> bar 1.0e-06; dX 3.7e-09 9.2e-09 7.2e-09; dU 2.3e-09 4.2e-08 8.1e-09
traj jvp cartpole N 20 B 1: no positive slack (1): du0*/dp 1.9e-08 -> bar 1.0e-06; dX 1.2e-09 4.1e-09 3.5e-09; dU 8.8e-10 1.3e-08 3.0e-09
traj jvp cartpole N 31 B 11: no positive slack (11): du0*/dp 4.8e-08 -> bar 1.0e-06; dX 2.0e-08 2.4e-08 4.1e-08; dU 3.9e-08 3.3e-08 3.8e-08
traj jvp cartpole N 31 B 1: no positive slack (1): du0*/dp 2.0e-08 -> bar 1.0e-06; dX 1.5e-09 4.6e-09 4.1e-09; dU 1.5e-09 1.9e-08 3.5e-09
traj jvp cartpole N 32 B 12: no positive slack (12): du0*/dp 4.0e-08 -> bar 1.0e-06; dX 6.6e-08 3.7e-08 3.6e-08; dU 6.3e-08 6.8e-08 3.6e-08
traj jvp cartpole N 32 B 1: no positive slack (1): du0*/dp 1.0e-10 -> bar 1.0e-06; dX 3.8e-10 2.0e-10 6.2e-10; dU 3.8e-10 2.5e-10 7.9e-10
traj jvp cartpole N 63 B 10: no positive slack (10): du0*/dp 6.5e-08 -> bar 1.0e-06; dX 5.7e-08 6.6e-08 8.1e-08; dU 5.2e-08 6.3e-08 9.8e-08
traj jvp cartpole N 63 B 1: no positive slack (1): du0*/dp 3.3e-09 -> bar 1.0e-06; dX 7.1e-10 1.5e-09 7.9e-10; dU 9.3e-10 2.8e-09 1.2e-09
traj jvp linear N 2 B 25: no positive slack (10): du0*/dp 2.2e-08 -> bar 1.0e-06; dX 6.0e-08 3.8e-08 3.2e-08; dU 4.7e-08 5.9e-08 3.0e-08
traj jvp linear N 2 B 1: no positive slack (1): du0*/dp 5.1e-09 -> bar 1.0e-06; dX 5.3e-09 4.0e-09 1.8e-09; dU 6.0e-09 1.2e-08 2.4e-09
traj jvp linear N 7 B 24: no positive slack (9): du0*/dp 2.4e-08 -> bar 1.0e-06; dX 4.0e-08 3.8e-08 1.4e-08; dU 2.6e-08 4.6e-08 2.5e-08
traj jvp linear N 7 B 1: no positive slack (1): du0*/dp 1.6e-08 -> bar 1.0e-06; dX 1.5e-08 1.5e-08 3.9e-09; dU 6.2e-09 2.0e-08 6.3e-09
traj jvp linear N 20 B 17: no positive slack (3): du0*/dp 1.3e-08 -> bar 1.0e-06; dX 5.0e-09 7.4e-09 2.0e-09; dU 9.7e-09 7.3e-09 6.0e-09
traj jvp linear N 20 B 1: no positive slack (1): du0*/dp 3.2e-09 -> bar 1.0e-06; dX 5.0e-09 7.4e-09 1.3e-09; dU 9.7e-09 7.3e-09 2.2e-09
traj jvp linear N 31 B 15: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; dX 0.0e+00 0.0e+00 0.0e+00; dU 0.0e+00 0.0e+00 0.0e+00
traj jvp linear N 31 B 1: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; dX 0.0e+00 0.0e+00 0.0e+00; dU 0.0e+00 0.0e+00 0.0e+00
traj jvp linear N 32 B 13: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; dX 0.0e+00 0.0e+00 0.0e+00; dU 0.0e+00 0.0e+00 0.0e+00
traj jvp linear N 32 B 1: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; dX 0.0e+00 0.0e+00 0.0e+00; dU 0.0e+00 0.0e+00 0.0e+00
traj jvp linear N 63 B 15: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; dX 0.0e+00 0.0e+00 0.0e+00; dU 0.0e+00 0.0e+00 0.0e+00
traj jvp linear N 63 B 1: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; dX 0.0e+00 0.0e+00 0.0e+00; dU 0.0e+00 0.0e+00 0.0e+00
traj jvp cartpole per-instance theta (2): du0*/dp 2.0e-08 -> bar 1.0e-06; dX 2.6e-09 4.0e-09 5.6e-09; dU 2.2e-09 9.6e-09 4.5e-09
traj jvp linear per-instance theta (2): du0*/dp 4.2e-09 -> bar 1.0e-06; dX 6.2e-09 4.6e-09 1.7e-09; dU 1.0e-08 9.7e-09 3.2e-09
traj jvp cartpole N 2 adjoint identity: 5.3e-15 (largest product 1.3e+02)
traj jvp cartpole N 15 adjoint identity: 2.8e-09 (largest product 9.1e+02)
traj jvp cartpole N 20 adjoint identity: 9.1e-10 (largest product 6.0e+02)
traj jvp cartpole N 31 adjoint identity: 7.5e-14 (largest product 2.0e+03)
traj jvp cartpole N 32 adjoint identity: 6.5e-13 (largest product 6.2e+02)
traj jvp cartpole N 63 adjoint identity: 6.2e-13 (largest product 1.4e+03)
traj jvp linear N 2 adjoint identity: 2.7e-15 (largest product 2.4e+01)
traj jvp linear N 7 adjoint identity: 6.9e-15 (largest product 1.4e+02)
traj jvp linear N 20 adjoint identity: 3.9e-08 (largest product 3.9e+02)
traj jvp linear N 31 adjoint identity: 1.5e-09 (largest product 2.1e+02)
traj jvp linear N 32 adjoint identity: 9.1e-09 (largest product 1.7e+02)
traj jvp linear N 63 adjoint identity: 2.3e-09 (largest product 3.4e+02)
traj jvp cartpole N 2 unit directions inside the library: dU_dtheta[0] against du0*/dp 7.4e-16; dU_dx0[0] against du0*/dx0 3.1e-16
traj jvp cartpole N 15 unit directions inside the library: dU_dtheta[0] against du0*/dp 4.7e-15; dU_dx0[0] against du0*/dx0 3.6e-15
traj jvp cartpole N 20 unit directions inside the library: dU_dtheta[0] against du0*/dp 4.2e-12; dU_dx0[0] against du0*/dx0 1.6e-10
traj jvp cartpole N 31 unit directions inside the library: dU_dtheta[0] against du0*/dp 1.8e-14; dU_dx0[0] against du0*/dx0 1.1e-14
traj jvp cartpole N 32 unit directions inside the library: dU_dtheta[0] against du0*/dp 5.7e-15; dU_dx0[0] against du0*/dx0 1.2e-14
traj jvp cartpole N 63 unit directions inside the library: dU_dtheta[0] against du0*/dp 3.2e-14; dU_dx0[0] against du0*/dx0 6.4e-14
traj jvp linear N 2 unit directions inside the library: dU_dtheta[0] against du0*/dp 3.0e-16; dU_dx0[0] against du0*/dx0 3.0e-16
traj jvp linear N 7 unit directions inside the library: dU_dtheta[0] against du0*/dp 4.1e-16; dU_dx0[0] against du0*/dx0 2.2e-16
traj jvp linear N 20 unit directions inside the library: dU_dtheta[0] against du0*/dp 4.1e-16; dU_dx0[0] against du0*/dx0 2.1e-16
traj jvp linear N 31 unit directions inside the library: dU_dtheta[0] against du0*/dp 5.1e-16; dU_dx0[0] against du0*/dx0 2.1e-16
traj jvp linear N 32 unit directions inside the library: dU_dtheta[0] against du0*/dp 2.4e-16; dU_dx0[0] against du0*/dx0 5.3e-17
traj jvp linear N 63 unit directions inside the library: dU_dtheta[0] against du0*/dp 3.8e-16; dU_dx0[0] against du0*/dx0 2.2e-16
"""
