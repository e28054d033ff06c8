"""mpcrl_traj_vjp (include/mpcrl_traj_ext.h) on the device: the vector-Jacobian product of the whole planned trajectory from
small_traj_vjp_kernel against the mirror fixture G11 (tests/golden/make_traj_vjp.py), against the library's own du0*/dp and du0*/dx0
for the unit cotangent on u_0, the call's contract, the same bits under every launch shape, and MPCLayer.trajectory on top.

Bars.  Against the fixture: max(1e-6, 4 x the error of the solve's own du0*/dp against G9's mirror du0*/dp on the same instances) —
another right-hand side of the same factorisation, the bar of tests/test_gpu_state_sens.py; 1e-6 is RTOL of tests/small_mode_cases.py.
Asserted on the instances without a positive slack (with one the mirror holds the slacks constant and is the definition, not a
yardstick).  Rows are scaled by max(|reference row|, 1).  Inside the library (unit cotangent against sens_pi / state_sens): 1e-6.
The layer against central differences of its own forward pass at h = 1e-5: 1e-5, the bar of the existing layer test.

Measured on an MI355X: MEASURED at the end of this file (every line the tests print).
"""
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
def g9():
    return np.load(os.path.join(GOLD, "g9_state_sens.npz"))


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(GOLD, "g11_traj_vjp.npz"))


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
    return all((x is None and y is None) or torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def split(mpc, G):
    """(gX [B, N+1, nx], gU [B, N, nu]) of cotangents [B, nw] in the mirror's order w = [u_0 .. u_{N-1}; x_0 .. x_N]."""
    G = torch.as_tensor(G, dtype=torch.float64, device=mpc.device)
    n = mpc.N * mpc.nu
    return G[:, n:].reshape(mpc.B, mpc.N + 1, mpc.nx).contiguous(), G[:, :n].reshape(mpc.B, mpc.N, mpc.nu).contiguous()


def raw_vjp(mpc, gX, gU, want=(True, True), flags=0, fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    bufs = [torch.full(sh, fill, **kw) if w else None for sh, w in zip(((mpc.B, mpc.nx), (mpc.B, mpc.n_p)), want)]
    mpc._call("mpcrl_traj_vjp", flags, gX, gU, *bufs)
    torch.cuda.synchronize()
    return bufs


# ---------------------------------------------------------------------- 1. against the fixture
def fixture_case(g9, g11, key, ocp, rows, theta=None):
    """Cold solve at tol 1e-9 on the fixture's x0, then one trajectory_vjp per cotangent.  Returns (bar, error of the solve's own
    du0*/dp, errors of g_theta and g_x0 over the cotangents, number of asserted instances)."""
    idx = g11[key + "idx"][rows]
    x0 = g11[key + "x0"][rows]
    mpc = handle(ocp, len(x0))
    if theta is not None:
        mpc.set_theta(theta[rows])
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
    firm = ~g11[key + "soft"][rows] if key + "soft" in g11.files else np.ones(len(x0), bool)
    got_t, got_x = [], []
    for c in range(3):
        gX, gU = split(mpc, g11[key + "G"][rows][:, c])
        g_x0, g_th = mpc.trajectory_vjp(gX, gU)
        got_t.append(g_th.cpu().numpy()), got_x.append(g_x0.cpu().numpy())
    if not firm.any():
        return RTOL, 0.0, [0.0] * 3, [0.0] * 3, 0
    ref_dp = g9[key + "dpi_dp"][idx].copy()
    if key + "cls" in g9.files:
        ref_dp[g9[key + "cls"][idx] == 2] = 0.0      # u_0 on its bound: the exact zero, as tests/test_gpu_state_sens.py takes it
    err_dp = scaled(r.dpi_dp.cpu().numpy()[firm], ref_dp[firm])
    e_t = [scaled(got_t[c][firm], g11[key + "g_theta"][rows][firm, c]) for c in range(3)]
    e_x = [scaled(got_x[c][firm], g11[key + "g_x0"][rows][firm, c]) for c in range(3)]
    return max(RTOL, 4.0 * err_dp), err_dp, e_t, e_x, int(firm.sum())


def fmt(e):
    return " ".join(f"{v:.1e}" for v in e)


@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]])
def test_trajectory_vjp_against_the_mirror(g9, g11, model, N):
    """Every instance of the fixture, then its first instance alone (B = 1); three cotangents each (two random over all of w, the
    unit vector on u_0).  Asserted on the instances without a positive slack; at linear N 31, 32 and 63 the fixture has none
    (tests/golden/make_traj_vjp.py says why) and the case only runs the call: those lane layouts are held to numbers by the unit
    cotangent below and by test_long_linear_horizons_against_differences_without_an_active_bound.  MEASURED on an MI355X at the end
    of this file."""
    ocp, _ = C.problem(model, N)
    key = f"{model}_N{N}_"
    for rows in (slice(None), slice(0, 1)):
        bar, err_dp, e_t, e_x, n = fixture_case(g9, g11, key, ocp, rows)
        print(f"traj vjp {model} N {N} B {len(g11[key + 'idx'][rows])}: no positive slack ({n}): du0*/dp {err_dp:.1e} -> bar {bar:.1e}; "
              f"g_theta {fmt(e_t)}; g_x0 {fmt(e_x)}")
        assert max(e_t) <= bar and max(e_x) <= bar, (model, N, bar, e_t, e_x)


@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_per_instance_theta_against_the_mirror(g9, g11, model):
    ocp, _ = C.problem(model, 20)
    key = f"{model}_th_"
    bar, err_dp, e_t, e_x, n = fixture_case(g9, g11, key, ocp, slice(None), theta=g11[key + "theta"])
    print(f"traj vjp {model} per-instance theta ({n}): du0*/dp {err_dp:.1e} -> bar {bar:.1e}; g_theta {fmt(e_t)}; g_x0 {fmt(e_x)}")
    assert n >= 2 and max(e_t) <= bar and max(e_x) <= bar


# ---------------------------------------------------------------------- 2. consistency inside the library
@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]])
def test_unit_cotangent_is_the_first_move_jacobian(g11, model, N):
    """G = e_{u_0}: g_theta against du0*/dp of the same solve run with sens_pi, g_x0 against du0*/dx0 of state_sens — one
    factorisation, one right-hand side, three kernels; every instance of the fixture, positive slacks included.  Then a cotangent on
    x_0 alone: nothing to solve for, g_x0 is that cotangent bit for bit and g_theta is exactly zero."""
    ocp, _ = C.problem(model, N)
    key = f"{model}_N{N}_"
    x0 = g11[key + "x0"]
    mpc = handle(ocp, len(x0))
    r = mpc.solve(x0, sens_pi=True, cold=True)
    s = mpc.state_sens(value=False)
    assert r.status.tolist() == [0] * len(x0)
    gU = torch.zeros((mpc.B, mpc.N, mpc.nu), dtype=torch.float64, device=mpc.device)
    gU[:, 0, 0] = 1.0
    g_x0, g_th = mpc.trajectory_vjp(None, gU)
    e_t, e_x = scaled(g_th, r.dpi_dp[:, 0].cpu().numpy()), scaled(g_x0, s.dpi_dx0[:, 0].cpu().numpy())
    print(f"traj vjp {model} N {N} unit cotangent inside the library: g_theta against du0*/dp {e_t:.1e}; g_x0 against du0*/dx0 {e_x:.1e}")
    assert e_t <= RTOL and e_x <= RTOL
    gX = torch.zeros((mpc.B, mpc.N + 1, mpc.nx), dtype=torch.float64, device=mpc.device)
    gX[:, 0] = torch.tensor(np.random.default_rng(5).standard_normal((mpc.B, mpc.nx)), device=mpc.device)
    g_x0, g_th = mpc.trajectory_vjp(gX, None)
    assert same((g_x0,), (gX[:, 0].contiguous(),)) and torch.all(g_th == 0)


# ---------------------------------------------------------------------- 3. contract
@pytest.fixture(scope="module")
def cp16():
    """cartpole N 20, B 16: x0 of tests/test_gpu_state_sens.py with instance 5 made NaN, and one cotangent over all of w."""
    ocp, _ = C.problem("cartpole", 20)
    rng = np.random.default_rng(41)
    x0 = rng.uniform(-1, 1, (16, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    x0[5, 2] = float("nan")
    return ocp, x0, rng.standard_normal((16, 20 * 1 + 21 * 4))


def test_every_requested_row_is_written_and_failed_instances_are_zero(cp16):
    ocp, x0, G = cp16
    mpc = handle(ocp, 16)
    r = mpc.solve(x0, cold=True)
    gX, gU = split(mpc, G)
    before = [t.clone() for t in (r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian())]
    g_x0, g_th = raw_vjp(mpc, gX, gU)
    st = r.status.cpu().numpy()
    assert st[5] == 1 and np.all(np.delete(st, 5) == 0)
    assert torch.isfinite(g_x0).all() and torch.isfinite(g_th).all()
    assert torch.all(g_x0[5] == 0) and torch.all(g_th[5] == 0) and torch.all(g_x0[4].abs() > 0) and torch.all(g_th[4, :3].abs() > 0)
    assert torch.all(g_th[:, 3:] == 0)      # the cartpole's W, yref block: no gradient, the convention of dpi_dp
    only_x, only_t = raw_vjp(mpc, gX, gU, (True, False)), raw_vjp(mpc, gX, gU, (False, True))
    assert only_x[1] is None and only_t[0] is None and same((only_x[0], only_t[1]), (g_x0, g_th))
    for a, b in ((gX, None), (None, gU)):      # a NULL cotangent counts as zeros
        za, zb = (torch.zeros_like(gX) if a is None else a), (torch.zeros_like(gU) if b is None else b)
        assert same(raw_vjp(mpc, a, b), raw_vjp(mpc, za, zb))
    p = mpc.trajectory_vjp(gX, gU)      # the Python surface: the same numbers, rows selected by the status it holds
    assert same(p, (g_x0, g_th))
    after = [r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian()]
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, after))      # (bytes: instance 5 holds NaN)


def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, chain_mass_ocp, linear_system_ocp
    lin = MPCBatch(linear_system_ocp(N=7), 3)
    x0 = np.array([[0.5, 0.1], [0.3, 0.2], [0.6, -0.1]])
    gX, gU = split(lin, np.ones((3, 7 + 8 * 2)))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU)                                        # before any solve
    with pytest.raises(RuntimeError):
        lin.trajectory_vjp(gX, gU)
    lin.solve(x0, cold=True, store_bounds=False)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU)                                        # the bound planes are placeholders
    with pytest.raises(RuntimeError):
        lin.trajectory_vjp(gX, gU)
    lin.solve(x0, cold=True)
    assert all(torch.isfinite(t).all() for t in raw_vjp(lin, gX, gU))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, None, None)                                    # both cotangents NULL
    with pytest.raises(ValueError):
        lin.trajectory_vjp(None, None)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU, (False, False))                        # both outputs NULL
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU, flags=_lib.STATE_Q_MODE)               # Q mode is not offered
    x, u, pi, _, _ = lin.get_iterate()
    lin.set_iterate(x, u, pi)                                       # without bnd
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(lin, gX, gU)
    lin.solve(x0, np.full((3, 1), 0.1), cold=True)                  # a solve with u0 fixed
    with pytest.raises(RuntimeError, match="Q mode"):
        lin.trajectory_vjp(gX, gU)
    chain = MPCBatch(chain_mass_ocp(n_mass=3, N=10), 2)
    chain.solve(np.tile(chain.ocp.x0, (2, 1)), cold=True)
    cX, cU = split(chain, np.ones((2, 10 * chain.nu + 11 * chain.nx)))
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        raw_vjp(chain, cX, cU)
    with pytest.raises(RuntimeError, match="chain"):
        chain.trajectory_vjp(cX, cU)


# ---------------------------------------------------------------------- 4. the same bits
def test_same_bits_whatever_the_order_and_the_launch_shape(cp16):
    """An explicit reversed packing order, the time-sliced against the plain solve launch, and a second call: the same bits."""
    ocp, x0, G = cp16
    x0 = np.nan_to_num(x0, nan=0.1)
    ref = None
    for mode, perm in ((-1, None), (1, None), (-1, torch.arange(15, -1, -1))):
        mpc = handle(ocp, 16)
        mpc.set_launch_mode(mode)
        mpc.set_order(perm)
        mpc.solve(x0, cold=True, reorder=False)
        gX, gU = split(mpc, G)
        a, b = raw_vjp(mpc, gX, gU), raw_vjp(mpc, gX, gU)
        assert same(a, b)
        ref = a if ref is None else ref
        assert same(a, ref), (mode, perm is not None)
    assert torch.isfinite(ref[0]).all() and torch.all(ref[0].abs() > 0)


def test_replays_inside_a_graph(cp16):
    ocp, x0, G = cp16
    mpc = handle(ocp, 16)
    mpc.solve(np.nan_to_num(x0, nan=0.1), cold=True)
    gX, gU = split(mpc, G)
    want = raw_vjp(mpc, gX, gU)
    g_x0 = torch.zeros((16, 4), dtype=torch.float64, device=mpc.device)
    g_th = torch.zeros((16, mpc.n_p), dtype=torch.float64, device=mpc.device)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node: no parallel branches
        mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th)
    torch.cuda.synchronize()
    assert torch.all(g_x0 == 0) and torch.all(g_th == 0)      # captured, not run
    for _ in range(2):
        g_x0.fill_(float("nan")), g_th.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same((g_x0, g_th), want)


# ---------------------------------------------------------------------- 5. the layer
def layer_differences(f, z, h=1e-5):
    """d f(z) / d z of a scalar f by central differences, entry by entry (z a float64 tensor on the device)."""
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


def layer_inputs(model, N, B, seed):
    ocp, _ = C.problem(model, N)
    rng = np.random.default_rng(seed)
    if model == "linear":
        x0 = np.column_stack([rng.uniform(0.2, 0.8, B), rng.uniform(-0.2, 0.3, B)])
    else:
        x0 = rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    Wx = torch.tensor(rng.uniform(-1, 1, (B, N + 1, ocp.nx)), device="cuda")
    Wu = torch.tensor(rng.uniform(-1, 1, (B, N, ocp.nu)), device="cuda")
    return ocp, x0, Wx, Wu


@pytest.mark.parametrize("model,N,B", [("linear", 8, 3), ("cartpole", 6, 2)])
def test_layer_trajectory_gradients_against_differences_of_its_forward_pass(model, N, B):
    from mpc4rl_amd import MPCLayer
    ocp, x0, Wx, Wu = layer_inputs(model, N, B, 21)
    layer = MPCLayer(handle(ocp, B, tol=1e-10), cold=True)
    x0 = torch.tensor(x0, device="cuda", requires_grad=True)
    theta = torch.tensor(ocp.p0, device="cuda", requires_grad=model == "linear")

    def loss(x, th):
        X, U = layer.trajectory(x, th)
        return (Wx * X).sum() + (Wu * U).sum()

    loss(x0, theta).backward()
    assert layer.last_status.tolist() == [0] * B
    with torch.no_grad():
        gx = layer_differences(lambda z: float(loss(z, theta.detach())), x0.detach().clone())
        e_x = scaled(x0.grad, gx.cpu().numpy())
        e_t = 0.0
        if model == "linear":      # shared theta: the gradient is the sum over the batch
            gt = layer_differences(lambda z: float(loss(x0.detach(), z)), theta.detach().clone())
            e_t = scaled(theta.grad[None], gt.cpu().numpy()[None])
    print(f"layer.trajectory {model} N {N}: d loss/d x0 {e_x:.1e}; d loss/d theta {e_t:.1e}")
    assert float(x0.grad.abs().max()) > 0 and e_x <= 1e-5 and e_t <= 1e-5


@pytest.mark.parametrize("N", [31, 32, 63])
def test_long_linear_horizons_against_differences_without_an_active_bound(N):
    """The horizons at which G11 has no instance to assert on (the plan converges onto the softened bound lbx = 0, where differences
    straddle a kink): the same layer check with every bound moved to +-100, where the plan is smooth in x0 and theta — random weights
    on all of (X, U), so every stage lane carries a right-hand side, on the lane layouts of 32, 33 and 64 lanes per instance.
    Bar 1e-5 as above: solves at tol 1e-10 differenced over 2 h = 2e-5 carry at most 5e-6, the truncation term is O(h^2)."""
    from mpc4rl_amd import MPCLayer, _lib
    ocp, x0, Wx, Wu = layer_inputs("linear", N, 2, 30 + N)
    mpc = handle(ocp, 2, tol=1e-10)
    mpc.set_bounds(_lib.BOUNDS_U0, [-100.0], [100.0])
    mpc.set_bounds(_lib.BOUNDS_STAGE, [-100.0] * 3, [100.0] * 3)
    layer = MPCLayer(mpc, cold=True)
    x0 = torch.tensor(x0, device="cuda", requires_grad=True)
    theta = torch.tensor(ocp.p0, device="cuda", requires_grad=True)

    def loss(x, th):
        X, U = layer.trajectory(x, th)
        return (Wx * X).sum() + (Wu * U).sum()

    loss(x0, theta).backward()
    assert layer.last_status.tolist() == [0, 0]
    with torch.no_grad():
        e_x = scaled(x0.grad, layer_differences(lambda z: float(loss(z, theta.detach())), x0.detach().clone()).cpu().numpy())
        gt = layer_differences(lambda z: float(loss(x0.detach(), z)), theta.detach().clone())
        e_t = scaled(theta.grad[None], gt.cpu().numpy()[None])
    print(f"layer.trajectory linear N {N}, bounds at +-100: d loss/d x0 {e_x:.1e}; d loss/d theta {e_t:.1e}")
    assert float(x0.grad.abs().max()) > 0 and float(theta.grad.abs().max()) > 0 and e_x <= 1e-5 and e_t <= 1e-5


def test_layer_trajectory_staleness_failed_instance_and_an_encoder_in_front():
    from mpc4rl_amd import MPCLayer
    ocp, x0n, Wx, Wu = layer_inputs("linear", 8, 3, 22)
    layer = MPCLayer(handle(ocp, 3, tol=1e-10), cold=True)
    x0 = torch.tensor(x0n, device="cuda", requires_grad=True)
    theta = torch.tensor(ocp.p0, device="cuda", requires_grad=True)
    X, U = layer.trajectory(x0, theta)
    layer(x0.detach(), theta.detach())                             # the handle now holds another pass's iterate
    with pytest.raises(RuntimeError, match="one backward per forward"):
        ((Wx * X).sum() + (Wu * U).sum()).backward()
    # an observation encoder upstream of x0 (float32, as a network would be): a finite, non-zero gradient reaches its weights
    enc = torch.nn.Linear(5, 2).cuda()
    obs = torch.tensor(np.random.default_rng(23).uniform(-1, 1, (3, 5)), dtype=torch.float32, device="cuda")
    X, U = layer.trajectory(0.1 * torch.tanh(enc(obs)) + torch.tensor([0.5, 0.0], device="cuda"), torch.tensor(ocp.p0, device="cuda"))
    assert X.dtype == torch.float32 and U.dtype == torch.float32
    ((Wx * X).sum() + (Wu * U).sum()).backward()
    assert layer.last_status.tolist() == [0] * 3
    for p in enc.parameters():
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0
    # an instance whose solve failed contributes exactly zero
    ocp, _, Wx, Wu = layer_inputs("cartpole", 6, 2, 24)
    layer = MPCLayer(handle(ocp, 2), cold=True)
    x0 = torch.tensor([[0.1, 0.0, 0.1, 0.0], [0.1, 0.0, float("nan"), 0.0]], device="cuda", requires_grad=True)
    theta = torch.tensor(np.tile(ocp.p0, (2, 1)), device="cuda", requires_grad=True)
    X, U = layer.trajectory(x0, theta)
    ((Wx * torch.nan_to_num(X)).sum() + (Wu * torch.nan_to_num(U)).sum()).backward()
    assert layer.last_status.tolist() == [0, 1]
    assert torch.isfinite(x0.grad).all() and torch.isfinite(theta.grad).all()
    assert torch.all(x0.grad[1] == 0) and torch.all(theta.grad[1] == 0) and torch.all(x0.grad[0] != 0) and torch.all(theta.grad[0, :3] != 0)


MEASURED = """\
traj vjp cartpole N 2 B 13: no positive slack (13): du0*/dp 2.9e-09 -> bar 1.0e-06; g_theta 6.1e-09 6.3e-09 8.5e-08; g_x0 3.1e-08 1.7e-08 4.3e-08
traj vjp cartpole N 2 B 1: no positive slack (1): du0*/dp 1.9e-10 -> bar 1.0e-06; g_theta 2.3e-10 2.7e-10 1.9e-10; g_x0 2.6e-10 3.3e-10 3.2e-10
traj vjp cartpole N 15 B 12: no positive slack (12): du0*/dp 3.1e-08 -> bar 1.0e-06; g_theta 8.6e-08 3.4e-08 3.1e-08; g_x0 4.0e-08 7.2e-08 1.5e-08
traj vjp cartpole N 15 B 1: no positive slack (1): du0*/dp 4.0e-10 -> bar 1.0e-06; g_theta 3.0e-10 4.9e-10 4.0e-10; g_x0 4.1e-10 6.2e-10 3.9e-10
traj vjp cartpole N 20 B 13: no positive slack (13): du0*/dp 1.9e-08 -> bar 1.0e-06; g_theta 2.1e-08 2.4e-08 1.9e-08; g_x0 6.9e-09 7.1e-09 1.4e-08
traj vjp cartpole N 20 B 1: no positive slack (1): du0*/dp 1.9e-08 -> bar 1.0e-06; g_theta 4.3e-09 1.7e-08 1.9e-08; g_x0 4.4e-09 3.7e-09 3.6e-09
traj vjp cartpole N 31 B 11: no positive slack (11): du0*/dp 4.8e-08 -> bar 1.0e-06; g_theta 2.2e-08 2.1e-08 4.8e-08; g_x0 1.1e-08 2.0e-08 1.0e-08
traj vjp cartpole N 31 B 1: no positive slack (1): du0*/dp 2.0e-08 -> bar 1.0e-06; g_theta 1.1e-08 3.9e-09 2.0e-08; g_x0 2.2e-09 2.8e-09 2.4e-09
traj vjp cartpole N 32 B 12: no positive slack (12): du0*/dp 4.0e-08 -> bar 1.0e-06; g_theta 4.9e-08 5.4e-08 4.0e-08; g_x0 4.6e-08 4.4e-08 4.2e-08
traj vjp cartpole N 32 B 1: no positive slack (1): du0*/dp 1.0e-10 -> bar 1.0e-06; g_theta 4.8e-10 4.1e-10 1.0e-10; g_x0 9.3e-10 8.5e-10 1.7e-09
traj vjp cartpole N 63 B 10: no positive slack (10): du0*/dp 6.5e-08 -> bar 1.0e-06; g_theta 6.6e-08 2.2e-08 6.5e-08; g_x0 4.7e-08 4.3e-08 4.4e-08
traj vjp cartpole N 63 B 1: no positive slack (1): du0*/dp 3.3e-09 -> bar 1.0e-06; g_theta 2.4e-09 1.6e-09 3.3e-09; g_x0 4.8e-10 1.0e-09 7.3e-10
traj vjp linear N 2 B 25: no positive slack (10): du0*/dp 2.2e-08 -> bar 1.0e-06; g_theta 3.6e-08 2.6e-08 2.2e-08; g_x0 2.9e-08 3.4e-08 2.1e-08
traj vjp linear N 2 B 1: no positive slack (1): du0*/dp 5.1e-09 -> bar 1.0e-06; g_theta 3.8e-09 3.0e-09 5.1e-09; g_x0 2.3e-09 1.4e-09 2.7e-09
traj vjp linear N 7 B 24: no positive slack (9): du0*/dp 2.4e-08 -> bar 1.0e-06; g_theta 3.2e-08 3.8e-08 2.4e-08; g_x0 1.4e-08 1.5e-08 2.2e-08
traj vjp linear N 7 B 1: no positive slack (1): du0*/dp 1.6e-08 -> bar 1.0e-06; g_theta 3.2e-08 1.7e-08 1.6e-08; g_x0 1.4e-08 1.3e-08 1.2e-08
traj vjp linear N 20 B 19: no positive slack (5): du0*/dp 3.2e-08 -> bar 1.0e-06; g_theta 2.2e-08 7.0e-09 3.2e-08; g_x0 2.9e-08 1.2e-08 3.2e-08
traj vjp linear N 20 B 1: no positive slack (1): du0*/dp 3.2e-09 -> bar 1.0e-06; g_theta 3.1e-09 8.0e-10 3.2e-09; g_x0 1.5e-09 2.2e-09 3.0e-09
traj vjp linear N 31 B 15: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; g_theta 0.0e+00 0.0e+00 0.0e+00; g_x0 0.0e+00 0.0e+00 0.0e+00
traj vjp linear N 31 B 1: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; g_theta 0.0e+00 0.0e+00 0.0e+00; g_x0 0.0e+00 0.0e+00 0.0e+00
traj vjp linear N 32 B 13: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; g_theta 0.0e+00 0.0e+00 0.0e+00; g_x0 0.0e+00 0.0e+00 0.0e+00
traj vjp linear N 32 B 1: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; g_theta 0.0e+00 0.0e+00 0.0e+00; g_x0 0.0e+00 0.0e+00 0.0e+00
traj vjp linear N 63 B 15: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; g_theta 0.0e+00 0.0e+00 0.0e+00; g_x0 0.0e+00 0.0e+00 0.0e+00
traj vjp linear N 63 B 1: no positive slack (0): du0*/dp 0.0e+00 -> bar 1.0e-06; g_theta 0.0e+00 0.0e+00 0.0e+00; g_x0 0.0e+00 0.0e+00 0.0e+00
traj vjp cartpole per-instance theta (2): du0*/dp 2.0e-08 -> bar 1.0e-06; g_theta 8.4e-09 3.6e-09 2.0e-08; g_x0 5.0e-09 4.3e-09 3.6e-09
traj vjp linear per-instance theta (2): du0*/dp 4.2e-09 -> bar 1.0e-06; g_theta 5.6e-10 6.6e-09 4.2e-09; g_x0 1.9e-09 2.8e-09 3.8e-09
traj vjp cartpole N 2 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp cartpole N 15 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp cartpole N 20 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp cartpole N 31 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp cartpole N 32 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp cartpole N 63 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp linear N 2 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp linear N 7 unit cotangent inside the library: g_theta against du0*/dp 0.0e+00; g_x0 against du0*/dx0 0.0e+00
traj vjp linear N 20 unit cotangent inside the library: g_theta against du0*/dp 2.4e-16; g_x0 against du0*/dx0 0.0e+00
traj vjp linear N 31 unit cotangent inside the library: g_theta against du0*/dp 5.1e-16; g_x0 against du0*/dx0 0.0e+00
traj vjp linear N 32 unit cotangent inside the library: g_theta against du0*/dp 2.4e-16; g_x0 against du0*/dx0 0.0e+00
traj vjp linear N 63 unit cotangent inside the library: g_theta against du0*/dp 3.7e-16; g_x0 against du0*/dx0 0.0e+00
layer.trajectory linear N 8: d loss/d x0 5.2e-11; d loss/d theta 1.4e-10
layer.trajectory cartpole N 6: d loss/d x0 2.6e-11; d loss/d theta 0.0e+00
layer.trajectory linear N 31, bounds at +-100: d loss/d x0 3.7e-11; d loss/d theta 1.4e-10
layer.trajectory linear N 32, bounds at +-100: d loss/d x0 6.9e-11; d loss/d theta 4.0e-11
layer.trajectory linear N 63, bounds at +-100: d loss/d x0 2.9e-11; d loss/d theta 2.0e-10
"""
