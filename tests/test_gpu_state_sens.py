"""mpcrl_state_sens (include/mpcrl_ext.h) on the device: du0*/dx0 of small_state_sens_kernel against the mirror fixture G9
(tests/golden/make_state_sens.py), dV/dx0 / dQ/dx0 / dQ/du0 of stage0_grad_kernel against the fixture and, for all three models,
against the oracle's own expression at the product's iterate, the closed form of the unconstrained linear system, the call's
contract, and the autograd layer on top.

Bars.  du0*/dx0 against the fixture: max(1e-6, 4 x the error of the solve's own du0*/dp against the fixture's mirror du0*/dp on the
same instances) — two right-hand sides of one factorisation, four for the nx columns; 1e-6 is RTOL of tests/small_mode_cases.py.
dV/dx0, dQ/dx0, dQ/du0 against the fixture: 1e-6.  Rows are scaled by max(|reference row|, 1).  Where u_0 sits on its bound the
reference of both Jacobians is the exact zero (the mirror's dense solve carries noise there).  Against the oracle's expression at
the pulled iterate: 1e-10.  The layer against central differences of its own forward pass at h = 1e-5: 1e-5.

Measured on an MI355X.  Against the fixture: MEASURED_POLICY at the end of this file (every line the first test prints).  Stage-0
gradients at the product's iterate, all eight cases: at most 3.9e-16 (rounding level, below 1e-12).  Closed form: du0*/dx0 2.2e-16,
dV/dx0 3.6e-15.  Layer against differences: linear N 8 3.6e-10 (x0), 5.0e-10 (shared theta); cartpole N 6 4.9e-11 (x0); layer.q
8.0e-11 (u0), 3.7e-10 (x0), 9.2e-10 (per-instance theta).
"""
import json
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


def parts(s):
    return (s.dV_dx0, s.dQ_du0, s.dpi_dx0)


# ---------------------------------------------------------------------- 1. kernel B (and A) against the fixture
def fixture_solve(g9, key, ocp, rows=slice(None), theta=None, u0=None):
    x0 = g9[key + "x0"][rows]
    mpc = handle(ocp, len(x0))
    if theta is not None:
        mpc.set_theta(theta)
    r = mpc.solve(x0, u0, sens_v=True, sens_pi=True, cold=True)
    s = mpc.state_sens(q_mode=u0 is not None)
    torch.cuda.synchronize()
    assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
    return r, s


def policy_errors(g9, key, r, s, rows=slice(None), pick=None):
    """(bar, error of the solve's du0*/dp, error of du0*/dx0) against the fixture on the instances ``pick`` (None = all)."""
    ref = g9[key + "dpi_dp"][rows].copy()
    if key + "cls" in g9.files:
        ref[g9[key + "cls"][rows] == 2] = 0.0
    pick = np.ones(len(ref), bool) if pick is None else pick
    if not pick.any():
        return RTOL, 0.0, 0.0
    err = scaled(r.dpi_dp.cpu().numpy()[pick], ref[pick])
    return max(RTOL, 4.0 * err), err, scaled(s.dpi_dx0.cpu().numpy()[pick], g9[key + "dpi_dx0"][rows][pick])


@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]])
def test_policy_and_value_jacobians_against_the_mirror(g9, model, N):
    """Cold solve at tol 1e-9 on the fixture's x0, every instance of the fixture, then the same for its first instance alone (B = 1).
    The bar of the module's docstring holds over all instances, and once more over those without a positive slack alone: with a
    positive slack (linear system) the solve's own du0*/dp is O(1) away from the mirror's dense solve, which makes the bar over all
    instances vacuous there.  MEASURED on an MI355X, see MEASURED_POLICY at the end of this file."""
    ocp, _ = C.problem(model, N)
    key = f"{model}_N{N}_"
    for rows in (slice(None), slice(0, 1)):
        r, s = fixture_solve(g9, key, ocp, rows)
        firm = ~g9[key + "soft"][rows]
        bar, err_dp, e_pi = policy_errors(g9, key, r, s, rows)
        bar_f, err_dp_f, e_pi_f = policy_errors(g9, key, r, s, rows, firm)
        e_v = scaled(s.dV_dx0, g9[key + "dV_dx0"][rows])
        print(f"state sens {model} N {N} B {len(firm)}: all: du0*/dp {err_dp:.1e} -> bar {bar:.1e}, du0*/dx0 {e_pi:.1e}; no positive slack "
              f"({int(firm.sum())}): du0*/dp {err_dp_f:.1e} -> bar {bar_f:.1e}, du0*/dx0 {e_pi_f:.1e}; dV/dx0 {e_v:.1e}")
        assert s.dQ_du0 is None and e_pi <= bar and e_pi_f <= bar_f and e_v <= RTOL, (model, N, err_dp, bar, e_pi, err_dp_f, bar_f, e_pi_f, e_v)


@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_q_mode_against_the_mirror(g9, model):
    ocp, _ = C.problem(model, 20)
    key = f"{model}_q_"
    r, s = fixture_solve(g9, key, ocp, u0=g9[key + "u0fix"])
    e_x, e_u = scaled(s.dV_dx0, g9[key + "dV_dx0"]), scaled(s.dQ_du0, g9[key + "dQ_du0"])
    print(f"state sens {model} Q mode: dQ/dx0 {e_x:.1e}; dQ/du0 {e_u:.1e}")
    assert e_x <= RTOL and e_u <= RTOL
    assert torch.equal(s.dpi_dx0, torch.zeros_like(s.dpi_dx0))


@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_per_instance_theta_against_the_mirror(g9, model):
    ocp, _ = C.problem(model, 20)
    key = f"{model}_th_"
    r, s = fixture_solve(g9, key, ocp, theta=g9[key + "theta"])
    bar, err_dp, e_pi = policy_errors(g9, key, r, s)
    e_v = scaled(s.dV_dx0, g9[key + "dV_dx0"])
    print(f"state sens {model} per-instance theta: du0*/dp {err_dp:.1e} -> bar {bar:.1e}; du0*/dx0 {e_pi:.1e}; dV/dx0 {e_v:.1e}")
    assert e_pi <= bar and e_v <= RTOL


# ---------------------------------------------------------------------- 2. kernel A at the product's own iterate
def stage0_case(name):
    from mpc4rl_amd import cartpole_ocp, chain_mass_ocp, linear_system_ocp
    from oracle.problems import make_cartpole, make_chain_mass, make_linear_system
    rng = np.random.default_rng(7)
    B = 5
    if name == "cartpole":
        return cartpole_ocp(), make_cartpole(), rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.5]), rng.uniform(-15, 15, (B, 1))
    if name == "linear":
        x0 = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.2, 0.5, B)])
        return linear_system_ocp(N=40), make_linear_system(N=40), x0, rng.uniform(-0.9, 0.9, (B, 1))
    n_mass, N = (3, 10) if name == "chain3" else (7, 8)
    ocp, P = chain_mass_ocp(n_mass=n_mass, N=N), make_chain_mass(n_mass=n_mass, N=N)
    return ocp, P, np.tile(ocp.x0, (B, 1)) + rng.normal(0.0, 0.02, (B, P.nx)), rng.uniform(-0.5, 0.5, (B, 3))


@pytest.mark.parametrize("q_mode", [False, True])
@pytest.mark.parametrize("name", ["cartpole", "linear", "chain3", "chain7"])
def test_stage0_gradients_at_the_products_iterate(name, q_mode):
    """dV/dx0 = -pi0 of solution_from_iterate on the pulled iterate, dQ/du0 = autograd of l0 with the oracle's stage_cost / F: one
    smooth fp64 expression at identical inputs on both sides.  Measured: at most 3.9e-16 over the eight cases."""
    from oracle.from_iterate import solution_from_iterate
    ocp, P, x0, u0 = stage0_case(name)
    mpc = handle(ocp, len(x0), tol=1e-8)
    r = mpc.solve(x0, u0 if q_mode else None, cold=True)
    s = mpc.state_sens(q_mode=q_mode, policy=False)
    x, u, pi, bnd, _ = (t.cpu().numpy() for t in mpc.get_iterate())
    assert s.dpi_dx0 is None and (s.dQ_du0 is not None) == q_mode
    want_x, want_u = [], []
    c0 = float(P.cost_scaling()[0])
    for i in range(len(x0)):
        sol = solution_from_iterate(P, x[i], u[i], pi[i], bnd[i], u0fix=u0[i] if q_mode else None, cost=float(r.V[i]))
        want_x.append(-sol.pi0)
        ut = torch.tensor(u[i, 0], requires_grad=True)
        l0 = c0 * P.stage_cost(0, torch.tensor(x[i, 0]), ut, torch.tensor(P.p0)) + torch.tensor(pi[i, 0]) @ P.F(torch.tensor(x[i, 0]), ut, torch.tensor(P.p0))
        want_u.append(torch.autograd.grad(l0, ut)[0].numpy())
    e_x = scaled(s.dV_dx0, np.array(want_x))
    e_u = scaled(s.dQ_du0, np.array(want_u)) if q_mode else 0.0
    print(f"stage-0 gradients {name} {'Q' if q_mode else 'V'} mode: d/dx0 {e_x:.1e}; dQ/du0 {e_u:.1e}")
    assert e_x <= 1e-10 and e_u <= 1e-10


# ---------------------------------------------------------------------- 3. closed form
def lqr_closed_form(A, B, P, gamma, N):
    """(K_0, S_0) of the discounted finite-horizon LQR the linear-system OCP is without bounds: stage weights c_k I (c_0 = 1,
    c_k = gamma^k), terminal weight gamma^N P."""
    S = gamma ** N * P
    K = None
    for k in range(N - 1, -1, -1):
        c = 1.0 if k == 0 else gamma ** k
        K = np.linalg.solve(c * np.eye(1) + B.T @ S @ B, B.T @ S @ A)
        S = c * np.eye(2) + A.T @ S @ (A - B @ K)
    return K, S


def test_closed_form_of_the_unconstrained_linear_system():
    """No bound active (all at +-100): u0* = -K_0 x0 and V = 1/2 x0' S_0 x0 + V_0, so du0*/dx0 = -K_0 and dV/dx0 = S_0 x0.  The
    closed form is first held to u0 and V of tests/golden/g1_lqr.json; 1e-9 is the bar tests/test_oracle.py holds that file to."""
    from mpc4rl_amd import _lib, linear_system_ocp
    g1 = json.load(open(os.path.join(GOLD, "g1_lqr.json")))
    A, Bm, P, x0 = np.array(g1["A"]), np.array(g1["B"]), np.array(g1["P_dare"]), np.array(g1["x0"])
    for c in g1["cases"]:
        K, S = lqr_closed_form(A, Bm, P, c["gamma"], g1["N"])
        assert abs(float((-K @ x0)[0]) - c["u0"]) < 1e-9 and abs(0.5 * x0 @ S @ x0 + g1["V_0"] - c["V"]) < 1e-9
        mpc = handle(linear_system_ocp(discount_factor=c["gamma"], N=g1["N"]), 1, tol=1e-10)
        mpc.set_bounds(_lib.BOUNDS_U0, [-100.0], [100.0])
        mpc.set_bounds(_lib.BOUNDS_STAGE, [-100.0] * 3, [100.0] * 3)
        r = mpc.solve(x0[None], cold=True)
        s = mpc.state_sens()
        torch.cuda.synchronize()
        e_u, e_v = float(np.abs(s.dpi_dx0[0].cpu().numpy() + K).max()), float(np.abs(s.dV_dx0[0].cpu().numpy() - S @ x0).max())
        print(f"closed form gamma {c['gamma']}: du0*/dx0 {e_u:.1e}; dV/dx0 {e_v:.1e}")
        assert int(r.status[0]) == 0 and abs(float(r.u0[0, 0]) - c["u0"]) < 1e-9
        assert e_u < 1e-9 and e_v < 1e-9


# ---------------------------------------------------------------------- 4. contract
def raw_state_sens(mpc, q_mode, want=(True, False, True), fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    from mpc4rl_amd import _lib
    kw = dict(dtype=torch.float64, device=mpc.device)
    shapes = ((mpc.B, mpc.nx), (mpc.B, mpc.nu), (mpc.B, mpc.nu, mpc.nx))
    bufs = [torch.full(sh, fill, **kw) if w else None for sh, w in zip(shapes, want)]
    mpc._call("mpcrl_state_sens", _lib.STATE_Q_MODE if q_mode else 0, *bufs)
    torch.cuda.synchronize()
    return bufs


@pytest.fixture(scope="module")
def cp16():
    """cartpole N 20, B 16: x0 of tests/small_mode_cases.py with instance 5 made NaN."""
    ocp, _ = C.problem("cartpole", 20)
    rng = np.random.default_rng(41)
    x0 = rng.uniform(-1, 1, (16, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    x0[5, 2] = float("nan")
    return ocp, x0


def test_every_requested_row_is_written_and_failed_instances_are_zero(cp16):
    ocp, x0 = cp16
    mpc = handle(ocp, 16)
    r = mpc.solve(x0, cold=True)
    dV, _, dpi = raw_state_sens(mpc, False)
    st = r.status.cpu().numpy()
    assert st[5] == 1 and np.all(np.delete(st, 5) == 0)
    assert torch.isfinite(dV).all() and torch.isfinite(dpi).all()
    assert torch.all(dV[5] == 0) and torch.all(dpi[5] == 0) and torch.all(dV[4].abs() > 0) and torch.all(dpi[4].abs() > 0)
    s = mpc.state_sens()      # the Python surface: the same numbers, rows selected by the status it holds
    assert same((dV, dpi), (s.dV_dx0, s.dpi_dx0))
    u0 = np.full((16, 1), 3.0)
    mpc.solve(x0, u0, cold=True)
    dV, dQ, dpi = raw_state_sens(mpc, True, (True, True, True))
    assert torch.isfinite(dV).all() and torch.isfinite(dQ).all() and torch.equal(dpi, torch.zeros_like(dpi))      # Q mode: exact zeros
    assert torch.all(dV[5] == 0) and torch.all(dQ[5] == 0) and torch.all(dQ[4].abs() > 0)
    only = raw_state_sens(mpc, True, (False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], dQ)


def test_refusals():
    from mpc4rl_amd import MPCBatch, chain_mass_ocp, linear_system_ocp
    lin = MPCBatch(linear_system_ocp(N=7), 3)
    x0 = np.array([[0.5, 0.1], [0.3, 0.2], [0.6, -0.1]])
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_state_sens(lin, False)                                  # before any solve
    with pytest.raises(RuntimeError):
        lin.state_sens()
    lin.solve(x0, cold=True, store_bounds=False)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_state_sens(lin, False)                                  # the bound planes are placeholders
    with pytest.raises(RuntimeError):
        lin.state_sens()
    lin.solve(x0, cold=True)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_state_sens(lin, False, (True, True, True))              # dQ/du0 in V mode
    x, u, pi, _, _ = lin.get_iterate()
    lin.set_iterate(x, u, pi)                                       # without bnd
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_state_sens(lin, False)
    chain = MPCBatch(chain_mass_ocp(n_mass=3, N=10), 2)
    chain.solve(np.tile(chain.ocp.x0, (2, 1)), cold=True)
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        raw_state_sens(chain, False)                                # du0*/dx0 on a chain handle
    dV, _, _ = raw_state_sens(chain, False, (True, False, False))
    assert torch.isfinite(dV).all()


def test_same_bits_whatever_the_order_and_the_launch_shape(cp16):
    """An explicit packing order, the time-sliced against the plain solve launch, and a second call: the same bits; and the call
    leaves the solve's outputs and the stored iterate alone."""
    ocp, x0 = cp16
    x0 = np.nan_to_num(x0, nan=0.1)
    ref = None
    for mode, perm in ((-1, None), (1, None), (-1, torch.arange(15, -1, -1))):
        mpc = handle(ocp, 16)
        mpc.set_launch_mode(mode)
        mpc.set_order(perm)
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True, reorder=False)
        before = [t.clone() for t in (r.u0, r.V, r.status, r.iters, r.dV_dp, r.dpi_dp, *mpc.get_iterate(), mpc.get_lagrangian())]
        a = raw_state_sens(mpc, False)
        b = raw_state_sens(mpc, False)
        after = [r.u0, r.V, r.status, r.iters, r.dV_dp, r.dpi_dp, *mpc.get_iterate(), mpc.get_lagrangian()]
        torch.cuda.synchronize()
        assert same((a[0], a[2]), (b[0], b[2]))
        assert all(torch.equal(p, q) for p, q in zip(before, after))
        ref = a if ref is None else ref
        assert same((a[0], a[2]), (ref[0], ref[2])), (mode, perm is not None)


def test_replays_inside_a_graph(cp16):
    ocp, x0 = cp16
    mpc = handle(ocp, 16)
    mpc.solve(np.nan_to_num(x0, nan=0.1), cold=True)
    want = raw_state_sens(mpc, False)
    from mpc4rl_amd import _lib
    dV = torch.zeros((16, 4), dtype=torch.float64, device=mpc.device)
    dpi = torch.zeros((16, 1, 4), dtype=torch.float64, device=mpc.device)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node chain: no parallel branches
        mpc._call("mpcrl_state_sens", 0, dV, None, dpi)
    torch.cuda.synchronize()
    assert torch.all(dV == 0) and torch.all(dpi == 0)      # captured, not run
    for _ in range(2):
        dV.fill_(float("nan")), dpi.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same((dV, dpi), (want[0], want[2]))


def test_mpc_getters_beside_their_dp_siblings():
    """MPC.get_dV_dx0 / get_dQ_du0 / get_dpi_dx0: numpy, shaped like get_dV_dp / get_dpi_dp, from the last update / q_update; a
    parameter written in between makes them solve again."""
    from mpc4rl_amd import LinearSystemMPC, MPCBatch
    mpc = LinearSystemMPC()
    x0 = np.array([0.4, 0.2])
    mpc.update(x0)
    dV, dpi = mpc.get_dV_dx0(), mpc.get_dpi_dx0()
    assert dV.shape == (1, 2) and dpi.shape == (1, 2) and mpc.get_dV_dp().shape == (1, mpc.ocp.n_p) and mpc.get_dpi_dp().shape == (1, mpc.ocp.n_p)
    ref = MPCBatch(mpc.ocp, 1)
    ref.solve(x0[None], cold=True)
    s = ref.state_sens()
    assert np.allclose(dV, s.dV_dx0.cpu().numpy(), rtol=0, atol=1e-9) and np.allclose(dpi, s.dpi_dx0[0].cpu().numpy(), rtol=0, atol=1e-9)
    with pytest.raises(RuntimeError):
        mpc.get_dQ_du0()
    p = mpc.get_p()
    p[5] *= 1.05
    mpc.set_p(p)
    assert np.abs(mpc.get_dpi_dx0() - dpi).max() > 1e-4      # another problem: solved again, not the cached rows
    mpc.q_update(x0, np.array([0.1]))
    assert mpc.get_dQ_du0().shape == (1, 1) and abs(float(mpc.get_dQ_du0()[0, 0])) > 0 and np.all(mpc.get_dpi_dx0() == 0)
    assert mpc.get_dV_dx0().shape == (1, 2)


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


@pytest.mark.parametrize("model,N,B", [("linear", 8, 3), ("cartpole", 6, 2)])
def test_layer_gradients_against_differences_of_its_forward_pass(model, N, B):
    from mpc4rl_amd import MPCLayer
    ocp, _ = C.problem(model, N)
    layer = MPCLayer(handle(ocp, B, tol=1e-10), cold=True)
    rng = np.random.default_rng(11)
    if model == "linear":
        x0 = np.column_stack([rng.uniform(0.2, 0.8, B), rng.uniform(-0.2, 0.3, B)])
    else:
        x0 = rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    x0 = torch.tensor(x0, device="cuda", requires_grad=True)
    theta = torch.tensor(ocp.p0, device="cuda", requires_grad=model == "linear")
    w = torch.tensor(rng.uniform(0.5, 1.5, (B, 1)), device="cuda")

    def loss(x, th):
        u0, V = layer(x, th)
        return (w * u0).sum() + V.sum()

    loss(x0, theta).backward()
    assert layer.last_status.tolist() == [0] * B
    with torch.no_grad():
        gx = layer_differences(lambda z: float(loss(z, theta.detach())), x0.detach().clone())
        e_x = scaled(x0.grad, gx.cpu().numpy())
        e_t = 0.0
        if model == "linear":      # shared theta: the gradient is the sum over the batch
            gt = layer_differences(lambda z: float(loss(x0.detach(), z)), theta.detach().clone())
            e_t = scaled(theta.grad[None], gt.cpu().numpy()[None])
    print(f"layer {model} N {N}: d loss/d x0 {e_x:.1e}; d loss/d theta {e_t:.1e}")
    assert e_x <= 1e-5 and e_t <= 1e-5


def test_layer_q_per_instance_theta_and_an_encoder_in_front():
    from mpc4rl_amd import MPCLayer
    ocp, _ = C.problem("linear", 8)
    B = 3
    layer = MPCLayer(handle(ocp, B, tol=1e-10), cold=True)
    rng = np.random.default_rng(12)
    x0 = torch.tensor(np.column_stack([rng.uniform(0.2, 0.8, B), rng.uniform(-0.2, 0.3, B)]), device="cuda", requires_grad=True)
    u0 = torch.tensor(rng.uniform(-0.5, 0.5, (B, 1)), device="cuda", requires_grad=True)
    theta = torch.tensor(np.tile(ocp.p0, (B, 1)), device="cuda", requires_grad=True)
    layer.q(x0, u0, theta).sum().backward()
    with torch.no_grad():
        gu = layer_differences(lambda z: float(layer.q(x0.detach(), z, theta.detach()).sum()), u0.detach().clone())
        gx = layer_differences(lambda z: float(layer.q(z, u0.detach(), theta.detach()).sum()), x0.detach().clone())
        gt = layer_differences(lambda z: float(layer.q(x0.detach(), u0.detach(), z).sum()), theta.detach().clone())
    e = [scaled(a.grad, b.cpu().numpy()) for a, b in ((u0, gu), (x0, gx), (theta, gt))]
    print(f"layer.q linear N 8: d/du0 {e[0]:.1e}; d/dx0 {e[1]:.1e}; d/dtheta (per instance) {e[2]:.1e}")
    assert theta.grad.shape == (B, ocp.n_p) and max(e) <= 1e-5
    # an observation encoder upstream of x0 (float32, as a network would be): a finite, non-zero gradient reaches its weights
    enc = torch.nn.Linear(5, 2).cuda()
    obs = torch.tensor(rng.uniform(-1, 1, (B, 5)), dtype=torch.float32, device="cuda")
    u, V = layer(0.1 * torch.tanh(enc(obs)) + torch.tensor([0.5, 0.0], device="cuda"), torch.tensor(ocp.p0, device="cuda"))
    (u.sum() + V.sum()).backward()
    assert layer.last_status.tolist() == [0] * B
    for p in enc.parameters():
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0


def test_layer_gives_zero_gradient_for_a_failed_instance_and_refuses_the_chain_policy_jacobian():
    from mpc4rl_amd import MPCBatch, MPCLayer, chain_mass_ocp
    ocp, _ = C.problem("cartpole", 6)
    layer = MPCLayer(handle(ocp, 2), cold=True)
    x0 = torch.tensor([[0.1, 0.0, 0.1, 0.0], [0.1, 0.0, float("nan"), 0.0]], device="cuda", requires_grad=True)
    theta = torch.tensor(ocp.p0, device="cuda", requires_grad=True)
    u, V = layer(x0, theta)
    (torch.nan_to_num(u).sum() + torch.nan_to_num(V).sum()).backward()
    assert layer.last_status.tolist() == [0, 1]
    assert torch.isfinite(x0.grad).all() and torch.isfinite(theta.grad).all() and torch.all(x0.grad[1] == 0) and torch.all(x0.grad[0] != 0)
    cocp = chain_mass_ocp(n_mass=3, N=10)
    chain = MPCLayer(MPCBatch(cocp, 2), cold=True)
    xc = torch.tensor(np.tile(cocp.x0, (2, 1)), device="cuda", requires_grad=True)
    u, V = chain(xc, torch.tensor(cocp.p0, device="cuda"))
    V.sum().backward()                                             # the value alone: dV/dx0 is there
    assert torch.isfinite(xc.grad).all() and float(xc.grad.abs().max()) > 0
    u, V = chain(xc, torch.tensor(cocp.p0, device="cuda"))
    with pytest.raises(RuntimeError, match="du0\\*/dx0 is not available for the chain"):
        (u.sum() + V.sum()).backward()


MEASURED_POLICY = """\
state sens cartpole N 2 B 13: all: du0*/dp 2.9e-09 -> bar 1.0e-06, du0*/dx0 3.1e-08; no positive slack (13): du0*/dp 2.9e-09 -> bar 1.0e-06, du0*/dx0 3.1e-08; dV/dx0 3.4e-11
state sens cartpole N 2 B 1: all: du0*/dp 1.9e-10 -> bar 1.0e-06, du0*/dx0 3.2e-10; no positive slack (1): du0*/dp 1.9e-10 -> bar 1.0e-06, du0*/dx0 3.2e-10; dV/dx0 2.7e-12
state sens cartpole N 15 B 13: all: du0*/dp 3.1e-08 -> bar 1.0e-06, du0*/dx0 1.5e-08; no positive slack (13): du0*/dp 3.1e-08 -> bar 1.0e-06, du0*/dx0 1.5e-08; dV/dx0 7.3e-11
state sens cartpole N 15 B 1: all: du0*/dp 4.0e-10 -> bar 1.0e-06, du0*/dx0 3.9e-10; no positive slack (1): du0*/dp 4.0e-10 -> bar 1.0e-06, du0*/dx0 3.9e-10; dV/dx0 1.1e-11
state sens cartpole N 20 B 13: all: du0*/dp 1.9e-08 -> bar 1.0e-06, du0*/dx0 1.4e-08; no positive slack (13): du0*/dp 1.9e-08 -> bar 1.0e-06, du0*/dx0 1.4e-08; dV/dx0 9.3e-11
state sens cartpole N 20 B 1: all: du0*/dp 1.9e-08 -> bar 1.0e-06, du0*/dx0 3.6e-09; no positive slack (1): du0*/dp 1.9e-08 -> bar 1.0e-06, du0*/dx0 3.6e-09; dV/dx0 2.5e-11
state sens cartpole N 31 B 13: all: du0*/dp 9.8e-08 -> bar 1.0e-06, du0*/dx0 7.3e-08; no positive slack (13): du0*/dp 9.8e-08 -> bar 1.0e-06, du0*/dx0 7.3e-08; dV/dx0 1.4e-10
state sens cartpole N 31 B 1: all: du0*/dp 9.8e-08 -> bar 1.0e-06, du0*/dx0 7.3e-08; no positive slack (1): du0*/dp 9.8e-08 -> bar 1.0e-06, du0*/dx0 7.3e-08; dV/dx0 6.3e-11
state sens cartpole N 32 B 13: all: du0*/dp 4.0e-08 -> bar 1.0e-06, du0*/dx0 4.2e-08; no positive slack (13): du0*/dp 4.0e-08 -> bar 1.0e-06, du0*/dx0 4.2e-08; dV/dx0 1.7e-10
state sens cartpole N 32 B 1: all: du0*/dp 1.0e-10 -> bar 1.0e-06, du0*/dx0 1.7e-09; no positive slack (1): du0*/dp 1.0e-10 -> bar 1.0e-06, du0*/dx0 1.7e-09; dV/dx0 1.1e-11
state sens cartpole N 63 B 13: all: du0*/dp 3.0e-07 -> bar 1.2e-06, du0*/dx0 4.4e-08; no positive slack (13): du0*/dp 3.0e-07 -> bar 1.2e-06, du0*/dx0 4.4e-08; dV/dx0 7.7e-11
state sens cartpole N 63 B 1: all: du0*/dp 3.0e-07 -> bar 1.2e-06, du0*/dx0 1.1e-08; no positive slack (1): du0*/dp 3.0e-07 -> bar 1.2e-06, du0*/dx0 1.1e-08; dV/dx0 8.9e-12
state sens linear N 2 B 25: all: du0*/dp 1.0e+00 -> bar 4.2e+00, du0*/dx0 1.0e+00; no positive slack (10): du0*/dp 2.2e-08 -> bar 1.0e-06, du0*/dx0 2.1e-08; dV/dx0 1.4e-15
state sens linear N 2 B 1: all: du0*/dp 5.1e-09 -> bar 1.0e-06, du0*/dx0 2.7e-09; no positive slack (1): du0*/dp 5.1e-09 -> bar 1.0e-06, du0*/dx0 2.7e-09; dV/dx0 1.4e-16
state sens linear N 7 B 25: all: du0*/dp 4.0e+00 -> bar 1.6e+01, du0*/dx0 1.1e+00; no positive slack (10): du0*/dp 1.2e-07 -> bar 1.0e-06, du0*/dx0 3.2e-08; dV/dx0 9.8e-09
state sens linear N 7 B 1: all: du0*/dp 1.6e-08 -> bar 1.0e-06, du0*/dx0 1.2e-08; no positive slack (1): du0*/dp 1.6e-08 -> bar 1.0e-06, du0*/dx0 1.2e-08; dV/dx0 1.3e-15
state sens linear N 20 B 25: all: du0*/dp 1.3e+00 -> bar 5.2e+00, du0*/dx0 1.1e+00; no positive slack (11): du0*/dp 1.3e-05 -> bar 5.2e-05, du0*/dx0 6.4e-07; dV/dx0 1.6e-08
state sens linear N 20 B 1: all: du0*/dp 3.2e-09 -> bar 1.0e-06, du0*/dx0 3.0e-09; no positive slack (1): du0*/dp 3.2e-09 -> bar 1.0e-06, du0*/dx0 3.0e-09; dV/dx0 1.8e-15
state sens linear N 31 B 25: all: du0*/dp 2.3e+00 -> bar 9.2e+00, du0*/dx0 1.1e+00; no positive slack (10): du0*/dp 7.7e-06 -> bar 3.1e-05, du0*/dx0 6.5e-08; dV/dx0 4.4e-09
state sens linear N 31 B 1: all: du0*/dp 4.2e-09 -> bar 1.0e-06, du0*/dx0 3.4e-09; no positive slack (1): du0*/dp 4.2e-09 -> bar 1.0e-06, du0*/dx0 3.4e-09; dV/dx0 8.7e-15
state sens linear N 32 B 25: all: du0*/dp 1.1e+01 -> bar 4.5e+01, du0*/dx0 1.3e+00; no positive slack (12): du0*/dp 5.1e-05 -> bar 2.1e-04, du0*/dx0 1.8e-07; dV/dx0 1.2e-08
state sens linear N 32 B 1: all: du0*/dp 5.1e-05 -> bar 2.1e-04, du0*/dx0 1.8e-07; no positive slack (1): du0*/dp 5.1e-05 -> bar 2.1e-04, du0*/dx0 1.8e-07; dV/dx0 1.2e-08
state sens linear N 63 B 25: all: du0*/dp 2.3e+00 -> bar 9.1e+00, du0*/dx0 1.1e+00; no positive slack (10): du0*/dp 1.0e-05 -> bar 4.1e-05, du0*/dx0 2.0e-06; dV/dx0 6.6e-09
state sens linear N 63 B 1: all: du0*/dp 2.4e-08 -> bar 1.0e-06, du0*/dx0 2.3e-08; no positive slack (1): du0*/dp 2.4e-08 -> bar 1.0e-06, du0*/dx0 2.3e-08; dV/dx0 1.2e-13
state sens cartpole Q mode: dQ/dx0 1.6e-10; dQ/du0 5.1e-12
state sens linear Q mode: dQ/dx0 3.3e-07; dQ/du0 1.1e-07
state sens cartpole per-instance theta: du0*/dp 2.0e-08 -> bar 1.0e-06; du0*/dx0 3.6e-09; dV/dx0 2.3e-11
state sens linear per-instance theta: du0*/dp 3.6e-08 -> bar 1.0e-06; du0*/dx0 3.7e-08; dV/dx0 1.5e-15
"""
