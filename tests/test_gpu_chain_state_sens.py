"""mpcrl_chain_policy_state_sens (include/mpcrl_chain_ext.h) on the device: du0*/dx0 of the chain of masses from the adjoint solve of
its du0*/dp pass (chain_state_sens_kernel, csrc/chain_sens.hpp) against the mirror fixture G10 (tests/golden/make_chain_state_sens.py),
the two launch routes bit for bit, the call's contract and refusals, graph capture, the MPC getter and the autograd layer.

Bars.  du0*/dx0 against the fixture: max(1e-6, 4 x the error of the same solve's du0*/dp against the fixture's mirror du0*/dp) — one
adjoint solution contracted twice, the rule of tests/test_gpu_state_sens.py; 1e-6 is RTOL of tests/small_mode_cases.py.  dV/dx0: 1e-6.
Rows are scaled by max(|reference row|, 1).  The layer against central differences of its own forward pass at h = 1e-5: 1e-5.

Measured on an MI355X: MEASURED at the end of this file (every line the first and the layer test print).
"""
import os

import numpy as np
import pytest
import torch

import small_mode_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = C.RTOL
SETS = ((3, 1, "ss"), (3, 2, "ss"), (3, 10, "ss"), (3, 10, "x0"), (4, 3, "ss"), (5, 8, "ss"), (6, 3, "ss"), (7, 5, "ss"))


@pytest.fixture(scope="module")
def g10():
    return np.load(os.path.join(ROOT, "tests", "golden", "g10_chain_state_sens.npz"))


def scaled(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    got, ref = got.reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)).max())


def chain(n_mass, N, B, tol=1e-9):
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    mpc = MPCBatch(chain_mass_ocp(n_mass=n_mass, N=N), B)
    mpc.set_options(tol=tol)
    return mpc


def bits(t):
    return t.view(torch.int64)


def raw(mpc, status, q_mode=False, fill=float("nan")):
    """The library call itself on a buffer poisoned with ``fill``."""
    from mpc4rl_amd import _lib
    out = torch.full((mpc.B, mpc.nu, mpc.nx), fill, dtype=torch.float64, device=mpc.device)
    mpc._call("mpcrl_chain_policy_state_sens", _lib.STATE_Q_MODE if q_mode else 0, status, out)
    torch.cuda.synchronize()
    return out


def x0_near_ss(mpc, B, seed):
    return np.tile(mpc.ocp.consts, (B, 1)) + np.random.default_rng(seed).normal(0.0, 0.01, (B, mpc.nx))


# ---------------------------------------------------------------------- 1. against the fixture
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_policy_and_value_jacobians_against_the_mirror(g10, n_mass, N, base):
    """Cold solve at tol 1e-9 with sens_v and sens_pi on the fixture's x0, all four instances and then the first alone (B = 1).
    Negative control: against the fixture rows of the neighbouring instance the error must exceed the bar (the neighbours' du0*/dx0
    differ by 6e-4 .. 1e-2 in the fixture)."""
    key = f"m{n_mass}_N{N}_{base}_"
    for rows in (slice(0, 4), slice(0, 1)):
        x0 = g10[key + "x0"][rows]
        mpc = chain(n_mass, N, len(x0))
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
        s = mpc.state_sens()
        torch.cuda.synchronize()
        assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
        err_dp = scaled(r.dpi_dp, g10[key + "dpi_dp"][rows])
        bar = max(RTOL, 4.0 * err_dp)
        e_pi, e_v = scaled(s.dpi_dx0, g10[key + "dpi_dx0"][rows]), scaled(s.dV_dx0, g10[key + "dV_dx0"][rows])
        wrong = scaled(s.dpi_dx0, np.roll(g10[key + "dpi_dx0"], -1, 0)[rows])
        print(f"chain state sens n_mass {n_mass} N {N} {base} B {len(x0)}: du0*/dp {err_dp:.1e} -> bar {bar:.1e}, du0*/dx0 {e_pi:.1e}; "
              f"dV/dx0 {e_v:.1e}; against the neighbour's rows {wrong:.1e}")
        assert s.dQ_du0 is None and s.dpi_dx0.shape == (len(x0), 3, mpc.nx)
        assert e_pi <= bar and e_v <= RTOL and wrong > bar, (key, err_dp, bar, e_pi, e_v, wrong)


# ---------------------------------------------------------------------- 2. the two routes
@pytest.mark.parametrize("n_mass,N", [(3, 10), (6, 3)])
def test_both_routes_give_the_same_bits(n_mass, N):
    """After a solve with sens_pi the call is the contraction alone; after a plain solve on the same inputs it runs the adjoint
    pipeline first.  The same bits, and a second call in a row gives them again."""
    got = []
    for sens_pi in (True, False):
        mpc = chain(n_mass, N, 4)
        r = mpc.solve(x0_near_ss(mpc, 4, 3), sens_pi=sens_pi, cold=True)
        a, b = raw(mpc, r.status), raw(mpc, r.status)
        assert r.status.tolist() == [0] * 4 and torch.isfinite(a).all() and float(a.abs().max()) > 0
        assert torch.equal(bits(a), bits(b)), sens_pi
        got.append(a)
    assert torch.equal(bits(got[0]), bits(got[1]))


# ---------------------------------------------------------------------- 3. contract
def test_rows_are_written_in_full_and_the_solve_is_left_alone():
    mpc = chain(3, 10, 4)
    x0 = x0_near_ss(mpc, 4, 5)
    x0[2, 4] = float("nan")
    for sens_pi in (True, False):      # both routes
        r = mpc.solve(x0, sens_v=True, sens_pi=sens_pi, cold=True)
        outs = [r.u0, r.V, r.status, r.iters, r.dV_dp] + ([r.dpi_dp] if sens_pi else [])
        before = [t.clone() for t in (*outs, *mpc.get_iterate(), mpc.get_lagrangian())]
        J = raw(mpc, r.status)
        st = r.status.tolist()
        assert st[2] not in (0, 2) and [st[i] for i in (0, 1, 3)] == [0, 0, 0]
        assert torch.isfinite(J).all() and torch.all(J[2] == 0)      # poisoned with NaN: every row was written
        for i in (0, 1, 3):
            assert float(J[i].abs().max()) > 0 and torch.all(J[i].abs().amax(1) > 0)
        after = [*outs, *mpc.get_iterate(), mpc.get_lagrangian()]
        torch.cuda.synchronize()
        assert all(torch.equal(bits(p) if p.dtype == torch.float64 else p, bits(q) if q.dtype == torch.float64 else q)
                   for p, q in zip(before, after))
        s = mpc.state_sens()      # the Python surface: the same numbers
        assert torch.equal(bits(s.dpi_dx0), bits(J)) and torch.all(s.dV_dx0[2] == 0)
    # Q mode: exact zeros, whatever the buffer held
    r = mpc.solve(np.nan_to_num(x0, nan=0.2), np.full((4, 3), 0.1), cold=True)
    assert torch.equal(raw(mpc, r.status, q_mode=True), torch.zeros((4, 3, mpc.nx), dtype=torch.float64, device=mpc.device))
    s = mpc.state_sens(q_mode=True)
    assert torch.all(s.dpi_dx0 == 0) and s.dQ_du0.shape == (4, 3) and torch.isfinite(s.dV_dx0).all()


# ---------------------------------------------------------------------- 4. refusals
def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, linear_system_ocp
    mpc = chain(3, 10, 2)
    x0 = x0_near_ss(mpc, 2, 7)
    st = torch.zeros((2,), dtype=torch.int32, device=mpc.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, st)                                                # before any solve
    with pytest.raises(RuntimeError):
        mpc.state_sens()
    r = mpc.solve(x0, cold=True)
    assert torch.isfinite(raw(mpc, r.status)).all()
    x, u, pi, bnd, _ = mpc.get_iterate()
    mpc.set_iterate(x, u, pi, bnd)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status)                                          # the workspace is not that iterate's
    with pytest.raises(RuntimeError, match="workspace of the last solve"):
        mpc.state_sens()
    r = mpc.solve(x0, cold=True)
    mpc.set_theta(torch.as_tensor(mpc.ocp.p0))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status)
    r = mpc.solve(x0, cold=True)
    mpc.set_bounds(_lib.BOUNDS_U0, -0.9 * np.ones(3), 0.9 * np.ones(3))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status)
    with pytest.raises(RuntimeError, match="workspace of the last solve"):
        mpc.state_sens()
    # the other three calls that clear the library's flags (raw() goes past the Python mirror of them)
    r = mpc.solve(x0, cold=True)
    mpc.set_discount_factor(0.99)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status)
    r = mpc.solve(x0, cold=True)
    x, u, pi, bnd, _ = mpc.get_iterate()
    mpc.set_iterate_rows(x, u, pi, bnd, torch.arange(2, dtype=torch.int64, device=mpc.device))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status)
    r = mpc.solve(x0, cold=True)
    mpc.reset(x0)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status)
    assert not mpc.chain_workspace_current
    r = mpc.solve(x0, cold=True)
    assert mpc.chain_workspace_current
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, None)                                              # status = NULL
    out = torch.zeros((2, 3, mpc.nx), dtype=torch.float64, device=mpc.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        mpc._call("mpcrl_chain_policy_state_sens", 2, r.status, out)      # unknown flag
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        mpc._call("mpcrl_chain_policy_state_sens", 0, r.status, None)
    assert torch.isfinite(raw(mpc, r.status)).all()                 # and the handle still answers
    lin = MPCBatch(linear_system_ocp(N=7), 2)
    rl = lin.solve(np.array([[0.5, 0.1], [0.3, 0.2]]), cold=True)
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        lin._call("mpcrl_chain_policy_state_sens", 0, rl.status, torch.zeros((2, 1, 2), dtype=torch.float64, device=lin.device))


# ---------------------------------------------------------------------- 5. graph capture
@pytest.mark.parametrize("sens_pi", [True, False])
def test_replays_inside_a_graph(sens_pi):
    mpc = chain(3, 10, 4)
    r = mpc.solve(x0_near_ss(mpc, 4, 9), sens_pi=sens_pi, cold=True)
    want = raw(mpc, r.status)
    out = torch.zeros_like(want)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node chain: no parallel branches
        mpc._call("mpcrl_chain_policy_state_sens", 0, r.status, out)
    torch.cuda.synchronize()
    assert torch.all(out == 0)          # captured, not run
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want))


# ---------------------------------------------------------------------- 6. the getter
def test_mpc_getter_on_the_chain():
    from mpc4rl_amd import ChainMassMPC, MPCBatch
    mpc = ChainMassMPC({"n_mass": 3, "N": 10})
    x0 = mpc.ocp.consts + np.random.default_rng(13).normal(0.0, 0.01, mpc.ocp.nx)
    mpc.update(x0)
    J = mpc.get_dpi_dx0()
    assert J.shape == (3, mpc.ocp.nx) and np.isfinite(J).all() and np.abs(J).max() > 0 and mpc.get_dV_dx0().shape == (1, mpc.ocp.nx)
    ref = MPCBatch(mpc.ocp, 1)
    ref.solve(x0[None], cold=True)
    assert np.allclose(J, ref.state_sens().dpi_dx0[0].cpu().numpy(), rtol=0, atol=1e-9)
    mpc.q_update(x0, np.array([0.1, 0.0, -0.1]))
    assert mpc.get_dpi_dx0().shape == (3, mpc.ocp.nx) and np.all(mpc.get_dpi_dx0() == 0)


def test_value_getters_on_the_chain_launch_what_they_launched_before():
    """get_dV_dx0 on a ChainMassMPC stays one mpcrl_state_sens without the policy part and never the chain call; after MPC.set it is
    evaluated at the edited iterate without another solve (as on the cartpole and the linear system); get_dpi_dx0 alone makes the
    chain call, once per solve, and refuses an iterate that was edited since."""
    from mpc4rl_amd import ChainMassMPC
    mpc = ChainMassMPC({"n_mass": 3, "N": 10})
    x0 = mpc.ocp.consts + np.random.default_rng(14).normal(0.0, 0.01, mpc.ocp.nx)
    mpc.update(x0)
    calls, inner = [], mpc._batch._call

    def recording(name, *args):
        calls.append((name, args))
        return inner(name, *args)

    mpc._batch._call = recording
    dV = mpc.get_dV_dx0()
    assert [n for n, _ in calls] == ["mpcrl_state_sens"] and calls[0][1][3] is None      # dpi_dx0 = NULL: stage0_grad_kernel alone
    assert mpc.get_dV_dx0() is not None and len(calls) == 1                              # cached
    J = mpc.get_dpi_dx0()
    assert [n for n, _ in calls] == ["mpcrl_state_sens", "mpcrl_chain_policy_state_sens"]
    assert np.array_equal(mpc.get_dpi_dx0(), J) and len(calls) == 2                      # cached on its own
    Q, last = mpc.get_Q(), mpc._last
    del calls[:]
    x1 = mpc.get(1, "x")
    mpc.set(1, "x", x1 + 1e-3)
    dV_edited = mpc.get_dV_dx0()
    names = [n for n, _ in calls]
    assert "mpcrl_solve" not in names and "mpcrl_chain_policy_state_sens" not in names and names.count("mpcrl_state_sens") == 1
    assert mpc._last is last and mpc.get_Q() == Q and dV_edited.shape == dV.shape and np.isfinite(dV_edited).all()
    with pytest.raises(RuntimeError, match="edited since"):
        mpc.get_dpi_dx0()
    assert "mpcrl_solve" not in [n for n, _ in calls]
    mpc.update(x0)
    assert np.allclose(mpc.get_dpi_dx0(), J, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------- 7. the layer
def layer_differences(f, z, h=1e-5):
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


def test_layer_with_the_chain_policy_jacobian():
    from mpc4rl_amd import MPCBatch, MPCLayer, cartpole_ocp
    B = 2
    mpc = chain(3, 6, B, tol=1e-10)
    ocp = mpc.ocp
    layer = MPCLayer(mpc, policy_jacobian=True, cold=True)
    rng = np.random.default_rng(17)
    x0 = torch.tensor(np.tile(ocp.consts, (B, 1)) + rng.normal(0.0, 0.01, (B, ocp.nx)), device="cuda", requires_grad=True)
    theta = torch.tensor(ocp.p0, device="cuda")
    w = torch.tensor(rng.uniform(0.5, 1.5, (B, 3)), device="cuda")

    def loss(x):
        u0, V = layer(x, theta)
        return (w * u0).sum() + V.sum()

    loss(x0).backward()
    assert layer.last_status.tolist() == [0] * B
    with torch.no_grad():
        gx = layer_differences(lambda z: float(loss(z)), x0.detach().clone())
    e_x = scaled(x0.grad, gx.cpu().numpy())
    print(f"layer chain n_mass 3 N 6: d loss/d x0 {e_x:.1e}")
    assert e_x <= 1e-5
    # an observation encoder upstream of x0 (float32, as a network would be): a finite, non-zero gradient reaches its weights
    enc = torch.nn.Linear(5, ocp.nx).cuda()
    obs = torch.tensor(rng.uniform(-1, 1, (B, 5)), dtype=torch.float32, device="cuda")
    u, V = layer(0.01 * torch.tanh(enc(obs)) + torch.tensor(ocp.consts, dtype=torch.float32, device="cuda"), theta)
    (u.sum() + V.sum()).backward()
    assert layer.last_status.tolist() == [0] * B
    for p in enc.parameters():
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0
    # the opt-out, on a model that has the Jacobian by default
    cocp = cartpole_ocp()
    off = MPCLayer(MPCBatch(cocp, 2), policy_jacobian=False, cold=True)
    xc = torch.tensor([[0.1, 0.0, 0.1, 0.0], [0.0, 0.1, 0.05, 0.0]], device="cuda", requires_grad=True)
    u, V = off(xc, torch.tensor(cocp.p0, device="cuda"))
    V.sum().backward()
    assert torch.isfinite(xc.grad).all()
    u, V = off(xc, torch.tensor(cocp.p0, device="cuda"))
    with pytest.raises(RuntimeError, match="policy_jacobian=False"):
        (u.sum() + V.sum()).backward()


MEASURED = """\
chain state sens n_mass 3 N 1 ss B 4: du0*/dp 1.6e-07 -> bar 1.0e-06, du0*/dx0 1.6e-07; dV/dx0 1.0e-09; against the neighbour's rows 3.8e-03
chain state sens n_mass 3 N 1 ss B 1: du0*/dp 1.6e-07 -> bar 1.0e-06, du0*/dx0 1.5e-07; dV/dx0 1.0e-09; against the neighbour's rows 6.6e-04
chain state sens n_mass 3 N 2 ss B 4: du0*/dp 3.2e-08 -> bar 1.0e-06, du0*/dx0 4.0e-08; dV/dx0 2.2e-09; against the neighbour's rows 3.5e-03
chain state sens n_mass 3 N 2 ss B 1: du0*/dp 3.1e-08 -> bar 1.0e-06, du0*/dx0 3.9e-08; dV/dx0 6.3e-10; against the neighbour's rows 2.8e-03
chain state sens n_mass 3 N 10 ss B 4: du0*/dp 3.9e-08 -> bar 1.0e-06, du0*/dx0 4.2e-08; dV/dx0 2.3e-09; against the neighbour's rows 4.8e-03
chain state sens n_mass 3 N 10 ss B 1: du0*/dp 3.5e-08 -> bar 1.0e-06, du0*/dx0 4.0e-08; dV/dx0 4.6e-10; against the neighbour's rows 3.8e-03
chain state sens n_mass 3 N 10 x0 B 4: du0*/dp 3.1e-08 -> bar 1.0e-06, du0*/dx0 4.2e-08; dV/dx0 2.2e-09; against the neighbour's rows 3.9e-03
chain state sens n_mass 3 N 10 x0 B 1: du0*/dp 3.1e-08 -> bar 1.0e-06, du0*/dx0 4.2e-08; dV/dx0 2.2e-09; against the neighbour's rows 3.8e-03
chain state sens n_mass 4 N 3 ss B 4: du0*/dp 1.3e-07 -> bar 1.0e-06, du0*/dx0 1.9e-07; dV/dx0 8.8e-10; against the neighbour's rows 9.6e-03
chain state sens n_mass 4 N 3 ss B 1: du0*/dp 6.9e-08 -> bar 1.0e-06, du0*/dx0 1.3e-07; dV/dx0 1.0e-11; against the neighbour's rows 9.6e-03
chain state sens n_mass 5 N 8 ss B 4: du0*/dp 4.3e-08 -> bar 1.0e-06, du0*/dx0 1.1e-07; dV/dx0 1.6e-10; against the neighbour's rows 5.2e-03
chain state sens n_mass 5 N 8 ss B 1: du0*/dp 3.8e-08 -> bar 1.0e-06, du0*/dx0 1.0e-07; dV/dx0 1.6e-10; against the neighbour's rows 2.0e-03
chain state sens n_mass 6 N 3 ss B 4: du0*/dp 4.4e-08 -> bar 1.0e-06, du0*/dx0 1.3e-07; dV/dx0 1.1e-09; against the neighbour's rows 1.0e-02
chain state sens n_mass 6 N 3 ss B 1: du0*/dp 4.4e-08 -> bar 1.0e-06, du0*/dx0 1.0e-07; dV/dx0 8.4e-11; against the neighbour's rows 1.0e-02
chain state sens n_mass 7 N 5 ss B 4: du0*/dp 9.1e-08 -> bar 1.0e-06, du0*/dx0 1.5e-07; dV/dx0 4.0e-10; against the neighbour's rows 5.5e-03
chain state sens n_mass 7 N 5 ss B 1: du0*/dp 8.4e-08 -> bar 1.0e-06, du0*/dx0 1.4e-07; dV/dx0 4.0e-11; against the neighbour's rows 2.0e-03
layer chain n_mass 3 N 6: d loss/d x0 1.1e-11
"""
