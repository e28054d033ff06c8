"""mpcrl_chain_traj_vjp (include/mpcrl_chain_traj_ext.h) on the device: the trajectory vector-Jacobian product of the chain of masses
from one adjoint Riccati solve (chain_traj_riccati_kernel / forward2_adj, chain_sens_mix2_kernel<M, 1>, chain_traj_out_kernel) against
the mirror fixture G12 (tests/golden/make_chain_traj_vjp.py), against the library's own du0*/dp and du0*/dx0, the two launch routes,
the call's contract and refusals, graph capture and the autograd layer.

Bars.  Against the fixture: max(1e-6, 4 x the error of the same solve's du0*/dp against the mirror's du0*/dp) — a second right-hand
side on one factorisation, the rule of tests/test_gpu_chain_state_sens.py; 1e-6 is RTOL of tests/small_mode_cases.py and the
fixture's gate.  Inside the library (unit cotangents against du0*/dp and du0*/dx0 of the same workspace): 1e-6; linearity of one
solve: 1e-12; the two routes: 1e-9 (the Hessians are recomputed in the same order; bit equality is not promised).  Rows are scaled
by max(|reference row|, 1).  The layer against central differences of its own forward pass at h = 1e-5: 1e-5.

Measured on an MI355X: MEASURED at the end of this file (every line the fixture and the layer test print).
"""
import os

import numpy as np
import pytest
import torch

import small_mode_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = C.RTOL
G10_SETS = ((3, 1, "ss"), (3, 2, "ss"), (3, 10, "ss"), (3, 10, "x0"), (4, 3, "ss"), (5, 8, "ss"), (6, 3, "ss"), (7, 5, "ss"))
SETS = G10_SETS + ((3, 10, "act"),)


@pytest.fixture(scope="module")
def g12():
    return np.load(os.path.join(ROOT, "tests", "golden", "g12_chain_traj_vjp.npz"))


@pytest.fixture(scope="module")
def g10():
    return np.load(os.path.join(ROOT, "tests", "golden", "g10_chain_state_sens.npz"))


def scaled(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)).max())


def chain(n_mass, N, B, tol=1e-9):
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    mpc = MPCBatch(chain_mass_ocp(n_mass=n_mass, N=N), B)
    mpc.set_options(tol=tol)
    return mpc


def bits(t):
    return t.view(torch.int64)


def split(mpc, G):
    """A cotangent on w = [U; X] (the mirror's order) [B, nw] -> gX [B, N+1, nx], gU [B, N, nu] on the device."""
    G = torch.as_tensor(np.asarray(G), dtype=torch.float64, device=mpc.device)
    nU = mpc.N * mpc.nu
    return G[:, nU:].reshape(mpc.B, mpc.N + 1, mpc.nx).contiguous(), G[:, :nU].reshape(mpc.B, mpc.N, mpc.nu).contiguous()


def raw(mpc, status, gX, gU, x0=True, theta=True, flags=0, fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    g_x0 = torch.full((mpc.B, mpc.nx), fill, **kw) if x0 else None
    g_th = torch.full((mpc.B, mpc.n_p), fill, **kw) if theta else None
    mpc._call("mpcrl_chain_traj_vjp", flags, status, gX, gU, g_x0, g_th)
    torch.cuda.synchronize()
    return g_x0, g_th


def policy(mpc, status):
    out = torch.full((mpc.B, mpc.nu, mpc.nx), float("nan"), dtype=torch.float64, device=mpc.device)
    mpc._call("mpcrl_chain_policy_state_sens", 0, status, out)
    torch.cuda.synchronize()
    return out


def x0_near_ss(mpc, B, seed):
    return np.tile(mpc.ocp.consts, (B, 1)) + np.random.default_rng(seed).normal(0.0, 0.01, (B, mpc.nx))


def normal_cotangent(mpc, seed):
    return split(mpc, np.random.default_rng(seed).standard_normal((mpc.B, mpc.N * mpc.nu + (mpc.N + 1) * mpc.nx)))


# ---------------------------------------------------------------------- 1. against the fixture
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_vjp_against_the_mirror(g12, g10, n_mass, N, base):
    """Cold solve at tol 1e-9 with sens_v and sens_pi on the fixture's x0, all four instances and then the first alone (B = 1); the
    fixture's three cotangents.  Negative control: against the fixture rows of the neighbouring instance the error must exceed the
    bar."""
    key = f"m{n_mass}_N{N}_{base}_"
    for rows in (slice(0, 4), slice(0, 1)):
        x0 = g12[key + "x0"][rows]
        mpc = chain(n_mass, N, len(x0))
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
        torch.cuda.synchronize()
        assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
        # the mirror's du0*/dp: all of it in G10; for the set G10 does not have, its row 0 (the fixture's unit cotangent)
        err_dp = scaled(r.dpi_dp, g10[key + "dpi_dp"][rows]) if base != "act" else scaled(r.dpi_dp[:, 0], g12[key + "g_theta"][rows, 2])
        bar = max(RTOL, 4.0 * err_dp)
        e_th = e_x = w_th = w_x = 0.0      # every figure the largest over the three cotangents, as the fixture's nb_theta / nb_x0
        for c in range(3):
            gX, gU = split(mpc, g12[key + "G"][rows, c])
            g_x0, g_th = mpc.chain_trajectory_vjp(gX, gU)
            assert g_x0.shape == (len(x0), mpc.nx) and g_th.shape == (len(x0), mpc.n_p)
            e_th, e_x = max(e_th, scaled(g_th, g12[key + "g_theta"][rows, c])), max(e_x, scaled(g_x0, g12[key + "g_x0"][rows, c]))
            w_th = max(w_th, scaled(g_th, np.roll(g12[key + "g_theta"][:, c], -1, 0)[rows]))
            w_x = max(w_x, scaled(g_x0, np.roll(g12[key + "g_x0"][:, c], -1, 0)[rows]))
        print(f"chain traj vjp n_mass {n_mass} N {N} {base} B {len(x0)}: du0*/dp {err_dp:.1e} -> bar {bar:.1e}, g_theta {e_th:.1e}, "
              f"g_x0 {e_x:.1e}; against the neighbour's rows {w_th:.1e} / {w_x:.1e}")
        assert e_th <= bar and e_x <= bar and w_th > bar and w_x > bar, (key, err_dp, bar, e_th, e_x, w_th, w_x)


# ---------------------------------------------------------------------- 2. inside the library
@pytest.mark.parametrize("n_mass,N", [(3, 10), (6, 3)])
def test_unit_cotangents_linearity_and_the_identity_term(n_mass, N):
    mpc = chain(n_mass, N, 4)
    r = mpc.solve(x0_near_ss(mpc, 4, 21), sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * 4
    J = policy(mpc, r.status)
    for c in range(3):      # e_{u_0, c}: row c of du0*/dp and of du0*/dx0, the same factorisation
        gU = torch.zeros((4, N, 3), dtype=torch.float64, device=mpc.device)
        gU[:, 0, c] = 1.0
        g_x0, g_th = raw(mpc, r.status, None, gU)
        e_th, e_x = scaled(g_th, r.dpi_dp[:, c]), scaled(g_x0, J[:, c])
        assert e_th <= RTOL and e_x <= RTOL, (c, e_th, e_x)
    gX, gU = normal_cotangent(mpc, 22)
    both, only_x, only_u = raw(mpc, r.status, gX, gU), raw(mpc, r.status, gX, None), raw(mpc, r.status, None, gU)
    for b, x, u in zip(both, only_x, only_u):      # one linear solve
        assert torch.isfinite(b).all() and float(b.abs().max()) > 0 and scaled(x + u, b) <= 1e-12
    g0 = torch.zeros_like(gX)      # a cotangent on x_0 alone: x_0 = x0 is the identity, nothing else sees it
    g0[:, 0] = gX[:, 0]
    g_x0, g_th = raw(mpc, r.status, g0, None)
    assert torch.equal(g_x0, gX[:, 0]) and torch.all(g_th == 0)
    # one output at a time gives the same bits
    assert torch.equal(bits(raw(mpc, r.status, gX, gU, theta=False)[0]), bits(both[0]))
    assert torch.equal(bits(raw(mpc, r.status, gX, gU, x0=False)[1]), bits(both[1]))


# ---------------------------------------------------------------------- 3. both routes and determinism
@pytest.mark.parametrize("n_mass,N", [(3, 10), (6, 3)])
def test_both_routes_agree_and_the_policy_call_is_left_alone(n_mass, N):
    """After a solve with sens_pi the exact Hessians are in the workspace; after a plain solve on the same inputs the call computes
    them first.  Equal within 1e-9; two calls in a row give the same bits; mpcrl_chain_policy_state_sens returns the same bits before
    and after."""
    got = []
    for sens_pi in (True, False):
        mpc = chain(n_mass, N, 4)
        r = mpc.solve(x0_near_ss(mpc, 4, 3), sens_pi=sens_pi, cold=True)
        gX, gU = normal_cotangent(mpc, 23)
        before = policy(mpc, r.status)
        a, b = raw(mpc, r.status, gX, gU), raw(mpc, r.status, gX, gU)
        after = policy(mpc, r.status)
        assert r.status.tolist() == [0] * 4 and all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in a)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b)), sens_pi
        assert torch.equal(bits(before), bits(after)), sens_pi
        got.append(a)
    assert scaled(got[1][0], got[0][0]) <= 1e-9 and scaled(got[1][1], got[0][1]) <= 1e-9


# ---------------------------------------------------------------------- 4. contract
def test_rows_are_written_in_full_and_the_solve_is_left_alone():
    mpc = chain(3, 10, 4)
    x0 = x0_near_ss(mpc, 4, 5)
    x0[2, 4] = float("nan")
    gX, gU = normal_cotangent(mpc, 24)
    for sens_pi in (True, False):      # both routes
        r = mpc.solve(x0, sens_v=True, sens_pi=sens_pi, cold=True)
        outs = [r.u0, r.V, r.status, r.iters, r.dV_dp] + ([r.dpi_dp] if sens_pi else [])
        before = [t.clone() for t in (*outs, *mpc.get_iterate(), mpc.get_lagrangian())]
        g_x0, g_th = raw(mpc, r.status, gX, gU)
        st = r.status.tolist()
        assert st[2] not in (0, 2) and [st[i] for i in (0, 1, 3)] == [0, 0, 0]
        for g in (g_x0, g_th):      # poisoned with NaN: every row was written
            assert torch.isfinite(g).all() and torch.all(g[2] == 0) and all(float(g[i].abs().max()) > 0 for i in (0, 1, 3))
        after = [*outs, *mpc.get_iterate(), mpc.get_lagrangian()]
        torch.cuda.synchronize()
        assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(before, after))      # (bytes: instance 2 holds NaN)
        p_x0, p_th = mpc.chain_trajectory_vjp(gX, gU)      # the Python surface: the same numbers
        assert torch.equal(bits(p_x0), bits(g_x0)) and torch.equal(bits(p_th), bits(g_th))
        assert mpc.chain_trajectory_vjp(gX, gU, theta=False)[1] is None and mpc.chain_trajectory_vjp(gX, gU, x0=False)[0] is None


def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, linear_system_ocp
    mpc = chain(3, 10, 2)
    x0 = x0_near_ss(mpc, 2, 7)
    gX, gU = normal_cotangent(mpc, 25)
    st = torch.zeros((2,), dtype=torch.int32, device=mpc.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, st, gX, gU)                                        # before any solve
    with pytest.raises(RuntimeError):
        mpc.chain_trajectory_vjp(gX, gU)
    # each setter that clears the library's flag (raw() goes past the Python mirror of it)
    idx = torch.arange(2, dtype=torch.int64, device=mpc.device)
    setters = (lambda it: mpc.set_iterate(*it[:4]), lambda it: mpc.set_theta(torch.as_tensor(mpc.ocp.p0)),
               lambda it: mpc.set_bounds(_lib.BOUNDS_U0, -0.9 * np.ones(3), 0.9 * np.ones(3)), lambda it: mpc.set_discount_factor(0.99),
               lambda it: mpc.set_iterate_rows(*it[:4], idx), lambda it: mpc.reset(x0))
    for touch in setters:
        r = mpc.solve(x0, cold=True)
        assert all(torch.isfinite(t).all() for t in raw(mpc, r.status, gX, gU))
        touch(mpc.get_iterate())
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, gX, gU)
        assert not mpc.chain_workspace_current
        with pytest.raises(RuntimeError):
            mpc.chain_trajectory_vjp(gX, gU)
    mpc.set_iterate(*mpc.get_iterate()[:4])
    with pytest.raises(RuntimeError, match="workspace of the last solve"):
        mpc.chain_trajectory_vjp(gX, gU)
    r = mpc.solve(x0, cold=True)
    assert mpc.chain_workspace_current
    for args in ((None, gX, gU, True, True), (r.status, None, None, True, True), (r.status, gX, gU, False, False)):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):      # status, both cotangents, both outputs NULL
            raw(mpc, args[0], args[1], args[2], x0=args[3], theta=args[4])
    for flags in (_lib.STATE_Q_MODE, 2):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, gX, gU, flags=flags)
    with pytest.raises(ValueError):
        mpc.chain_trajectory_vjp(None, None)
    with pytest.raises(ValueError):
        mpc.chain_trajectory_vjp(gX, gU, x0=False, theta=False)
    assert all(torch.isfinite(t).all() for t in raw(mpc, r.status, gX, gU))      # and the handle still answers
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):                     # the small models' call stays closed to the chain
        mpc._call("mpcrl_traj_vjp", 0, gX, gU, torch.zeros((2, mpc.nx), dtype=torch.float64, device=mpc.device), None)
    # after a solve with u0 fixed: flags = 0 answers (u_0 free at the pinned value), the Python method refuses
    r = mpc.solve(x0, np.full((2, 3), 0.1), cold=True)
    assert r.status.tolist() == [0, 0] and all(not (t == 7.0).any() for t in raw(mpc, r.status, gX, gU, fill=7.0))
    with pytest.raises(RuntimeError, match="Q mode"):
        mpc.chain_trajectory_vjp(gX, gU)
    lin = MPCBatch(linear_system_ocp(N=7), 2)
    rl = lin.solve(np.array([[0.5, 0.1], [0.3, 0.2]]), cold=True)
    kw = dict(dtype=torch.float64, device=lin.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        lin._call("mpcrl_chain_traj_vjp", 0, rl.status, torch.zeros((2, 8, 2), **kw), None, torch.zeros((2, 2), **kw), None)
    with pytest.raises(RuntimeError, match="chain of masses"):
        lin.chain_trajectory_vjp(torch.zeros((2, 8, 2), **kw), None)


# ---------------------------------------------------------------------- 5. graph capture
@pytest.mark.parametrize("sens_pi", [True, False])
def test_replays_inside_a_graph(sens_pi):
    mpc = chain(3, 10, 4)
    r = mpc.solve(x0_near_ss(mpc, 4, 9), sens_pi=sens_pi, cold=True)
    gX, gU = normal_cotangent(mpc, 26)
    want = raw(mpc, r.status, gX, gU)
    out = [torch.zeros_like(t) for t in want]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node chain: no parallel branches
        mpc._call("mpcrl_chain_traj_vjp", 0, r.status, gX, gU, out[0], out[1])
    torch.cuda.synchronize()
    assert all(torch.all(t == 0) for t in out)          # captured, not run
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(t), bits(w)) for t, w in zip(out, want))


# ---------------------------------------------------------------------- 6. the layer
def differences(f, z, entries, h=1e-5):
    """Central differences of the scalar f over the listed flat entries of z."""
    flat, g = z.reshape(-1), []
    for j in entries:
        keep = flat[j].item()
        flat[j] = keep + h
        fp = f(z)
        flat[j] = keep - h
        fm = f(z)
        flat[j] = keep
        g.append((fp - fm) / (2 * h))
    return np.array(g)


def test_layer_trajectory_on_the_chain():
    from mpc4rl_amd import MPCLayer
    B, N = 2, 6
    mpc = chain(3, N, B, tol=1e-10)
    ocp = mpc.ocp
    layer = MPCLayer(mpc, cold=True)
    rng = np.random.default_rng(27)
    x0 = torch.tensor(np.tile(ocp.consts, (B, 1)) + rng.normal(0.0, 0.01, (B, ocp.nx)), device="cuda", requires_grad=True)
    X_ref = torch.tensor(np.tile(ocp.consts, (B, N + 1, 1)) + rng.normal(0.0, 0.01, (B, N + 1, ocp.nx)), device="cuda")
    theta = torch.tensor(np.tile(ocp.p0, (B, 1)), device="cuda", requires_grad=True)      # per instance
    nl = 2
    cols = [0, nl, 4 * nl + 1, 7 * nl + 2]      # one entry each of m, D, L, C

    def loss(x, th):
        X, U = layer.trajectory(x, th)
        return ((X - X_ref) ** 2).sum() + (U ** 2).sum()

    calls, inner = [], mpc._call

    def recording(name, *args):
        calls.append(name)
        return inner(name, *args)

    mpc._call = recording
    loss(x0, theta).backward()      # no opt-in: one plain solve forward, one chain VJP backward
    mpc._call = inner
    assert calls.count("mpcrl_solve") == 1 and calls.count("mpcrl_chain_traj_vjp") == 1 and "mpcrl_traj_vjp" not in calls
    assert layer.last_status.tolist() == [0] * B and theta.grad.shape == (B, mpc.n_p)
    with torch.no_grad():
        xd, td = x0.detach().clone(), theta.detach().clone()
        gx = differences(lambda z: float(loss(z, td)), xd, range(B * ocp.nx)).reshape(B, ocp.nx)
        gt = differences(lambda z: float(loss(xd, z)), td, [b * mpc.n_p + c for b in range(B) for c in cols]).reshape(B, len(cols))
    e_x, e_t = scaled(x0.grad, gx), scaled(theta.grad[:, cols], gt)
    # a shared theta [n_p]: its gradient is the sum over the batch
    shared = torch.tensor(ocp.p0, device="cuda", requires_grad=True)
    loss(x0.detach(), shared).backward()
    e_s = scaled(shared.grad[None], theta.grad.sum(0, keepdim=True))
    print(f"layer trajectory chain n_mass 3 N {N}: d loss/d x0 {e_x:.1e}, d loss/d theta (m, D, L, C) {e_t:.1e}; shared theta against "
          f"the sum of the rows {e_s:.1e}")
    assert shared.grad.shape == (mpc.n_p,) and e_x <= 1e-5 and e_t <= 1e-5 and e_s <= 1e-9, (e_x, e_t, e_s)


MEASURED = """\
chain traj vjp n_mass 3 N 1 ss B 4: du0*/dp 1.6e-07 -> bar 1.0e-06, g_theta 1.7e-07, g_x0 1.7e-07; against the neighbour's rows 2.5e+00 / 2.4e+00
chain traj vjp n_mass 3 N 1 ss B 1: du0*/dp 1.6e-07 -> bar 1.0e-06, g_theta 1.6e-07, g_x0 1.7e-07; against the neighbour's rows 2.1e+00 / 2.1e+00
chain traj vjp n_mass 3 N 2 ss B 4: du0*/dp 3.2e-08 -> bar 1.0e-06, g_theta 3.9e-08, g_x0 4.0e-08; against the neighbour's rows 6.9e+00 / 4.2e+00
chain traj vjp n_mass 3 N 2 ss B 1: du0*/dp 3.1e-08 -> bar 1.0e-06, g_theta 3.1e-08, g_x0 4.0e-08; against the neighbour's rows 2.7e+00 / 2.6e+00
chain traj vjp n_mass 3 N 10 ss B 4: du0*/dp 3.9e-08 -> bar 1.0e-06, g_theta 7.6e-08, g_x0 4.4e-08; against the neighbour's rows 4.8e+00 / 2.6e+00
chain traj vjp n_mass 3 N 10 ss B 1: du0*/dp 3.5e-08 -> bar 1.0e-06, g_theta 4.4e-08, g_x0 4.2e-08; against the neighbour's rows 1.6e+00 / 1.4e+00
chain traj vjp n_mass 3 N 10 x0 B 4: du0*/dp 3.1e-08 -> bar 1.0e-06, g_theta 3.1e-08, g_x0 4.2e-08; against the neighbour's rows 3.0e+00 / 2.6e+00
chain traj vjp n_mass 3 N 10 x0 B 1: du0*/dp 3.1e-08 -> bar 1.0e-06, g_theta 3.1e-08, g_x0 4.2e-08; against the neighbour's rows 2.0e+00 / 1.9e+00
chain traj vjp n_mass 4 N 3 ss B 4: du0*/dp 1.3e-07 -> bar 1.0e-06, g_theta 2.9e-07, g_x0 2.4e-07; against the neighbour's rows 4.6e+00 / 1.8e+00
chain traj vjp n_mass 4 N 3 ss B 1: du0*/dp 6.9e-08 -> bar 1.0e-06, g_theta 2.9e-07, g_x0 1.8e-07; against the neighbour's rows 1.9e+00 / 1.8e+00
chain traj vjp n_mass 5 N 8 ss B 4: du0*/dp 4.3e-08 -> bar 1.0e-06, g_theta 2.5e-07, g_x0 3.6e-07; against the neighbour's rows 1.6e+00 / 1.8e+00
chain traj vjp n_mass 5 N 8 ss B 1: du0*/dp 3.8e-08 -> bar 1.0e-06, g_theta 1.7e-07, g_x0 3.4e-07; against the neighbour's rows 1.6e+00 / 1.8e+00
chain traj vjp n_mass 6 N 3 ss B 4: du0*/dp 4.4e-08 -> bar 1.0e-06, g_theta 3.5e-07, g_x0 3.0e-07; against the neighbour's rows 4.1e+00 / 2.6e+00
chain traj vjp n_mass 6 N 3 ss B 1: du0*/dp 4.4e-08 -> bar 1.0e-06, g_theta 1.2e-07, g_x0 3.0e-07; against the neighbour's rows 1.9e+00 / 2.6e+00
chain traj vjp n_mass 7 N 5 ss B 4: du0*/dp 9.1e-08 -> bar 1.0e-06, g_theta 4.7e-07, g_x0 4.4e-07; against the neighbour's rows 3.6e+00 / 1.9e+00
chain traj vjp n_mass 7 N 5 ss B 1: du0*/dp 8.4e-08 -> bar 1.0e-06, g_theta 2.0e-07, g_x0 2.9e-07; against the neighbour's rows 1.3e+00 / 1.8e+00
chain traj vjp n_mass 3 N 10 act B 4: du0*/dp 2.8e-08 -> bar 1.0e-06, g_theta 6.8e-08, g_x0 1.4e-07; against the neighbour's rows 3.5e+00 / 2.4e+00
chain traj vjp n_mass 3 N 10 act B 1: du0*/dp 9.6e-09 -> bar 1.0e-06, g_theta 2.2e-08, g_x0 7.4e-08; against the neighbour's rows 2.8e+00 / 2.4e+00
layer trajectory chain n_mass 3 N 6: d loss/d x0 3.8e-09, d loss/d theta (m, D, L, C) 1.7e-06; shared theta against the sum of the rows 0.0e+00
"""
