"""mpcrl_chain_bound_vjp and mpcrl_bound_value_grad (include/mpcrl_bound_ext.h) on the chain of masses: the derivatives of the planned
trajectory and of the value with respect to the box bounds (chain_bound_out_kernel on the solution of chain_traj_riccati_kernel;
bound_value_grad_kernel) against the mirror fixture G13 (tests/golden/make_bound_vjp.py), the known answer on active rows, the bits of
mpcrl_chain_traj_vjp, the two launch routes, the call's contract and refusals, graph capture and the autograd layer.

Bars.  Against the fixture: max(1e-6, 4 x the error of the same solve's du0*/dp against the mirror's du0*/dp), the bar and the
scaling (rows by max(|reference row|, 1), a row an instance's whole [N + 1, nu + nx] gradient) of tests/test_gpu_chain_traj_vjp.py.
The two routes: 1e-12 of each other (the Hessians are recomputed in the same order; measured: the same bits).  The
layer against central differences of its own forward pass at h = 1e-5: 1e-5.

Measured on an MI355X: MEASURED at the end of this file (every line the tests print).
"""
import os

import numpy as np
import pytest
import torch

import small_mode_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = C.RTOL
SETS = ((3, 10, "act"), (3, 10, "x0"), (5, 8, "ss"))


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_bound_vjp.npz"))


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


def same(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def split(mpc, G):
    G = torch.as_tensor(np.asarray(G), dtype=torch.float64, device=mpc.device)
    nU = mpc.N * mpc.nu
    return G[:, nU:].reshape(mpc.B, mpc.N + 1, mpc.nx).contiguous(), G[:, :nU].reshape(mpc.B, mpc.N, mpc.nu).contiguous()


def raw(mpc, status, gX, gU, want=(True, True, True, True), flags=0, fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    nb = (mpc.B, mpc.N + 1, mpc.nu + mpc.nx)
    bufs = [torch.full(sh, fill, **kw) if w else None for sh, w in zip(((mpc.B, mpc.nx), (mpc.B, mpc.n_p), nb, nb), want)]
    mpc._call("mpcrl_chain_bound_vjp", flags, status, gX, gU, *bufs)
    torch.cuda.synchronize()
    return bufs


def raw_traj(mpc, status, gX, gU):
    kw = dict(dtype=torch.float64, device=mpc.device)
    out = [torch.full((mpc.B, mpc.nx), float("nan"), **kw), torch.full((mpc.B, mpc.n_p), float("nan"), **kw)]
    mpc._call("mpcrl_chain_traj_vjp", 0, status, gX, gU, *out)
    torch.cuda.synchronize()
    return out


def policy(mpc, status):
    out = torch.full((mpc.B, mpc.nu, mpc.nx), float("nan"), dtype=torch.float64, device=mpc.device)
    mpc._call("mpcrl_chain_policy_state_sens", 0, status, out)
    torch.cuda.synchronize()
    return out


def x0_act(mpc, B, seed):
    """x0 of the fixture's set m3_N10_act: x0_default + N(0, 0.2), where control rows are active."""
    return np.tile(mpc.ocp.x0, (B, 1)) + np.random.default_rng(seed).normal(0.0, 0.2, (B, mpc.nx))


def normal_cotangent(mpc, seed):
    return split(mpc, np.random.default_rng(seed).standard_normal((mpc.B, mpc.N * mpc.nu + (mpc.N + 1) * mpc.nx)))


# ---------------------------------------------------------------------- 1. against the fixture
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_bound_vjp_against_the_mirror(g13, n_mass, N, base):
    """Cold solve at tol 1e-9 with sens_pi on the fixture's x0 (default bounds |u| <= 1), all four instances and then the first alone;
    the fixture's three cotangents; dV/db against the fixture and equal to the stored multipliers on the rows that exist.  The structural
    zeros (every state coordinate: the chain has no state bounds; the controls of stage N) are exact."""
    key = f"m{n_mass}_N{N}_{base}_"
    for rows in (slice(0, 4), slice(0, 1)):
        x0 = g13[key + "x0"][rows]
        mpc = chain(n_mass, N, len(x0))
        r = mpc.solve(x0, sens_pi=True, cold=True)
        assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
        ref_dp = g13[key + "dpi_dp"][rows]
        err_dp = scaled(r.dpi_dp, ref_dp)
        bar = max(RTOL, 4.0 * err_dp)
        e = []
        for c in range(3):
            gX, gU = split(mpc, g13[key + "G"][rows, c])
            _, _, g_lb, g_ub = mpc.bound_vjp(gX, gU, x0=False, theta=False)
            assert torch.all(g_lb[:, :, 3:] == 0) and torch.all(g_ub[:, :, 3:] == 0) and torch.all(g_lb[:, N] == 0) and torch.all(g_ub[:, N] == 0)
            e.append(scaled(torch.stack([g_lb, g_ub], 1), np.stack([g13[key + "g_lb"][rows, c], g13[key + "g_ub"][rows, c]], 1)))
        dlb, dub = mpc.bound_value_grad()
        bnd = mpc.get_iterate()[3]
        assert torch.equal(dlb[:, :N, :3], bnd[:, 0, :N, :3]) and torch.equal(dub[:, :N, :3], -bnd[:, 1, :N, :3])
        assert torch.all(dlb[:, :, 3:] == 0) and torch.all(dub[:, :, 3:] == 0) and torch.all(dlb[:, N] == 0) and torch.all(dub[:, N] == 0)
        e_V = scaled(torch.stack([dlb, dub], 1), np.stack([g13[key + "dV_dlb"][rows], g13[key + "dV_dub"][rows]], 1))
        print(f"chain bound vjp n_mass {n_mass} N {N} {base} B {len(x0)}: du0*/dp {err_dp:.1e} -> bar {bar:.1e}; g_lb, g_ub "
              f"{' '.join(f'{v:.1e}' for v in e)}; dV/dlb, dV/dub {e_V:.1e}")
        assert max(e) <= bar and e_V <= bar, (key, bar, e, e_V)


def test_known_answer_on_the_active_rows(g13):
    """m3_N10_act: a unit cotangent on a control the fixture marks as sitting on its bound, at a stage >= 1 and at stage 0, gives 1
    with respect to that row's active side and 0 with respect to the other, within the bar of the fixture test."""
    key, N = "m3_N10_act_", 10
    x0 = g13[key + "x0"]
    act = np.stack([g13[key + "act_lb"][:, :, :3], g13[key + "act_ub"][:, :, :3]], 1)      # [B, side, stage, control]
    mpc = chain(3, N, 4)
    r = mpc.solve(x0, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * 4
    bar = max(RTOL, 4.0 * scaled(r.dpi_dp, g13[key + "dpi_dp"]))
    worst, seen = {}, {}
    for name, stages in (("stage >= 1", range(1, N)), ("stage 0", range(0, 1))):
        pick = [next(((k, sd, c) for k in stages for sd in (0, 1) for c in range(3) if act[i, sd, k, c]), None) for i in range(4)]
        gU = torch.zeros((4, N, 3), dtype=torch.float64, device=mpc.device)
        for i, p in enumerate(pick):
            if p is not None:
                gU[i, p[0], p[2]] = 1.0
        g = torch.stack(mpc.bound_vjp(None, gU, x0=False, theta=False)[2:], 1).cpu().numpy()
        dev = [abs(g[i, p[1], p[0], p[2]] - 1.0) for i, p in enumerate(pick) if p is not None]
        dev += [abs(g[i, 1 - p[1], p[0], p[2]]) for i, p in enumerate(pick) if p is not None]
        worst[name], seen[name] = max(dev), len(dev) // 2
    print(f"chain bound vjp m3_N10_act known answer: |g - 1| on the active side, |g| on the other: stage >= 1 ({seen['stage >= 1']}) "
          f"{worst['stage >= 1']:.1e}; stage 0 ({seen['stage 0']}) {worst['stage 0']:.1e}; bar {bar:.1e}")
    assert seen["stage >= 1"] == 4 and seen["stage 0"] >= 1 and max(worst.values()) <= bar


# ---------------------------------------------------------------------- 2. the bits of the trajectory VJP, both routes
@pytest.mark.parametrize("sens_pi", [True, False])
def test_bits_of_the_trajectory_vjp_and_the_other_calls_are_left_alone(sens_pi):
    """With the bound outputs NULL the call is mpcrl_chain_traj_vjp; with them requested g_x0 and g_theta keep those bits, each bound
    output alone gives the bits it has among all four, two calls give the same bits, and mpcrl_chain_policy_state_sens and
    mpcrl_chain_traj_vjp return the same bits before and after."""
    mpc = chain(3, 10, 4)
    r = mpc.solve(x0_act(mpc, 4, 31), sens_pi=sens_pi, cold=True)
    assert r.status.tolist() == [0] * 4
    gX, gU = normal_cotangent(mpc, 32)
    pol, traj = policy(mpc, r.status), raw_traj(mpc, r.status, gX, gU)
    full, again = raw(mpc, r.status, gX, gU), raw(mpc, r.status, gX, gU)
    assert all(torch.isfinite(t).all() for t in full) and float(full[2].abs().max()) > 1e-3 and same(full, again)
    assert same(full[:2], traj) and same(raw(mpc, r.status, gX, gU, (True, True, False, False))[:2], traj)
    assert same(raw(mpc, r.status, gX, gU, (False, False, True, False))[2:3], full[2:3])
    assert same(raw(mpc, r.status, gX, gU, (False, True, False, True))[1::2], full[1::2])
    assert same((policy(mpc, r.status),), (pol,)) and same(raw_traj(mpc, r.status, gX, gU), traj)
    for a, b in ((gX, None), (None, gU)):      # a NULL cotangent counts as zeros
        za, zb = (torch.zeros_like(gX) if a is None else a), (torch.zeros_like(gU) if b is None else b)
        assert same(raw(mpc, r.status, a, b), raw(mpc, r.status, za, zb))
    assert same(mpc.bound_vjp(gX, gU), full)      # the Python surface: the same numbers


def test_both_routes_agree():
    """After a solve with sens_pi the exact Hessians are in the workspace (4 launches with the bound outputs); after a plain solve the
    call computes them first (6)."""
    got = []
    for sens_pi in (True, False):
        mpc = chain(3, 10, 4)
        r = mpc.solve(x0_act(mpc, 4, 33), sens_pi=sens_pi, cold=True)
        assert r.status.tolist() == [0] * 4
        got.append(raw(mpc, r.status, *normal_cotangent(mpc, 34)))
    e = [scaled(a, b) for a, b in zip(got[1], got[0])]
    print(f"chain bound vjp m3 N 10 the two routes: g_x0 {e[0]:.1e}, g_theta {e[1]:.1e}, g_lb {e[2]:.1e}, g_ub {e[3]:.1e}")
    assert max(e) <= 1e-12


# ---------------------------------------------------------------------- 3. contract
def test_rows_of_other_statuses_are_zero_and_the_solve_is_left_alone():
    mpc = chain(3, 10, 4)
    x0 = x0_act(mpc, 4, 35)
    x0[2, 4] = float("nan")
    gX, gU = normal_cotangent(mpc, 36)
    r = mpc.solve(x0, sens_v=True, cold=True)
    outs = [r.u0, r.V, r.status, r.iters, r.dV_dp]
    before = [t.clone() for t in (*outs, *mpc.get_iterate(), mpc.get_lagrangian())]
    full = raw(mpc, r.status, gX, gU)
    dlb, dub = mpc.bound_value_grad()
    st = r.status.tolist()
    assert st[2] not in (0, 2) and [st[i] for i in (0, 1, 3)] == [0, 0, 0]
    for g in full + [dlb, dub]:      # poisoned with NaN: every row was written
        assert torch.isfinite(g).all() and torch.all(g[2] == 0) and all(float(g[i].abs().max()) > 0 for i in (0, 1, 3))
    after = [*outs, *mpc.get_iterate(), mpc.get_lagrangian()]
    torch.cuda.synchronize()
    assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(before, after))


def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, cartpole_ocp
    mpc = chain(3, 10, 2)
    x0 = x0_act(mpc, 2, 37)
    gX, gU = normal_cotangent(mpc, 38)
    st = torch.zeros((2,), dtype=torch.int32, device=mpc.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, st, gX, gU)                                        # before any solve
    with pytest.raises(RuntimeError):
        mpc.bound_vjp(gX, gU)
    for touch in (lambda: mpc.set_bounds(_lib.BOUNDS_U0, -0.9 * np.ones(3), 0.9 * np.ones(3)), lambda: mpc.set_theta(torch.as_tensor(mpc.ocp.p0))):
        r = mpc.solve(x0, cold=True)
        assert all(torch.isfinite(t).all() for t in raw(mpc, r.status, gX, gU))
        touch()                                                     # the workspace no longer describes the handle
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, gX, gU)
        with pytest.raises(RuntimeError, match="workspace of the last solve"):
            mpc.bound_vjp(gX, gU)
    r = mpc.solve(x0, cold=True)
    for args in ((None, gX, gU, (True,) * 4), (r.status, None, None, (True,) * 4), (r.status, gX, gU, (False,) * 4)):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):      # status, both cotangents, all outputs NULL
            raw(mpc, args[0], args[1], args[2], args[3])
    for flags in (_lib.STATE_Q_MODE, 2):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, gX, gU, flags=flags)
    assert all(torch.isfinite(t).all() for t in raw(mpc, r.status, gX, gU))      # and the handle still answers
    cp = MPCBatch(cartpole_ocp(N=6, tf=0.6), 2)
    rc = cp.solve(np.array([[0.1, 0.0, 0.1, 0.0], [0.2, 0.0, -0.1, 0.0]]), cold=True)
    kw = dict(dtype=torch.float64, device=cp.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        cp._call("mpcrl_chain_bound_vjp", 0, rc.status, torch.zeros((2, 7, 4), **kw), None, torch.zeros((2, 4), **kw), None, None, None)


# ---------------------------------------------------------------------- 4. graph capture
@pytest.mark.parametrize("sens_pi", [True, False])
def test_replays_inside_a_graph(sens_pi):
    mpc = chain(3, 10, 4)
    r = mpc.solve(x0_act(mpc, 4, 39), sens_pi=sens_pi, cold=True)
    gX, gU = normal_cotangent(mpc, 40)
    want = raw(mpc, r.status, gX, gU)
    out = [torch.zeros_like(t) for t in want]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node chain: no parallel branches
        mpc._call("mpcrl_chain_bound_vjp", 0, r.status, gX, gU, *out)
    torch.cuda.synchronize()
    assert all(torch.all(t == 0) for t in out)          # captured, not run
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, want)


# ---------------------------------------------------------------------- 5. the layer
def test_layer_bounds_on_the_chain():
    """n_mass 3, N 10, x0 of the active set: d loss / d bounds of ``trajectory`` and of ``forward`` over the control bounds (the state
    bounds are absent: +-1e30 is no place to difference) against central differences of the layer's own forward pass."""
    from mpc4rl_amd import BoxBounds, MPCLayer
    B, N = 2, 10
    mpc = chain(3, N, B, tol=1e-10)
    ocp = mpc.ocp
    layer = MPCLayer(mpc, cold=True)
    rng = np.random.default_rng(41)
    x0 = torch.tensor(x0_act(mpc, B, 42), device="cuda")
    theta = torch.tensor(ocp.p0, device="cuda")
    Wx, Wu = torch.tensor(rng.uniform(-1, 1, (B, N + 1, ocp.nx)), device="cuda"), torch.tensor(rng.uniform(-1, 1, (B, N, 3)), device="cuda")
    wu, wV = torch.tensor(rng.uniform(-1, 1, (B, 3)), device="cuda"), torch.tensor(rng.uniform(-1, 1, B), device="cuda")
    inf = [1e30] * ocp.nx

    def box(lb0, ub0, lbu, ubu):
        f = dict(dtype=torch.float64)
        return BoxBounds(lb0, ub0, torch.cat([lbu, -torch.tensor(inf, **f)]), torch.cat([ubu, torch.tensor(inf, **f)]),
                         -torch.tensor(inf, **f), torch.tensor(inf, **f))

    def traj_loss(b):
        X, U = layer.trajectory(x0, theta, b)
        return (Wx * X).sum() + (Wu * U).sum()

    def fwd_loss(b):
        u0, V = layer(x0, theta, b)
        return (wu * u0).sum() + (wV * V).sum()

    for name, loss in (("trajectory", traj_loss), ("forward", fwd_loss)):
        leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in ([-1.0] * 3, [1.0] * 3, [-1.0] * 3, [1.0] * 3)]
        calls, inner = [], mpc._call

        def recording(fn, *args):
            calls.append(fn)
            return inner(fn, *args)

        mpc._call = recording
        loss(box(*leaves)).backward()
        mpc._call = inner
        assert calls.count("mpcrl_solve") == 1 and calls.count("mpcrl_chain_bound_vjp") == 1 and "mpcrl_chain_traj_vjp" not in calls
        assert layer.last_status.tolist() == [0] * B
        assert float(mpc.get_iterate()[3][:, 2:4, :N, :3].min()) < 1e-8      # a control row is active
        errs = []
        with torch.no_grad():
            for i, leaf in enumerate(leaves):
                z = [v.detach().clone() for v in leaves]
                g = np.zeros(3)
                for j in range(3):
                    for sgn in (1.0, -1.0):
                        z[i][j] = leaves[i][j].item() + sgn * 1e-5
                        g[j] += sgn * float(loss(box(*z))) / 2e-5
                    z[i][j] = leaves[i][j].item()
                errs.append(scaled(leaf.grad[None], g[None]))
        print(f"layer.{name} chain n_mass 3 N {N} with bounds: d loss/d (lb0 ub0 lbu ubu) {' '.join(f'{v:.1e}' for v in errs)}; "
              f"largest |gradient| {max(float(v.grad.abs().max()) for v in leaves):.2e}")
        assert max(float(v.grad.abs().max()) for v in leaves) > 1e-2 and max(errs) <= 1e-5


MEASURED = """\
chain bound vjp n_mass 3 N 10 act B 4: du0*/dp 6.7e-08 -> bar 1.0e-06; g_lb, g_ub 8.2e-08 8.7e-08 8.1e-10; dV/dlb, dV/dub 8.4e-10
chain bound vjp n_mass 3 N 10 act B 1: du0*/dp 1.8e-08 -> bar 1.0e-06; g_lb, g_ub 8.2e-08 8.7e-08 2.9e-10; dV/dlb, dV/dub 1.1e-10
chain bound vjp n_mass 3 N 10 x0 B 4: du0*/dp 3.1e-08 -> bar 1.0e-06; g_lb, g_ub 2.4e-08 3.2e-08 2.6e-09; dV/dlb, dV/dub 1.5e-10
chain bound vjp n_mass 3 N 10 x0 B 1: du0*/dp 3.1e-08 -> bar 1.0e-06; g_lb, g_ub 2.4e-08 1.6e-09 2.6e-09; dV/dlb, dV/dub 3.9e-11
chain bound vjp n_mass 5 N 8 ss B 4: du0*/dp 4.3e-08 -> bar 1.0e-06; g_lb, g_ub 1.7e-10 1.2e-10 7.8e-12; dV/dlb, dV/dub 3.6e-12
chain bound vjp n_mass 5 N 8 ss B 1: du0*/dp 3.8e-08 -> bar 1.0e-06; g_lb, g_ub 1.7e-10 7.9e-11 7.6e-12; dV/dlb, dV/dub 3.4e-12
chain bound vjp m3_N10_act known answer: |g - 1| on the active side, |g| on the other: stage >= 1 (4) 5.0e-10; stage 0 (4) 8.1e-10; bar 1.0e-06
chain bound vjp m3 N 10 the two routes: g_x0 0.0e+00, g_theta 0.0e+00, g_lb 0.0e+00, g_ub 0.0e+00
layer.trajectory chain n_mass 3 N 10 with bounds: d loss/d (lb0 ub0 lbu ubu) 3.0e-09 1.0e-09 6.3e-10 3.7e-09; largest |gradient| 3.84e+00
layer.forward chain n_mass 3 N 10 with bounds: d loss/d (lb0 ub0 lbu ubu) 5.4e-10 5.4e-10 2.6e-10 1.1e-09; largest |gradient| 1.26e+00
"""
