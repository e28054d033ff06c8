"""mpcrl_chain_traj_jvp (include/mpcrl_chain_traj_jvp_ext.h) on the device: the trajectory Jacobian-vector product of the chain of
masses from one primal Riccati solve per direction (chain_jvp_rhs_kernel, chain_traj_jvp_riccati_kernel) against the mirror fixture
G16 (tests/golden/make_chain_traj_jvp.py), against the library's own trajectory VJP (the adjoint identity), du0*/dx0 and du0*/dp, the
independence of a result from the other directions and the batch, what the call leaves alone, its contract and refusals, graph
capture and the Jacobian built from it.

Bars.  Against the fixture: max(1e-6, 4 x the error of the same solve's du0*/dp against the mirror's du0*/dp) — another right-hand
side on one factorisation, the rule of tests/test_gpu_chain_traj_vjp.py and tests/test_gpu_chain_state_sens.py; 1e-6 is RTOL of
tests/small_mode_cases.py and the fixture's gate.  Per direction over the whole of dW = (dU, dX), scaled by max(|dW|_inf, 1), the
fixture's own scale.  The adjoint identity <G, JVP(v)> = g_x0 . vx + g_theta . vp: 1e-6 x max(sum |G_i dW_i|, 1) — both sides are
within that of the mirror.  u_0 rows against du0*/dx0 and du0*/dp of the same workspace: 1e-6, rows scaled by max(|row|, 1).  The two
routes (Hessians left by the solve / recomputed): 1e-9.  Everything else is torch.equal.

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
G10_SETS = ((3, 1, "ss"), (3, 2, "ss"), (3, 10, "ss"), (3, 10, "x0"), (4, 3, "ss"), (5, 8, "ss"), (6, 3, "ss"), (7, 5, "ss"))
SETS = G10_SETS + ((3, 10, "act"),)


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(ROOT, "tests", "golden", "g16_chain_traj_jvp.npz"))


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


def dev(mpc, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64, device=mpc.device).contiguous()


def w_of(dX, dU):
    """(dX [B, R, N+1, nx], dU [B, R, N, nu]) -> dW [B * R, nw] in the mirror's order [U; X], one row per (instance, direction)."""
    dX, dU = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (dX, dU))
    B, R = dX.shape[:2]
    return np.concatenate([dU.reshape(B * R, -1), dX.reshape(B * R, -1)], 1)


def raw(mpc, status, ndir, dx0, dtheta, X=True, U=True, flags=0, fill=float("nan")):
    """The library call itself on buffers poisoned with ``fill``."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    n = max(ndir, 1)
    dX = torch.full((mpc.B, n, mpc.N + 1, mpc.nx), fill, **kw) if X else None
    dU = torch.full((mpc.B, n, mpc.N, mpc.nu), fill, **kw) if U else None
    mpc._call("mpcrl_chain_traj_jvp", flags, status, ndir, dx0, dtheta, dX, dU)
    torch.cuda.synchronize()
    return dX, dU


def policy(mpc, status):
    out = torch.full((mpc.B, mpc.nu, mpc.nx), float("nan"), dtype=torch.float64, device=mpc.device)
    mpc._call("mpcrl_chain_policy_state_sens", 0, status, out)
    torch.cuda.synchronize()
    return out


def x0_near_ss(mpc, B, seed):
    return np.tile(mpc.ocp.consts, (B, 1)) + np.random.default_rng(seed).normal(0.0, 0.01, (B, mpc.nx))


def normal_directions(mpc, R, seed):
    rng = np.random.default_rng(seed)
    return dev(mpc, rng.standard_normal((mpc.B, R, mpc.nx))), dev(mpc, rng.standard_normal((mpc.B, R, mpc.n_p)))


def normal_cotangent(mpc, seed):
    rng = np.random.default_rng(seed)
    return dev(mpc, rng.standard_normal((mpc.B, mpc.N + 1, mpc.nx))), dev(mpc, rng.standard_normal((mpc.B, mpc.N, mpc.nu)))


# ---------------------------------------------------------------------- 1. against the fixture
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_jvp_against_the_mirror(g16, g12, g10, n_mass, N, base):
    """Cold solve at tol 1e-9 with sens_pi on the fixture's x0, the kept instances together and then the first alone (B = 1); the
    fixture's three directions in one call.  Negative control: against the fixture rows of the neighbouring instance the error must
    exceed the bar."""
    key = f"m{n_mass}_N{N}_{base}_"
    idx = g16[key + "idx"]
    for rows in (slice(0, len(idx)), slice(0, 1)):
        x0 = g16[key + "x0"][rows]
        mpc = chain(n_mass, N, len(x0))
        r = mpc.solve(x0, sens_pi=True, cold=True)
        torch.cuda.synchronize()
        assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
        # the mirror's du0*/dp: all of it in G10; for the set G10 does not have, its row 0 (G12's unit cotangent)
        err_dp = (scaled(r.dpi_dp, g10[key + "dpi_dp"][idx[rows]]) if base != "act"
                  else scaled(r.dpi_dp[:, 0], g12[key + "g_theta"][idx[rows], 2]))
        bar = max(RTOL, 4.0 * err_dp)
        dX, dU = mpc.chain_trajectory_jvp(g16[key + "vx"][rows], g16[key + "vp"][rows])
        assert dX.shape == (len(x0), 3, N + 1, mpc.nx) and dU.shape == (len(x0), 3, N, mpc.nu)
        assert torch.equal(dX[:, :, 0], dev(mpc, g16[key + "vx"][rows]))      # x_0 = x0
        got, ref = w_of(dX, dU), w_of(g16[key + "dX"][rows], g16[key + "dU"][rows])
        nb = w_of(np.roll(g16[key + "dX"], -1, 0)[rows], np.roll(g16[key + "dU"], -1, 0)[rows])
        err = [scaled(got[d::3], ref[d::3]) for d in range(3)]
        wrong = [scaled(got[d::3], nb[d::3]) for d in range(3)]
        print(f"chain traj jvp n_mass {n_mass} N {N} {base} B {len(x0)}: du0*/dp {err_dp:.1e} -> bar {bar:.1e}, dW "
              f"{err[0]:.1e} / {err[1]:.1e} / {err[2]:.1e}; against the neighbour's rows {min(wrong):.1e}")
        assert max(err) <= bar and min(wrong) > bar, (key, err_dp, bar, err, wrong)


# ---------------------------------------------------------------------- 2. the adjoint identity inside the library
@pytest.mark.parametrize("n_mass,N,own_theta", [(3, 10, False), (5, 8, False), (7, 5, False), (3, 10, True)])
def test_adjoint_identity_with_the_trajectory_vjp(n_mass, N, own_theta):
    """<G, JVP(v)> = g_x0 . vx + g_theta . vp with chain_trajectory_vjp on the same workspace; cotangents and directions standard
    normal over all of w, x0 and p.  The right-hand side of the JVP is the exact transpose of what the VJP contracts, so the identity
    pins every sign and coefficient of the new kernels.  Once with a theta per instance (m, D x U(0.95, 1.05))."""
    B = 4
    mpc = chain(n_mass, N, B)
    if own_theta:
        th = np.tile(mpc.ocp.p0, (B, 1))
        nl = n_mass - 1
        th[:, :4 * nl] *= np.random.default_rng(31).uniform(0.95, 1.05, (B, 4 * nl))
        mpc.set_theta(torch.as_tensor(th))
    r = mpc.solve(x0_near_ss(mpc, B, 32), sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * B
    gX, gU = normal_cotangent(mpc, 33)
    vx, vp = normal_directions(mpc, 2, 34)
    g_x0, g_th = mpc.chain_trajectory_vjp(gX, gU)
    dX, dU = mpc.chain_trajectory_jvp(vx, vp)
    lhs = (gX[:, None] * dX).sum((2, 3)) + (gU[:, None] * dU).sum((2, 3))
    rhs = (g_x0[:, None] * vx).sum(2) + (g_th[:, None] * vp).sum(2)
    scale = ((gX[:, None] * dX).abs().sum((2, 3)) + (gU[:, None] * dU).abs().sum((2, 3))).clamp(min=1.0)
    worst = float(((lhs - rhs).abs() / scale).max())
    print(f"chain traj jvp adjoint identity n_mass {n_mass} N {N}{' theta per instance' if own_theta else ''}: {worst:.1e}")
    assert torch.isfinite(lhs).all() and float(lhs.abs().min()) > 0 and worst <= 1e-6, worst


# ---------------------------------------------------------------------- 3. the rows of u_0
@pytest.mark.parametrize("n_mass,N", [(3, 10), (6, 3)])
def test_rows_of_u0_are_the_policy_sensitivities(n_mass, N):
    """Unit directions on x0: the u_0 rows of dU are du0*/dx0 (mpcrl_chain_policy_state_sens).  Unit directions on entries of every
    block of p (m, D, L, C, Q, R, w): they are the columns of the solve's dpi_dp."""
    B = 2
    mpc = chain(n_mass, N, B)
    r = mpc.solve(x0_near_ss(mpc, B, 41), sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * B
    J = policy(mpc, r.status)
    nx, nl = mpc.nx, n_mass - 1
    off_q = 10 * nl
    off_r = off_q + nx * nx
    cols = [0, nl - 1, nl, 4 * nl + 1, 7 * nl + 2, off_q, off_q + 1, off_q + nx * nx - 1, off_r, off_r + 4, off_r + 9, mpc.n_p - 1]
    eye = torch.eye(nx, dtype=torch.float64, device=mpc.device).expand(B, nx, nx).contiguous()
    _, dU = mpc.chain_trajectory_jvp(eye, None)
    e_x = scaled(dU[:, :, 0].transpose(1, 2), J)
    dth = torch.zeros((B, len(cols), mpc.n_p), dtype=torch.float64, device=mpc.device)
    dth[:, torch.arange(len(cols)), torch.as_tensor(cols)] = 1.0
    _, dU = mpc.chain_trajectory_jvp(None, dth)
    e_p = scaled(dU[:, :, 0].transpose(1, 2), r.dpi_dp[:, :, cols])
    assert float(dU.abs().amax((0, 2, 3)).min()) > 0      # every block moves the plan
    print(f"chain traj jvp u_0 rows n_mass {n_mass} N {N}: against du0*/dx0 {e_x:.1e}, against dpi_dp {e_p:.1e}")
    assert e_x <= RTOL and e_p <= RTOL, (e_x, e_p)


# ---------------------------------------------------------------------- 4. same bits
def test_a_result_does_not_depend_on_the_other_directions_or_the_batch():
    n_mass, N, B = 3, 10, 4
    x0 = x0_near_ss(chain(n_mass, N, 1), B, 51)
    mpc = chain(n_mass, N, B)
    r = mpc.solve(x0, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * B
    vx, vp = normal_directions(mpc, 17, 52)
    X17, U17 = raw(mpc, r.status, 17, vx, vp)
    assert torch.isfinite(X17).all() and torch.isfinite(U17).all()
    for R_ in (1, 3):      # ndir 1 against 3 against 17
        Xr, Ur = raw(mpc, r.status, R_, vx[:, :R_].contiguous(), vp[:, :R_].contiguous())
        assert torch.equal(bits(Xr), bits(X17[:, :R_])) and torch.equal(bits(Ur), bits(U17[:, :R_]))
    # a direction placed last instead of first
    flip = lambda t: torch.flip(t, (1,)).contiguous()
    Xf, Uf = raw(mpc, r.status, 17, flip(vx), flip(vp))
    assert torch.equal(bits(flip(Xf)), bits(X17)) and torch.equal(bits(flip(Uf)), bits(U17))
    # one input NULL is that input zero
    Xz, Uz = raw(mpc, r.status, 3, None, vp[:, :3].contiguous())
    X0, U0 = raw(mpc, r.status, 3, torch.zeros_like(vx[:, :3]), vp[:, :3].contiguous())
    assert torch.equal(bits(Xz), bits(X0)) and torch.equal(bits(Uz), bits(U0))
    # one output at a time
    assert torch.equal(bits(raw(mpc, r.status, 3, vx[:, :3].contiguous(), vp[:, :3].contiguous(), U=False)[0]), bits(X17[:, :3]))
    assert torch.equal(bits(raw(mpc, r.status, 3, vx[:, :3].contiguous(), vp[:, :3].contiguous(), X=False)[1]), bits(U17[:, :3]))
    # B = 4 against B = 1
    one = chain(n_mass, N, 1)
    r1 = one.solve(x0[2:3], sens_pi=True, cold=True)
    X1, U1 = raw(one, r1.status, 3, vx[2:3, :3].contiguous(), vp[2:3, :3].contiguous())
    assert torch.equal(bits(X1), bits(X17[2:3, :3])) and torch.equal(bits(U1), bits(U17[2:3, :3]))
    # after a plain solve the call computes the Hessians first: the same numbers to 1e-9 (bit equality is not promised)
    plain = chain(n_mass, N, B)
    rp = plain.solve(x0, cold=True)
    Xp, Up = raw(plain, rp.status, 3, vx[:, :3].contiguous(), vp[:, :3].contiguous())
    Xq, Uq = raw(plain, rp.status, 3, vx[:, :3].contiguous(), vp[:, :3].contiguous())
    assert torch.equal(bits(Xp), bits(Xq)) and torch.equal(bits(Up), bits(Uq))
    e = max(scaled(Xp.reshape(B * 3, -1), X17[:, :3].reshape(B * 3, -1)), scaled(Up.reshape(B * 3, -1), U17[:, :3].reshape(B * 3, -1)))
    assert e <= 1e-9, e


# ---------------------------------------------------------------------- 5. left alone
@pytest.mark.parametrize("sens_pi", [True, False])
def test_the_call_leaves_the_handle_as_it_was(sens_pi):
    """Around a JVP call: mpcrl_chain_policy_state_sens and chain_trajectory_vjp return the same bits, the solve's outputs, the
    iterate and the Lagrangian are untouched, and a following warm solve is the one of a twin handle that made no JVP call."""
    n_mass, N, B = 4, 6, 3
    mpc, twin = chain(n_mass, N, B), chain(n_mass, N, B)
    x0 = x0_near_ss(mpc, B, 61)
    r, rt = mpc.solve(x0, sens_v=True, sens_pi=sens_pi, cold=True), twin.solve(x0, sens_v=True, sens_pi=sens_pi, cold=True)
    assert r.status.tolist() == [0] * B
    gX, gU = normal_cotangent(mpc, 62)
    vx, vp = normal_directions(mpc, 2, 63)
    outs = [r.u0, r.V, r.status, r.iters, r.dV_dp] + ([r.dpi_dp] if sens_pi else [])
    before = [t.clone() for t in (*outs, *mpc.get_iterate(), mpc.get_lagrangian())]
    J0, v0 = policy(mpc, r.status), mpc.chain_trajectory_vjp(gX, gU)
    dX, dU = raw(mpc, r.status, 2, vx, vp)
    assert torch.isfinite(dX).all() and torch.isfinite(dU).all() and float(dU.abs().max()) > 0
    J1, v1 = policy(mpc, r.status), mpc.chain_trajectory_vjp(gX, gU)
    after = [*outs, *mpc.get_iterate(), mpc.get_lagrangian()]
    torch.cuda.synchronize()
    assert torch.equal(bits(J0), bits(J1)) and all(torch.equal(bits(p), bits(q)) for p, q in zip(v0, v1))
    assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(before, after))
    x1 = x0 + np.random.default_rng(64).normal(0.0, 0.005, x0.shape)
    a, b = mpc.solve(x1, sens_pi=True), twin.solve(x1, sens_pi=True)      # warm
    torch.cuda.synchronize()
    assert a.status.tolist() == b.status.tolist() == [0] * B and torch.equal(a.iters, b.iters)
    assert torch.equal(bits(a.u0), bits(b.u0)) and torch.equal(bits(a.V), bits(b.V)) and torch.equal(bits(a.dpi_dp), bits(b.dpi_dp))


# ---------------------------------------------------------------------- 6. contract
def test_rows_are_written_in_full():
    mpc = chain(3, 10, 4)
    x0 = x0_near_ss(mpc, 4, 71)
    x0[2, 4] = float("nan")
    vx, vp = normal_directions(mpc, 3, 72)
    for sens_pi in (True, False):      # both routes
        r = mpc.solve(x0, sens_pi=sens_pi, cold=True)
        st = r.status.tolist()
        assert st[2] not in (0, 2) and [st[i] for i in (0, 1, 3)] == [0, 0, 0]
        for fill in (float("nan"), 7.0):
            dX, dU = raw(mpc, r.status, 3, vx, vp, fill=fill)
            for t in (dX, dU):      # poisoned: every row was written
                assert torch.isfinite(t).all() and not (t == 7.0).any() and torch.all(t[2] == 0)
                assert all(float(t[i, d].abs().max()) > 0 for i in (0, 1, 3) for d in range(3))
            assert torch.equal(dX[[0, 1, 3], :, 0], vx[[0, 1, 3]])
        p_X, p_U = mpc.chain_trajectory_jvp(vx, vp)      # the Python surface: the same numbers
        assert torch.equal(bits(p_X), bits(dX)) and torch.equal(bits(p_U), bits(dU))
        assert mpc.chain_trajectory_jvp(vx, vp, U=False)[1] is None and mpc.chain_trajectory_jvp(vx, vp, X=False)[0] is None
        # [B, .] in, [B, ...] out; a 1-D dtheta is the same direction for every instance
        s_X, s_U = mpc.chain_trajectory_jvp(vx[:, 0], vp[:, 0])
        assert s_X.shape == (4, 11, mpc.nx) and torch.equal(bits(s_X), bits(dX[:, 0])) and torch.equal(bits(s_U), bits(dU[:, 0]))
        b_X, _ = mpc.chain_trajectory_jvp(None, vp[0, 1])
        assert torch.equal(bits(b_X[0]), bits(raw(mpc, r.status, 1, None, vp[0:1, 1:2].expand(4, 1, mpc.n_p).contiguous())[0][0, 0]))


def test_a_solve_cut_off_at_max_iter_follows_its_status():
    """max_iter = 1 from the problem's default start: no instance converges.  The rows follow the status word the solve wrote — the
    values at the stored iterate for 2 (max_iter), zeros for anything else — and a status word the caller overwrites with 4 gives
    zeros whatever the workspace holds."""
    mpc = chain(3, 10, 2)
    mpc.set_options(tol=1e-9, max_iter=1)
    r = mpc.solve(np.tile(mpc.ocp.x0, (2, 1)), cold=True)
    vx, vp = normal_directions(mpc, 2, 74)
    dX, dU = raw(mpc, r.status, 2, vx, vp)
    for i, st in enumerate(r.status.tolist()):
        assert st != 0, "max_iter = 1 must not converge from the default start"
        if st == 2:
            # (far from a KKT point the exact-Hessian matrix need not be positive definite: then every entry is NaN)
            assert ((torch.isfinite(dX[i]).all() and torch.isfinite(dU[i]).all() and torch.equal(dX[i, :, 0], vx[i]))
                    or (torch.isnan(dX[i]).all() and torch.isnan(dU[i]).all()))
        else:
            assert torch.all(dX[i] == 0) and torch.all(dU[i] == 0)
    forced = r.status.clone()
    forced[1] = 4
    fX, fU = raw(mpc, forced, 2, vx, vp, fill=7.0)
    assert torch.all(fX[1] == 0) and torch.all(fU[1] == 0)
    assert torch.equal(bits(fX[0]), bits(dX[0])) and torch.equal(bits(fU[0]), bits(dU[0]))


def test_refusals():
    from mpc4rl_amd import MPCBatch, _lib, cartpole_ocp
    mpc = chain(3, 10, 2)
    x0 = x0_near_ss(mpc, 2, 75)
    vx, vp = normal_directions(mpc, 2, 76)
    st = torch.zeros((2,), dtype=torch.int32, device=mpc.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, st, 2, vx, vp)                                     # before any solve
    with pytest.raises(RuntimeError):
        mpc.chain_trajectory_jvp(vx, vp)
    # each setter that clears the library's flag (raw() goes past the Python mirror of it)
    idx = torch.arange(2, dtype=torch.int64, device=mpc.device)
    setters = (lambda it: mpc.set_iterate(*it[:4]), lambda it: mpc.set_theta(torch.as_tensor(mpc.ocp.p0)),
               lambda it: mpc.set_bounds(_lib.BOUNDS_U0, -0.9 * np.ones(3), 0.9 * np.ones(3)), lambda it: mpc.set_discount_factor(0.99),
               lambda it: mpc.set_iterate_rows(*it[:4], idx), lambda it: mpc.reset(x0))
    for touch in setters:
        r = mpc.solve(x0, cold=True)
        assert all(torch.isfinite(t).all() for t in raw(mpc, r.status, 2, vx, vp))
        touch(mpc.get_iterate())
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, 2, vx, vp)
        with pytest.raises(RuntimeError):
            mpc.chain_trajectory_jvp(vx, vp)
    mpc.set_iterate(*mpc.get_iterate()[:4])
    with pytest.raises(RuntimeError, match="workspace of the last solve"):
        mpc.chain_trajectory_jvp(vx, vp)
    r = mpc.solve(x0, cold=True)
    # status, both directions, both outputs NULL; ndir < 1
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, None, 2, vx, vp)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status, 2, None, None)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw(mpc, r.status, 2, vx, vp, X=False, U=False)
    for ndir in (0, -1):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, ndir, vx, vp)
    for flags in (_lib.STATE_Q_MODE, 2):
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw(mpc, r.status, 2, vx, vp, flags=flags)
    with pytest.raises(ValueError):
        mpc.chain_trajectory_jvp(None, None)
    with pytest.raises(ValueError):
        mpc.chain_trajectory_jvp(vx, vp, X=False, U=False)
    with pytest.raises(ValueError):
        mpc.chain_trajectory_jvp(vx, vp[:, 0])                      # [B, R, nx] with [B, n_p]
    assert all(torch.isfinite(t).all() for t in raw(mpc, r.status, 2, vx, vp))      # and the handle still answers
    # the small models' surface stays closed to the chain
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        mpc._call("mpcrl_traj_jvp", 0, 2, vx, vp, torch.zeros((2, 2, 11, mpc.nx), dtype=torch.float64, device=mpc.device), None)
    for closed in (lambda: mpc.trajectory_jvp(vx, vp), mpc.trajectory_jacobian, mpc.n_diff):
        with pytest.raises(RuntimeError, match="chain of masses"):
            closed()
    # after a solve with u0 fixed: flags = 0 answers (u_0 free at the pinned value), the Python method refuses
    r = mpc.solve(x0, np.full((2, 3), 0.1), cold=True)
    assert r.status.tolist() == [0, 0] and all(not (t == 7.0).any() for t in raw(mpc, r.status, 2, vx, vp, fill=7.0))
    with pytest.raises(RuntimeError, match="Q mode"):
        mpc.chain_trajectory_jvp(vx, vp)
    cp = MPCBatch(cartpole_ocp(), 2)
    rc = cp.solve(np.zeros((2, 4)), cold=True)
    kw = dict(dtype=torch.float64, device=cp.device)
    with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
        cp._call("mpcrl_chain_traj_jvp", 0, rc.status, 1, torch.zeros((2, 1, 4), **kw), None, torch.zeros((2, 1, cp.N + 1, 4), **kw), None)
    with pytest.raises(RuntimeError, match="chain of masses"):
        cp.chain_trajectory_jvp(torch.zeros((2, 4), **kw), None)
    with pytest.raises(RuntimeError, match="chain of masses"):
        cp.chain_trajectory_jacobian()


# ---------------------------------------------------------------------- 7. graph capture
@pytest.mark.parametrize("sens_pi", [True, False])
def test_replays_inside_a_graph(sens_pi):
    mpc = chain(3, 10, 4)
    r = mpc.solve(x0_near_ss(mpc, 4, 81), sens_pi=sens_pi, cold=True)
    vx, vp = normal_directions(mpc, 3, 82)
    want = raw(mpc, r.status, 3, vx, vp)
    out = [torch.zeros_like(t) for t in want]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream, one node chain: no parallel branches
        mpc._call("mpcrl_chain_traj_jvp", 0, r.status, 3, vx, vp, out[0], out[1])
    torch.cuda.synchronize()
    assert all(torch.all(t == 0) for t in out)          # captured, not run
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(t), bits(w)) for t, w in zip(out, want))


# ---------------------------------------------------------------------- 8. the Jacobian
def test_jacobian_columns_are_single_direction_calls():
    from mpc4rl_amd.problems import chain_param_layout
    n_mass, N, B = 3, 10, 2
    mpc = chain(n_mass, N, B)
    r = mpc.solve(x0_near_ss(mpc, B, 91), sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * B
    J = mpc.chain_trajectory_jacobian()
    nx, nl, off = mpc.nx, n_mass - 1, chain_param_layout(n_mass)[4]
    assert J.entries.tolist() == list(range(10 * nl))      # the default: m, D, L, C
    assert J.dX_dx0.shape == (B, N + 1, nx, nx) and J.dU_dx0.shape == (B, N, 3, nx)
    assert J.dX_dtheta.shape == (B, N + 1, nx, 10 * nl) and J.dU_dtheta.shape == (B, N, 3, 10 * nl)
    assert torch.equal(J.dX_dx0[:, 0], torch.eye(nx, dtype=torch.float64, device=mpc.device).expand(B, nx, nx))
    assert torch.all(J.dX_dtheta[:, 0] == 0)
    for j in (0, nx - 1):      # a column in x0
        e = torch.zeros((B, nx), dtype=torch.float64, device=mpc.device)
        e[:, j] = 1.0
        dX, dU = mpc.chain_trajectory_jvp(e, None)
        assert torch.equal(bits(dX), bits(J.dX_dx0[..., j].contiguous())) and torch.equal(bits(dU), bits(J.dU_dx0[..., j].contiguous()))
    for j in (0, nl + 1, 10 * nl - 1):      # a column in theta
        e = torch.zeros((mpc.n_p,), dtype=torch.float64, device=mpc.device)
        e[j] = 1.0
        dX, dU = mpc.chain_trajectory_jvp(None, e)
        assert float(dU.abs().max()) > 0
        assert torch.equal(bits(dX), bits(J.dX_dtheta[..., j].contiguous())) and torch.equal(bits(dU), bits(J.dU_dtheta[..., j].contiguous()))
    # by name and by index
    by_name, by_index = mpc.chain_trajectory_jacobian(("C", "w")), mpc.chain_trajectory_jacobian(list(range(*off["C"])) + list(range(*off["w"])))
    assert by_name.entries.tolist() == by_index.entries.tolist() == list(range(*off["C"])) + list(range(*off["w"]))
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(by_name[:4], by_index[:4]))
    assert torch.equal(bits(by_name.dX_dtheta[..., :3 * nl]), bits(J.dX_dtheta[..., 7 * nl:]))      # the C block, again


MEASURED = """\
chain traj jvp n_mass 3 N 1 ss B 4: du0*/dp 1.6e-07 -> bar 1.0e-06, dW 1.6e-07 / 1.5e-07 / 1.7e-07; against the neighbour's rows 2.6e+00
chain traj jvp n_mass 3 N 1 ss B 1: du0*/dp 1.6e-07 -> bar 1.0e-06, dW 1.5e-07 / 1.5e-07 / 1.7e-07; against the neighbour's rows 1.3e+00
chain traj jvp n_mass 3 N 2 ss B 4: du0*/dp 3.2e-08 -> bar 1.0e-06, dW 3.2e-08 / 3.2e-08 / 5.9e-08; against the neighbour's rows 2.4e+00
chain traj jvp n_mass 3 N 2 ss B 1: du0*/dp 3.1e-08 -> bar 1.0e-06, dW 3.0e-08 / 2.9e-08 / 3.5e-08; against the neighbour's rows 4.8e-01
chain traj jvp n_mass 3 N 10 ss B 4: du0*/dp 3.9e-08 -> bar 1.0e-06, dW 4.8e-08 / 3.8e-08 / 3.3e-08; against the neighbour's rows 1.7e+00
chain traj jvp n_mass 3 N 10 ss B 1: du0*/dp 3.5e-08 -> bar 1.0e-06, dW 3.5e-08 / 3.5e-08 / 3.3e-08; against the neighbour's rows 9.0e-01
chain traj jvp n_mass 3 N 10 x0 B 4: du0*/dp 3.1e-08 -> bar 1.0e-06, dW 2.1e-08 / 4.4e-08 / 3.4e-08; against the neighbour's rows 1.5e+00
chain traj jvp n_mass 3 N 10 x0 B 1: du0*/dp 3.1e-08 -> bar 1.0e-06, dW 2.1e-08 / 4.4e-08 / 3.4e-08; against the neighbour's rows 1.3e+00
chain traj jvp n_mass 4 N 3 ss B 4: du0*/dp 1.3e-07 -> bar 1.0e-06, dW 2.7e-07 / 2.3e-07 / 1.7e-07; against the neighbour's rows 1.9e+00
chain traj jvp n_mass 4 N 3 ss B 1: du0*/dp 6.9e-08 -> bar 1.0e-06, dW 1.0e-07 / 9.1e-08 / 1.7e-07; against the neighbour's rows 7.3e-01
chain traj jvp n_mass 5 N 8 ss B 4: du0*/dp 4.3e-08 -> bar 1.0e-06, dW 2.7e-07 / 2.4e-07 / 3.5e-07; against the neighbour's rows 2.0e+00
chain traj jvp n_mass 5 N 8 ss B 1: du0*/dp 3.8e-08 -> bar 1.0e-06, dW 2.4e-07 / 2.4e-07 / 3.5e-07; against the neighbour's rows 1.8e+00
chain traj jvp n_mass 6 N 3 ss B 4: du0*/dp 4.4e-08 -> bar 1.0e-06, dW 2.7e-07 / 1.6e-07 / 3.2e-07; against the neighbour's rows 1.9e+00
chain traj jvp n_mass 6 N 3 ss B 1: du0*/dp 4.4e-08 -> bar 1.0e-06, dW 2.7e-07 / 4.4e-08 / 2.3e-07; against the neighbour's rows 5.7e-01
chain traj jvp n_mass 7 N 5 ss B 4: du0*/dp 9.1e-08 -> bar 1.0e-06, dW 3.5e-07 / 3.6e-07 / 2.7e-07; against the neighbour's rows 1.6e+00
chain traj jvp n_mass 7 N 5 ss B 1: du0*/dp 8.4e-08 -> bar 1.0e-06, dW 1.8e-07 / 3.6e-07 / 2.0e-07; against the neighbour's rows 8.2e-01
chain traj jvp n_mass 3 N 10 act B 4: du0*/dp 2.8e-08 -> bar 1.0e-06, dW 2.3e-08 / 9.8e-09 / 8.3e-08; against the neighbour's rows 2.0e+00
chain traj jvp n_mass 3 N 10 act B 1: du0*/dp 9.6e-09 -> bar 1.0e-06, dW 1.5e-08 / 9.0e-09 / 2.2e-08; against the neighbour's rows 1.1e+00
chain traj jvp adjoint identity n_mass 3 N 10: 1.9e-15
chain traj jvp adjoint identity n_mass 5 N 8: 2.5e-15
chain traj jvp adjoint identity n_mass 7 N 5: 5.4e-16
chain traj jvp adjoint identity n_mass 3 N 10 theta per instance: 1.3e-15
chain traj jvp u_0 rows n_mass 3 N 10: against du0*/dx0 1.3e-15, against dpi_dp 3.9e-16
chain traj jvp u_0 rows n_mass 6 N 3: against du0*/dx0 5.5e-16, against dpi_dp 6.1e-16
"""
