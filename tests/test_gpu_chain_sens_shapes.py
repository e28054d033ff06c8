"""The four derivative calls of the chain's plan — mpcrl_chain_traj_jvp, mpcrl_chain_traj_vjp, mpcrl_chain_bound_vjp and
mpcrl_chain_policy_state_sens — past one workgroup and past horizon 10.  chain_jvp_rhs_kernel and chain_sens_mix2_kernel<M, 1> are
flattened over the batch, a lane per (instance, stage): gid = 64 blockIdx + threadIdx, inst = gid / N, k = gid - inst N, grid
(B N + 63) / 64.  The tests of the four calls elsewhere stop at B N = 40: one workgroup, never full.  The sets of the fixture G17
(tests/golden/make_chain_sens_shapes.py) reach a second and a third workgroup, a grid that is an exact multiple of 64, tails of 2 lanes,
instances whose stages straddle two workgroups, inst up to 12, and the horizons 16, 33, 40 (the default and the benchmark's) and 63 (the
longest mpcrl_create accepts), where the per-instance kernels (chain_traj_riccati_kernel, chain_traj_jvp_riccati_kernel,
chain_traj_out_kernel, chain_bound_out_kernel, chain_state_sens_kernel) size their LDS and their loops from N:

    set          B   B N   workgroups of (instance, stage) lanes
    m3_N10_mix  13   130   3, a tail of 2; instances 6 and 12 straddle a boundary (both have control rows on their bounds)
    m3_N16_ss    8   128   exactly 2, no tail
    m3_N40_mix   3   120   2; instance 1 straddles
    m3_N63_ss    2   126   2; instance 1 straddles
    m5_N40_ss    2    80   2; instance 1 straddles
    m7_N33_ss    2    66   2, a tail of 2; instance 1 straddles

The adjoint identity cannot see the index arithmetic (the JVP's right-hand side is the transpose of mix2<M, 1> on the same arithmetic: a
shared mistake cancels), so the statements here are against references that do not share it: (a) the mirror's dense Jacobians, with
the neighbouring instance's rows as negative control, per instance; (b) a lone handle (B = 1: inst = 0, one workgroup) bit for bit, and
the batch in reversed order, where every instance sits at another workgroup offset; (c) the solve's own du0*/dp, which comes from the
NU-wide mix2 launch on another grid, and du0*/dx0; (d) the identity, for the coefficients; (e) the calls' contract with a failed
instance on a workgroup boundary.

Bars (none of them new).  Against the fixture: max(1e-6, 4 x the error of the same solve's du0*/dp against the mirror's), the rule
of tests/test_gpu_chain_traj_jvp.py, test_gpu_chain_traj_vjp.py, test_gpu_chain_bound_vjp.py and test_gpu_chain_state_sens.py, with
their scalings: the JVP per direction over all of dW, the others per instance, rows scaled by max(|reference row|, 1); dV/dx0: 1e-6.
The fixture stores its two standard-normal cotangents; the third of the other files, the unit cotangent on component 0 of u_0, is held
against row 0 of the fixture's du0*/dp and du0*/dx0, without bound rows and without the negative control.
(c) and (d): 1e-6 (RTOL of tests/small_mode_cases.py).  Everything else is torch.equal on the bits.  On the ss sets the bound
gradients have no negative control: nothing is active there, the reference rows are below the bar themselves
(tests/test_chain_sens_shapes_cpu.py).

Measured on an MI355X: MEASURED at the end of this file (every line the tests print).
"""
import os

import numpy as np
import pytest
import torch

import small_mode_cases as C
import test_gpu_chain_bound_vjp as bnd
import test_gpu_chain_state_sens as sens
import test_gpu_chain_traj_jvp as jvp
import test_gpu_chain_traj_vjp as vjp
from test_gpu_chain_traj_jvp import bits, chain, dev, normal_cotangent, normal_directions, policy, scaled, w_of
from test_gpu_chain_traj_vjp import split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = C.RTOL
SETS = ((3, 10, "mix"), (3, 16, "ss"), (3, 40, "mix"), (3, 63, "ss"), (5, 40, "ss"), (7, 33, "ss"))
NAMES = ("jvp dX", "jvp dU") + tuple(f"{call} {out} [{c}]" for c in range(3) for call, outs in
                                    (("traj vjp", ("g_x0", "g_theta")), ("bound vjp", ("g_x0", "g_theta", "g_lb", "g_ub"))) for out in outs) + ("du0*/dx0",)


@pytest.fixture(scope="module")
def g17():
    return np.load(os.path.join(ROOT, "tests", "golden", "g17_chain_sens_shapes.npz"))


def rows(got, ref):
    """``scaled`` before its last max: one figure per row of ref."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    got, ref = got.reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1)
    return np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)


def own_theta(n_mass, N, B):
    """m and D x U(0.95, 1.05) per instance, as test_adjoint_identity_with_the_trajectory_vjp draws it."""
    from mpc4rl_amd import chain_mass_ocp
    th = np.tile(chain_mass_ocp(n_mass=n_mass, N=N).p0, (B, 1))
    nl = n_mass - 1
    th[:, :4 * nl] *= np.random.default_rng(31).uniform(0.95, 1.05, (B, 4 * nl))
    return th


def solve(n_mass, N, x0, theta=None):
    mpc = chain(n_mass, N, len(x0))
    if theta is not None:
        mpc.set_theta(torch.as_tensor(theta))
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    torch.cuda.synchronize()
    return mpc, r


def take(mpc, fx, key, idx):
    """The fixture's directions and cotangents of the instances ``idx`` on the device of a handle of len(idx) instances.  Cotangents
    0 and 1 are the fixture's; 2 is the unit cotangent on component 0 of u_0, which the fixture's gate saw and the file leaves out
    (its references are row 0 of dpi_dp and of dpi_dx0)."""
    unit = np.zeros((len(idx), fx[key + "G"].shape[2]))
    unit[:, 0] = 1.0
    cot = [split(mpc, fx[key + "G"][idx, c]) for c in range(2)] + [split(mpc, unit)]
    return dict(vx=dev(mpc, fx[key + "vx"][idx]), vp=dev(mpc, fx[key + "vp"][idx]), gX=[c[0] for c in cot], gU=[c[1] for c in cot])


def four_calls(mpc, status, inp, fill=float("nan")):
    """Every output of the four calls, each the library call itself on buffers poisoned with ``fill`` (NAMES, each [B, ...])."""
    out = list(jvp.raw(mpc, status, 3, inp["vx"], inp["vp"], fill=fill))
    for c in range(3):
        out += list(vjp.raw(mpc, status, inp["gX"][c], inp["gU"][c], fill=fill))
        out += list(bnd.raw(mpc, status, inp["gX"][c], inp["gU"][c], fill=fill))
    out.append(sens.raw(mpc, status, fill=fill))
    return out


def solve_outputs(r):
    return [r.u0, r.V, r.dV_dp, r.dpi_dp]


class Batch:
    """A set of the fixture solved in one handle, and what the four calls return on it."""

    def __init__(self, fx, n_mass, N, base, per_instance_theta=False):
        self.key = f"m{n_mass}_N{N}_{base}_"
        self.x0 = fx[self.key + "x0"]
        self.B = len(self.x0)
        self.theta = own_theta(n_mass, N, self.B) if per_instance_theta else None
        self.mpc, self.r = solve(n_mass, N, self.x0, self.theta)
        self.status = self.r.status.tolist()
        self.inp = take(self.mpc, fx, self.key, np.arange(self.B))
        self.outs = four_calls(self.mpc, self.r.status, self.inp) if self.status == [0] * self.B else None


@pytest.fixture(scope="module")
def batch(g17):
    memo = {}

    def get(n_mass, N, base, per_instance_theta=False):
        k = (n_mass, N, base, per_instance_theta)
        if k not in memo:
            memo[k] = Batch(g17, n_mass, N, base, per_instance_theta)
        assert memo[k].status == [0] * memo[k].B, (k, memo[k].status)
        return memo[k]

    return get


# ---------------------------------------------------------------------- a. against the mirror
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_the_four_calls_against_the_mirror(g17, batch, n_mass, N, base):
    """The whole set in one handle: cold solve at tol 1e-9 with sens_v and sens_pi.  Every instance's rows within the bar of the
    fixture's, and — the negative control — every instance's rows further than the bar from the fixture rows of the next instance:
    an instance index that is off by one cannot pass."""
    b = batch(n_mass, N, base)
    mpc, r, key, B = b.mpc, b.r, b.key, b.B
    fx = {k: g17[key + k] for k in ("vx", "vp", "dX", "dU", "G", "g_theta", "g_x0", "g_lb", "g_ub", "dpi_dp", "dpi_dx0", "dV_dx0")}
    for k, full in (("g_theta", fx["dpi_dp"]), ("g_x0", fx["dpi_dx0"])):      # the unit cotangent on u_0[0]: row 0 of the policy Jacobians
        fx[k] = np.concatenate([fx[k], full[:, None, 0]], 1)
    nxt = {k: np.roll(v, -1, 0) for k, v in fx.items()}
    err_dp = scaled(r.dpi_dp, fx["dpi_dp"])
    bar = max(RTOL, 4.0 * err_dp)
    # the JVP, the fixture's three directions in one call
    dX, dU = mpc.chain_trajectory_jvp(fx["vx"], fx["vp"])
    assert dX.shape == (B, 3, N + 1, mpc.nx) and dU.shape == (B, 3, N, mpc.nu) and torch.equal(dX[:, :, 0], dev(mpc, fx["vx"]))
    got, ref, nb = w_of(dX, dU), w_of(fx["dX"], fx["dU"]), w_of(nxt["dX"], nxt["dU"])
    e_jvp = [rows(got[d::3], ref[d::3]).max() for d in range(3)]
    w_jvp = min(rows(got[d::3], nb[d::3]).min() for d in range(3))
    # the VJP and the bound VJP, the fixture's three cotangents
    e_th = e_x = e_b = w_b = 0.0
    w_th = w_x = np.inf
    for c in range(3):
        gX, gU = b.inp["gX"][c], b.inp["gU"][c]
        g_x0, g_th = mpc.chain_trajectory_vjp(gX, gU)
        assert g_x0.shape == (B, mpc.nx) and g_th.shape == (B, mpc.n_p)
        e_th, e_x = max(e_th, rows(g_th, fx["g_theta"][:, c]).max()), max(e_x, rows(g_x0, fx["g_x0"][:, c]).max())
        _, _, g_lb, g_ub = mpc.bound_vjp(gX, gU, x0=False, theta=False)
        assert g_lb.shape == g_ub.shape == (B, N + 1, 3 + mpc.nx)
        # the chain has no state bounds, stage N no controls: exact zeros
        assert torch.all(g_lb[:, :, 3:] == 0) and torch.all(g_ub[:, :, 3:] == 0) and torch.all(g_lb[:, N] == 0) and torch.all(g_ub[:, N] == 0)
        if c == 2:      # no negative control (a u_0[0] on its bound has zero rows in both instances) and no bound rows in the fixture
            continue
        w_th, w_x = min(w_th, rows(g_th, nxt["g_theta"][:, c]).min()), min(w_x, rows(g_x0, nxt["g_x0"][:, c]).min())
        both = torch.stack([g_lb[:, :N, :3], g_ub[:, :N, :3]], 1)
        e_b = max(e_b, scaled(both, np.stack([fx["g_lb"][:, c], fx["g_ub"][:, c]], 1)))
        w_b = max(w_b, scaled(both, np.stack([nxt["g_lb"][:, c], nxt["g_ub"][:, c]], 1)))
    # du0*/dx0 and dV/dx0
    s = mpc.state_sens()
    torch.cuda.synchronize()
    assert s.dQ_du0 is None and s.dpi_dx0.shape == (B, 3, mpc.nx) and torch.equal(bits(s.dpi_dx0), bits(policy(mpc, r.status)))
    e_pi, e_v = rows(s.dpi_dx0, fx["dpi_dx0"]).max(), rows(s.dV_dx0, fx["dV_dx0"]).max()
    w_pi, w_v = rows(s.dpi_dx0, nxt["dpi_dx0"]).min(), rows(s.dV_dx0, nxt["dV_dx0"]).min()
    print(f"chain sens shapes a {key[:-1]} B {B}: du0*/dp {err_dp:.1e} -> bar {bar:.1e}; dW {e_jvp[0]:.1e} / {e_jvp[1]:.1e} / {e_jvp[2]:.1e}, "
          f"g_theta {e_th:.1e}, g_x0 {e_x:.1e}, g_lb g_ub {e_b:.1e}, du0*/dx0 {e_pi:.1e}, dV/dx0 {e_v:.1e}; the least against the "
          f"neighbour's rows: dW {w_jvp:.1e}, g_theta {w_th:.1e}, g_x0 {w_x:.1e}, du0*/dx0 {w_pi:.1e}, dV/dx0 {w_v:.1e}; g_lb g_ub {w_b:.1e}")
    assert max(e_jvp) <= bar and e_th <= bar and e_x <= bar and e_b <= bar and e_pi <= bar and e_v <= RTOL, (key, bar)
    assert min(w_jvp, w_th, w_x, w_pi, w_v) > bar and (base != "mix" or w_b > bar), (key, bar)


# ---------------------------------------------------------------------- b. same bits as a lone handle, and in reversed order
@pytest.mark.parametrize("n_mass,N,base,per_instance_theta", [s + (False,) for s in SETS] + [(3, 10, "mix", True), (3, 40, "mix", True)])
def test_same_bits_as_a_lone_handle_and_in_reversed_order(g17, batch, n_mass, N, base, per_instance_theta):
    """Every instance of the batch against a handle of its own (B = 1) on its x0 (and its row of theta): the solve's outputs and every
    output of the four calls, the same bits.  Then the batch in reversed order on a fresh handle: flipped back, the same bits — every
    instance has sat at two different workgroup offsets."""
    b = batch(n_mass, N, base, per_instance_theta)
    key, B = b.key, b.B
    assert all(torch.isfinite(t).all() for t in b.outs)
    for i in range(B):
        one, r1 = solve(n_mass, N, b.x0[i:i + 1], None if b.theta is None else b.theta[i:i + 1])
        assert r1.status.tolist() == [0], (key, i)
        for name, p, q in zip(("u0", "V", "dV_dp", "dpi_dp"), solve_outputs(b.r), solve_outputs(r1)):
            assert torch.equal(bits(p[i:i + 1]), bits(q)), (key, i, name)
        for name, p, q in zip(NAMES, b.outs, four_calls(one, r1.status, take(one, g17, key, np.array([i])))):
            assert torch.equal(bits(p[i:i + 1]), bits(q)), (key, i, name)
    back = np.arange(B)[::-1].copy()
    rev, rr = solve(n_mass, N, b.x0[back], None if b.theta is None else b.theta[back])
    assert rr.status.tolist() == [0] * B
    flip = lambda t: torch.flip(t, (0,))
    for name, p, q in zip(("u0", "V", "dV_dp", "dpi_dp"), solve_outputs(b.r), solve_outputs(rr)):
        assert torch.equal(bits(p), bits(flip(q))), (key, "reversed", name)
    for name, p, q in zip(NAMES, b.outs, four_calls(rev, rr.status, take(rev, g17, key, back))):
        assert torch.equal(bits(p), bits(flip(q))), (key, "reversed", name)
    print(f"chain sens shapes b {key[:-1]} B {B}{' theta per instance' if per_instance_theta else ''}: {B} lone handles and the reversed "
          f"batch, {len(NAMES) + 4} outputs each: the same bits")


# ---------------------------------------------------------------------- c. against the solve's own du0*/dp and du0*/dx0
@pytest.mark.parametrize("n_mass,N,base", [(3, 10, "mix"), (3, 40, "mix"), (7, 33, "ss")])
def test_u0_rows_and_unit_cotangents_are_the_policy_sensitivities(batch, n_mass, N, base):
    """Forward: unit directions on x0 and on the twelve entries of p of test_rows_of_u0_are_the_policy_sensitivities give the u_0 rows
    du0*/dx0 and the columns of du0*/dp.  Reverse: unit cotangents on the entries of u_0 give their rows.  du0*/dp comes from the
    NU-wide mix2 launch (another grid, held to the port at the benchmark's size): every stage lane's contribution to g_theta, and
    every stage lane's right-hand side of the JVP, is in these numbers."""
    b = batch(n_mass, N, base)
    mpc, r, B = b.mpc, b.r, b.B
    J = policy(mpc, r.status)
    nx, nl = mpc.nx, n_mass - 1
    off_q = 10 * nl
    off_r = off_q + nx * nx
    cols = [0, nl - 1, nl, 4 * nl + 1, 7 * nl + 2, off_q, off_q + 1, off_q + nx * nx - 1, off_r, off_r + 4, off_r + 9, mpc.n_p - 1]
    eye = torch.eye(nx, dtype=torch.float64, device=mpc.device).expand(B, nx, nx).contiguous()
    _, dU = mpc.chain_trajectory_jvp(eye, None)
    f_x = scaled(dU[:, :, 0].transpose(1, 2), J)
    dth = torch.zeros((B, len(cols), mpc.n_p), dtype=torch.float64, device=mpc.device)
    dth[:, torch.arange(len(cols)), torch.as_tensor(cols)] = 1.0
    _, dU = mpc.chain_trajectory_jvp(None, dth)
    f_p = scaled(dU[:, :, 0].transpose(1, 2), r.dpi_dp[:, :, cols])
    assert float(dU.abs().amax((0, 2, 3)).min()) > 0      # every block moves the plan
    r_th = r_x = 0.0
    for c in range(3):
        gU = torch.zeros((B, N, 3), dtype=torch.float64, device=mpc.device)
        gU[:, 0, c] = 1.0
        g_x0, g_th = vjp.raw(mpc, r.status, None, gU)
        r_th, r_x = max(r_th, scaled(g_th, r.dpi_dp[:, c])), max(r_x, scaled(g_x0, J[:, c]))
    print(f"chain sens shapes c {b.key[:-1]} B {B}: u_0 rows of the JVP against du0*/dx0 {f_x:.1e}, against dpi_dp {f_p:.1e}; unit "
          f"cotangents: g_theta against dpi_dp {r_th:.1e}, g_x0 against du0*/dx0 {r_x:.1e}")
    assert max(f_x, f_p, r_th, r_x) <= RTOL, (f_x, f_p, r_th, r_x)


# ---------------------------------------------------------------------- d. the adjoint identity
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_adjoint_identity(batch, n_mass, N, base):
    """<G, JVP(v)> = g_x0 . vx + g_theta . vp, cotangents and directions standard normal over all of w, x0 and p, with the scaling of
    test_adjoint_identity_with_the_trajectory_vjp: the coefficients of both kernels at these horizons (not their index arithmetic)."""
    b = batch(n_mass, N, base)
    mpc = b.mpc
    gX, gU = normal_cotangent(mpc, 33)
    vx, vp = normal_directions(mpc, 2, 34)
    g_x0, g_th = mpc.chain_trajectory_vjp(gX, gU)
    dX, dU = mpc.chain_trajectory_jvp(vx, vp)
    lhs = (gX[:, None] * dX).sum((2, 3)) + (gU[:, None] * dU).sum((2, 3))
    rhs = (g_x0[:, None] * vx).sum(2) + (g_th[:, None] * vp).sum(2)
    scale = ((gX[:, None] * dX).abs().sum((2, 3)) + (gU[:, None] * dU).abs().sum((2, 3))).clamp(min=1.0)
    worst = float(((lhs - rhs).abs() / scale).max())
    print(f"chain sens shapes d {b.key[:-1]} B {b.B}: adjoint identity {worst:.1e}")
    assert torch.isfinite(lhs).all() and float(lhs.abs().min()) > 0 and worst <= 1e-6, worst


# ---------------------------------------------------------------------- e. contract at more than one workgroup
def test_a_failed_instance_on_a_workgroup_boundary(g17, batch):
    """m3_N10_mix with a NaN in x0 of instance 6, whose stage lanes 60 .. 69 lie in workgroups 0 and 1: its status is neither 0 nor 2
    and its rows are zeros for all four calls, whatever the buffers held; every other instance keeps the bits it has without the
    NaN.  Then ndir = 17: the directions flipped give the flipped bits."""
    n_mass, N, base = 3, 10, "mix"
    clean = batch(n_mass, N, base)
    x0 = clean.x0.copy()
    x0[6, 4] = float("nan")
    mpc, r = solve(n_mass, N, x0)
    st = r.status.tolist()
    others = [i for i in range(clean.B) if i != 6]
    assert st[6] not in (0, 2) and [st[i] for i in others] == [0] * len(others), st
    for fill in (float("nan"), 7.0):
        for name, t, ref in zip(NAMES, four_calls(mpc, r.status, clean.inp, fill=fill), clean.outs):
            assert torch.isfinite(t).all() and not (t == 7.0).any() and torch.all(t[6] == 0), (name, fill)
            assert torch.equal(bits(t[others]), bits(ref[others])), (name, fill)
    vx, vp = normal_directions(mpc, 17, 52)
    X17, U17 = jvp.raw(mpc, r.status, 17, vx, vp)
    flip = lambda t: torch.flip(t, (1,)).contiguous()
    Xf, Uf = jvp.raw(mpc, r.status, 17, flip(vx), flip(vp))
    assert torch.isfinite(X17).all() and torch.isfinite(U17).all() and torch.all(X17[6] == 0) and torch.all(U17[6] == 0)
    assert all(float(U17[i, d].abs().max()) > 0 for i in others for d in range(17))
    assert torch.equal(bits(flip(Xf)), bits(X17)) and torch.equal(bits(flip(Uf)), bits(U17))
    print(f"chain sens shapes e m3_N10_mix B {clean.B}: status {st}; instance 6 zeros, the others' bits kept, ndir 17 flipped: the same bits")


MEASURED = """\
"""
