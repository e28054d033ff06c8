"""mpcrl_cost_vjp and mpcrl_cost_value_grad (include/mpcrl_cost_ext.h) on the device: the derivatives of the cartpole's planned
trajectory and of its value with respect to the tracking cost (W_0, W, W_e, yref_0, yref, yref_e: entries 3 .. 82 of p, each an
independent variable) from small_cost_vjp_kernel / cost_value_grad_kernel against the mirror fixture G14
(tests/golden/make_cost_vjp.py), the closed forms of the value gradient restated in float64 on ``get_iterate()``, the calls' contract,
the same bits as mpcrl_bound_vjp on the four outputs they share, every lane layout, and MPCLayer(cost_gradient=True) on top.

Bars.  Against the fixture: max(1e-6, 4 x the error of that solve's own du0*/dp against the fixture's mirror du0*/dp on the same
instances) — the bar of tests/test_gpu_bound_vjp.py, in its measure: a row is an instance's whole [83] gradient, scaled by
max(|reference|, 1).  The instances with an active hard state row are asserted on their own and printed on their own line.  The value
formulas against their float64 restatement: 1e-12 (sums of at most 62 products, in another order).  The layer against central
differences of its own forward pass at h = 1e-5: 1e-5, the bar of the existing layer tests.  Q mode against differences of Q at
h = 1e-4 (solves at tol 1e-10): 1e-6, the existing Q-mode bar.

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
SETS = [("A", N) for N in (2, 15, 20, 31, 32, 63)] + [("B", N) for N in (2, 15, 20, 32)]
RTOL = C.RTOL
NP, NDYN = 83, 3
W_BLOCKS = ((3, 5), (28, 5), (53, 4))      # (offset, side) of W_0, W, W_e in p, each column-major


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(GOLD, "g14_cost_vjp.npz"))


def scaled(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    if not len(ref):
        return 0.0
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)).max())


def same(a, b):
    """bit-identical, NaN included"""
    return all((x is None and y is None) or torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def handle(ocp, B, bounds=None, tol=1e-9, theta=None):
    from mpc4rl_amd import MPCBatch, _lib
    mpc = MPCBatch(ocp, B)
    mpc.set_options(tol=tol)
    if bounds is not None:
        mpc.set_bounds(_lib.BOUNDS_U0, bounds[0], bounds[1])
        mpc.set_bounds(_lib.BOUNDS_STAGE, bounds[2], bounds[3])
        mpc.set_bounds(_lib.BOUNDS_TERMINAL, bounds[4], bounds[5])
    if theta is not None:
        mpc.set_theta(theta)
    return mpc


def fixture_bounds(g14, key):
    return tuple(g14[key + k] for k in ("lb0", "ub0", "lb", "ub", "lbe", "ube"))


def split(mpc, G):
    """(gX [B, N+1, nx], gU [B, N, nu]) of cotangents [B, nw] in the mirror's order w = [u_0 .. u_{N-1}; x_0 .. x_N]."""
    G = torch.as_tensor(G, dtype=torch.float64, device=mpc.device)
    n = mpc.N * mpc.nu
    return G[:, n:].reshape(mpc.B, mpc.N + 1, mpc.nx).contiguous(), G[:, :n].reshape(mpc.B, mpc.N, mpc.nu).contiguous()


def shapes(mpc):
    nb = (mpc.B, mpc.N + 1, mpc.nu + mpc.nx)
    return (mpc.B, mpc.nx), (mpc.B, mpc.n_p), nb, nb, (mpc.B, mpc.n_p)


def raw_vjp(mpc, gX, gU, want=(True,) * 5, flags=0, name="mpcrl_cost_vjp"):
    """The library call itself on NaN-poisoned buffers (``mpcrl_bound_vjp``: the first four)."""
    kw = dict(dtype=torch.float64, device=mpc.device)
    bufs = [torch.full(sh, float("nan"), **kw) if w else None for sh, w in zip(shapes(mpc), want)]
    mpc._call(name, flags, gX, gU, *(bufs if name == "mpcrl_cost_vjp" else bufs[:4]))
    torch.cuda.synchronize()
    return bufs


def raw_value(mpc, flags=0, want=True):
    buf = torch.full((mpc.B, mpc.n_p), float("nan"), dtype=torch.float64, device=mpc.device) if want else None
    mpc._call("mpcrl_cost_value_grad", flags, buf)
    torch.cuda.synchronize()
    return buf


def symmetric_bits(g):
    """every W block of g [B, 83] holds the same bits at [a, b] and [b, a]"""
    return all(torch.equal(b.view(torch.int64), b.transpose(1, 2).contiguous().view(torch.int64))
               for b in (g[:, o:o + n * n].reshape(-1, n, n).contiguous() for o, n in W_BLOCKS))


def perturbed_theta(p0, B, seed):
    """Per-instance parameter vectors as the fixture's set B draws them: every weight W + L L' + (K - K'), not symmetric and not
    diagonal, every reference 0.1 N(0, 1).  (About a third of such draws do not solve at N >= 15; the seeds used below are ones at which
    the port's default mode, the product's twin, solves every instance of its test, perturbed solves of the differences included.)"""
    rng = np.random.default_rng(seed)
    p = np.tile(np.asarray(p0, float), (B, 1))
    for i in range(B):
        for o, n in W_BLOCKS:
            L, K = 0.1 * rng.standard_normal((n, 2)), 0.01 * rng.standard_normal((n, n))
            p[i, o:o + n * n] = (p[i, o:o + n * n].reshape(n, n).T + L @ L.T + (K - K.T)).flatten("F")
        p[i, 69:] = 0.1 * rng.standard_normal(14)
    return p


def fmt(e):
    return " ".join(f"{v:.1e}" for v in e)


# ---------------------------------------------------------------------- 1. against the fixture
def fixture_case(g14, key, ocp, rows):
    x0, p = g14[key + "x0"][rows], g14[key + "p"][rows]
    mpc = handle(ocp, len(x0), fixture_bounds(g14, key), theta=p)
    r = mpc.solve(x0, sens_pi=True, cold=True)
    assert r.status.tolist() == [0] * len(x0), (key, r.status.tolist())
    act_x = g14[key + "act_x"][rows]
    ref_dp = g14[key + "dpi_dp"][rows].copy()
    ref_dp[g14[key + "act_u0"][rows]] = 0.0      # u_0 on its bound: the exact zero, as tests/test_gpu_state_sens.py takes it
    assert torch.all(r.dpi_dp[:, :, NDYN:] == 0)      # du0*/dp keeps its zero cost block
    err_dp = scaled(r.dpi_dp.cpu().numpy()[:, :, :NDYN], ref_dp)
    e_all, e_x, got0 = [], [], None
    for c in range(3):
        gX, gU = split(mpc, g14[key + "G"][rows][:, c])
        g = mpc.cost_vjp(gX, gU, x0=False, theta=False)[4]
        assert torch.all(g[:, :NDYN] == 0) and symmetric_bits(g)
        ref = g14[key + "g_cost"][rows][:, c]
        e_all.append(scaled(g, ref)), e_x.append(scaled(g.cpu().numpy()[act_x], ref[act_x]))
        got0 = g.cpu().numpy() if c == 0 else got0
    dV = mpc.cost_value_grad()
    assert torch.all(dV[:, :NDYN] == 0) and symmetric_bits(dV)
    e_V = scaled(dV, g14[key + "dV_dcost"][rows])
    return max(RTOL, 4.0 * err_dp), err_dp, e_all, e_x, e_V, int(act_x.sum()), got0


@pytest.mark.parametrize("which,N", SETS)
def test_cost_vjp_against_the_mirror(g14, which, N):
    """Every instance of the set, then its first instance alone (B = 1); three cotangents each (two random over all of w, the unit
    vector on u_0).  Set A: the nominal p; set B: a per-instance p with weights that are not symmetric.  Negative control: an
    instance's g_cost for its own cotangent is farther than 100 x the bar from the next instance's reference."""
    ocp, _ = C.problem("cartpole", N)
    key = f"{which}_N{N}_"
    for rows in (slice(None), slice(0, 1)):
        bar, err_dp, e_all, e_x, e_V, nx, got = fixture_case(g14, key, ocp, rows)
        B = len(g14[key + "x0"][rows])
        print(f"cost vjp set {which} N {N} B {B}: du0*/dp {err_dp:.1e} -> bar {bar:.1e}; g_cost {fmt(e_all)}; dV/dcost {e_V:.1e}; "
              f"largest |g_cost| {np.abs(got).max():.2e}")
        if nx:
            print(f"cost vjp set {which} N {N} B {B}: active hard state row ({nx}): g_cost {fmt(e_x)}")
        assert max(e_all) <= bar and e_V <= bar, (which, N, bar, e_all, e_V)
        assert max(e_x) <= bar, (which, N, bar, e_x)
        if B > 1:
            # (among the instances whose plan moves with the cost: with every control on its bound, as at N = 2, the row is zero)
            ref = g14[key + "g_cost"][:, 0]
            moves = np.where(np.abs(ref).max(1) >= 1.0)[0]
            far = min(scaled(got[i:i + 1], ref[j:j + 1]) for i, j in zip(moves, np.roll(moves, -1)))
            print(f"cost vjp set {which} N {N} negative control ({len(moves)} instances): nearest neighbour's reference at {far:.1e}")
            assert len(moves) >= 2 and far > 100.0 * bar


# ---------------------------------------------------------------------- 2. the known answer, no fixture value
def value_formulas(X, U, theta, dT):
    """dV/dcost [B, 83] restated in float64 with torch on the host: dV/dW[a, b] = sum_k c_k 1/2 r_a r_b, dV/dyref[a] =
    -sum_k c_k (H r)_a, H = 1/2 (W + W'), c_k = dT on stages 0 .. N-1 and 1 on stage N."""
    from mpc4rl_amd import CartpoleCost, cartpole_cost_of, cartpole_theta
    X, U, theta = X.cpu(), U.cpu(), theta.cpu()
    c = cartpole_cost_of(theta)
    N = U.shape[1]
    y = torch.cat([X[:, :N], U], 2)      # [B, N, 5]
    sym = lambda W: 0.5 * (W + W.transpose(-1, -2))      # noqa: E731
    r0, r, re = y[:, 0] - c.yref_0, y[:, 1:] - c.yref[:, None], X[:, N] - c.yref_e
    grad = CartpoleCost(W_0=dT * 0.5 * r0[:, :, None] * r0[:, None, :],
                        W=dT * 0.5 * torch.einsum("bka,bkc->bac", r, r),
                        W_e=0.5 * re[:, :, None] * re[:, None, :],
                        yref_0=-dT * torch.einsum("bac,bc->ba", sym(c.W_0), r0),
                        yref=-dT * torch.einsum("bac,bkc->ba", sym(c.W), r),
                        yref_e=-torch.einsum("bac,bc->ba", sym(c.W_e), re))
    return cartpole_theta(torch.zeros((len(X), NDYN), dtype=torch.float64), grad)


@pytest.mark.parametrize("N", [2, 20])
def test_value_gradient_is_the_closed_form_on_the_stored_iterate(g14, N):
    """V mode and Q mode (u_0 pinned), per-instance theta with weights that are not symmetric: 1e-12."""
    ocp, _ = C.problem("cartpole", N)
    key = f"A_N{N}_"
    x0 = g14[key + "x0"][:5]
    theta = perturbed_theta(ocp.p0, 5, [7, N, 0])
    mpc = handle(ocp, 5, fixture_bounds(g14, key), theta=theta)
    u0 = None
    for _ in range(2):      # V mode, then u_0 pinned a tenth short of the control the V-mode solve found
        r = mpc.solve(x0, u0, cold=True)
        assert r.status.tolist() == [0] * 5
        X, U = mpc.get_iterate()[:2]
        got, ref = mpc.cost_value_grad(), value_formulas(X, U, mpc.get_theta(), ocp.dT)
        err = scaled(got, ref)
        print(f"cost value grad N {N} {'V' if u0 is None else 'Q'} mode against the closed form: {err:.1e}; largest {float(ref.abs().max()):.2e}")
        assert float(ref.abs().max()) > 1e-3 and err <= 1e-12
        assert same([got], [raw_value(mpc)])
        u0 = 0.9 * r.u0


@pytest.mark.parametrize("N", [2, 20])
def test_single_stage_blocks_satisfy_the_relation_between_their_w_and_yref_rows(g14, N):
    """Stage 0 and stage N are single-term blocks: g_W = -c 1/2 (y r' + r y') and g_yref = c H y with the same y.  With r from the
    stored iterate, s = y'r = -r' g_W r / (c |r|^2) and y = (-2 g_W r / c - s r) / |r|^2 recover y from the W rows alone, and
    c H y must then be the yref rows.  A handful of float64 operations divided by |r|^2 (0.01 .. 1 here) on gradients of up to 1e2:
    1e-9 in the scaled measure leaves three digits of margin over rounding and is far below any wrong sign, factor or index."""
    from mpc4rl_amd import cartpole_cost_of
    ocp, _ = C.problem("cartpole", N)
    key = f"A_N{N}_"
    x0 = g14[key + "x0"][:5]
    theta = perturbed_theta(ocp.p0, 5, [8, N, 0])
    mpc = handle(ocp, 5, fixture_bounds(g14, key), theta=theta)
    assert mpc.solve(x0, cold=True).status.tolist() == [0] * 5
    gX, gU = split(mpc, np.random.default_rng([9, N]).standard_normal((5, N + 4 * (N + 1))))
    g = cartpole_cost_of(mpc.cost_vjp(gX, gU, x0=False, theta=False)[4].cpu())
    X, U = (t.cpu() for t in mpc.get_iterate()[:2])
    c = cartpole_cost_of(mpc.get_theta().cpu())
    errs = []
    for gW, gy, W, r, ck in ((g.W_0, g.yref_0, c.W_0, torch.cat([X[:, 0], U[:, 0]], 1) - c.yref_0, ocp.dT),
                             (g.W_e, g.yref_e, c.W_e, X[:, N] - c.yref_e, 1.0)):
        rr = (r * r).sum(1, keepdim=True)
        gr = torch.einsum("bac,bc->ba", gW, r)
        s = -(r * gr).sum(1, keepdim=True) / (ck * rr)
        y = (-2.0 * gr / ck - s * r) / rr
        errs.append(scaled(gy, ck * torch.einsum("bac,bc->ba", 0.5 * (W + W.transpose(1, 2)), y)))
        assert float(gy.abs().max()) > 1e-3
    print(f"cost vjp N {N} relation between the W and the yref rows of stage 0, stage N: {fmt(errs)}")
    assert max(errs) <= 1e-9


# ---------------------------------------------------------------------- 3. contract, the same bits as mpcrl_bound_vjp
CP_BOUNDS = ([-8.0], [8.0], [-8.0, -0.6, -1.0, -0.4, -1.5], [8.0, 0.6, 1.0, 0.4, 1.5], [-0.6, -1.0, -0.4, -1.5], [0.6, 1.0, 0.4, 1.5])


@pytest.fixture(scope="module")
def cp16():
    """cartpole N 20, B 16 with the bounds of the fixture: the x0 of tests/test_gpu_bound_vjp.py (instance 5 NaN), a per-instance theta
    and one cotangent over all of w."""
    ocp, _ = C.problem("cartpole", 20)
    rng = np.random.default_rng(43)
    x0 = rng.uniform(-1, 1, (16, 4)) * np.array([0.5, 0.3, 0.3, 0.5])
    x0[5, 2] = float("nan")
    return ocp, x0, rng.standard_normal((16, 20 * 1 + 21 * 4)), perturbed_theta(ocp.p0, 16, [44, 0])


def test_every_output_combination_and_the_bits_of_bound_vjp(cp16):
    ocp, x0, G, theta = cp16
    mpc = handle(ocp, 16, CP_BOUNDS, theta=theta)
    r = mpc.solve(x0, cold=True)
    gX, gU = split(mpc, G)
    before = [t.clone() for t in (r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian())]
    full = raw_vjp(mpc, gX, gU)
    st = r.status.cpu().numpy()
    assert st[5] == 1 and np.all(np.delete(st, 5) == 0)
    assert all(torch.isfinite(t).all() for t in full)
    assert all(torch.all(t[5] == 0) for t in full)                  # a NaN-x0 instance gives zero rows
    g = full[4]
    assert torch.all(g[:, :NDYN] == 0) and symmetric_bits(g) and float(g[4, NDYN:].abs().max()) > 1e-3
    assert torch.all(g[:, 3:28].reshape(16, 5, 5)[:, :4, :4] == 0)  # x_0 = x0 does not move: the state block of W_0 is exactly zero
    assert torch.all(full[1][:, NDYN:] == 0)                        # g_theta keeps its zero cost block
    bound = raw_vjp(mpc, gX, gU, (True, True, True, True, False), name="mpcrl_bound_vjp")
    assert same(full[:4], bound[:4])                                # with g_cost requested: the bits of mpcrl_bound_vjp
    for want in itertools.product((False, True), repeat=5):         # the 31 non-empty combinations, NaN-poisoned buffers
        if any(want):
            got = raw_vjp(mpc, gX, gU, want)
            assert all((t is None) == (not w) for t, w in zip(got, want)) and same(got, [f if w else None for f, w in zip(full, want)]), want
    for a, b in ((gX, None), (None, gU)):                           # a NULL cotangent counts as zeros
        za, zb = (torch.zeros_like(gX) if a is None else a), (torch.zeros_like(gU) if b is None else b)
        assert same(raw_vjp(mpc, a, b), raw_vjp(mpc, za, zb))
    assert same(mpc.cost_vjp(gX, gU, bounds=True), full)            # the Python surface: the same numbers
    dV = raw_value(mpc)
    assert torch.isfinite(dV).all() and torch.all(dV[5] == 0) and torch.all(dV[:, :NDYN] == 0) and symmetric_bits(dV)
    assert torch.all(dV[4, [3, 28, 53]] > 0)                        # dV/dW[0, 0] = sum c 1/2 r_0^2
    assert same([mpc.cost_value_grad()], [dV])
    after = [r.u0, r.V, r.status, r.iters, *mpc.get_iterate(), mpc.get_lagrangian()]
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, after))      # (bytes: instance 5 holds NaN)


def test_refusals():
    from mpc4rl_amd import MPCBatch, MPCLayer, _lib, chain_mass_ocp, linear_system_ocp
    ocp, _ = C.problem("cartpole", 6)
    cp = handle(ocp, 3)
    x0 = np.array([[0.2, 0.1, 0.15, -0.2], [-0.3, 0.2, -0.2, 0.1], [0.1, 0.0, 0.1, 0.0]])
    gX, gU = split(cp, np.ones((3, 6 + 7 * 4)))
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(cp, gX, gU)                                         # before any solve
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(cp)
    with pytest.raises(RuntimeError):
        cp.cost_vjp(gX, gU)
    with pytest.raises(RuntimeError):
        cp.cost_value_grad()
    cp.solve(x0, cold=True)
    assert all(torch.isfinite(t).all() for t in raw_vjp(cp, gX, gU)) and torch.isfinite(raw_value(cp)).all()
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(cp, None, None)                                     # both cotangents NULL
    with pytest.raises(ValueError):
        cp.cost_vjp(None, None)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_vjp(cp, gX, gU, (False,) * 5)                           # all outputs NULL
    with pytest.raises(ValueError):
        cp.cost_vjp(gX, gU, x0=False, theta=False, bounds=False, cost=False)
    with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
        raw_value(cp, want=False)
    for flags in (_lib.STATE_Q_MODE, 4):                            # flags must be 0 on both calls
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw_vjp(cp, gX, gU, flags=flags)
        with pytest.raises(RuntimeError, match="MPCRL_E_ARG"):
            raw_value(cp, flags=flags)
    cp.solve(x0, np.full((3, 1), 0.1), cold=True)                   # a solve with u0 fixed: the value gradient is dQ/dcost, no VJP
    assert torch.isfinite(cp.cost_value_grad()).all()
    with pytest.raises(RuntimeError, match="Q mode"):
        cp.cost_vjp(gX, gU)
    lin = MPCBatch(linear_system_ocp(N=7), 3)
    lin.solve(np.array([[0.5, 0.1], [0.3, 0.2], [0.6, -0.1]]), cold=True)
    chain = MPCBatch(chain_mass_ocp(n_mass=3, N=10), 2)
    chain.solve(np.tile(chain.ocp.x0, (2, 1)), cold=True)
    for other in (lin, chain):
        oX, oU = split(other, np.ones((other.B, other.N * other.nu + (other.N + 1) * other.nx)))
        with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
            raw_vjp(other, oX, oU)
        with pytest.raises(RuntimeError, match="MPCRL_E_MODEL"):
            raw_value(other)
        with pytest.raises(RuntimeError, match="cartpole"):
            other.cost_vjp(oX, oU)
        with pytest.raises(RuntimeError, match="cartpole"):
            other.cost_value_grad()
        with pytest.raises(ValueError, match="cartpole"):
            MPCLayer(other, cost_gradient=True)


# ---------------------------------------------------------------------- 4. lane layouts and edges
@pytest.mark.parametrize("N", [2, 15, 20, 31, 32, 63])
def test_rows_are_written_in_full_and_nothing_beyond_b_at_every_lane_layout(g14, N):
    """B = 5 (no multiple of the 4, 3, 2 or 1 instances a wavefront holds at these horizons) and B = 1: every row of g_cost and of
    dV_dcost is written in full, the guard row behind the last instance keeps its sentinel, and an instance's row is the same bits
    under a reversed packing order, the time-sliced solve launch and a second call."""
    ocp, _ = C.problem("cartpole", N)
    key = f"A_N{N}_"
    bounds = fixture_bounds(g14, key)
    G = np.random.default_rng([10, N]).standard_normal((5, N + 4 * (N + 1)))
    ref = None
    for B, mode, perm in ((5, -1, None), (5, 1, None), (5, -1, torch.arange(4, -1, -1)), (1, -1, None)):
        mpc = handle(ocp, B, bounds, theta=perturbed_theta(ocp.p0, 5, [11, N, 0])[:B])
        mpc.set_launch_mode(mode)
        mpc.set_order(perm)
        assert mpc.solve(g14[key + "x0"][:B], cold=True, reorder=False).status.tolist() == [0] * B
        gX, gU = split(mpc, G[:B])
        out = []
        for _ in range(2):
            guarded = torch.full((2, B + 1, NP), float("nan"), dtype=torch.float64, device=mpc.device)
            guarded[:, B] = 7.25
            mpc._call("mpcrl_cost_vjp", 0, gX, gU, None, None, None, None, guarded[0])
            mpc._call("mpcrl_cost_value_grad", 0, guarded[1])
            torch.cuda.synchronize()
            assert torch.isfinite(guarded[:, :B]).all() and torch.all(guarded[:, B] == 7.25)
            assert torch.all(guarded[:, :B, :NDYN] == 0) and symmetric_bits(guarded[0, :B]) and symmetric_bits(guarded[1, :B])
            assert float(guarded[0, 0, NDYN:].abs().max()) > 1e-3 and torch.all(guarded[1, :B, 3] > 0)      # (instance 0 is off its bounds)
            out.append(guarded[:, :B].clone())
        assert same(out[:1], out[1:])
        if B == 5:
            ref = out[0] if ref is None else ref
            assert same([out[0]], [ref]), (N, mode, perm is not None)


# ---------------------------------------------------------------------- 5. Q mode
Q_ENTRIES = (3 + 4 * 5 + 0, 28 + 2 * 5 + 2, 53 + 3 * 4 + 1, 69 + 4, 74 + 2, 79 + 0)      # W_0[0, 4], W[2, 2], W_e[1, 3], yref_0[4], yref[2], yref_e[0]


def test_cost_value_grad_in_q_mode_against_differences_of_q(g14):
    """u_0 pinned: dQ/dcost on one entry of every block against central differences of Q over that entry of p alone (an off-diagonal
    entry of a weight moved on its own: every entry is an independent variable)."""
    N = 15
    ocp, _ = C.problem("cartpole", N)
    key = f"A_N{N}_"
    x0, u0 = g14[key + "x0"][:3], np.array([[0.4], [-0.3], [0.2]])
    theta = perturbed_theta(ocp.p0, 3, [12, 0])
    mpc = handle(ocp, 3, fixture_bounds(g14, key), tol=1e-10, theta=theta)
    assert mpc.solve(x0, u0, cold=True).status.tolist() == [0] * 3
    got = mpc.cost_value_grad()[:, list(Q_ENTRIES)].cpu().numpy()
    ref, h = np.zeros((3, len(Q_ENTRIES))), 1e-4
    for j, e in enumerate(Q_ENTRIES):
        Q = []
        for sgn in (1.0, -1.0):
            th = theta.copy()
            th[:, e] += sgn * h
            mpc.set_theta(th)
            rr = mpc.solve(x0, u0, cold=True)
            assert rr.status.tolist() == [0] * 3
            Q.append(rr.V.cpu().numpy())
        ref[:, j] = (Q[0] - Q[1]) / (2 * h)
    err = scaled(got, ref)
    print(f"cost value grad N {N} Q mode: dQ/d(W_0[0,4] W[2,2] W_e[1,3] yref_0[4] yref[2] yref_e[0]) against differences {err:.1e}; "
          f"smallest column {np.abs(ref).max(0).min():.2e}, largest {np.abs(ref).max():.2e}")
    assert np.abs(ref).max(0).min() > 1e-6 and err <= 1e-6


# ---------------------------------------------------------------------- 6. inside a graph
def test_replays_inside_a_graph(cp16):
    ocp, x0, G, theta = cp16
    mpc = handle(ocp, 16, CP_BOUNDS, theta=theta)
    mpc.solve(np.nan_to_num(x0, nan=0.1), cold=True)
    gX, gU = split(mpc, G)
    want = raw_vjp(mpc, gX, gU) + [raw_value(mpc)]
    bufs = [torch.zeros(sh, dtype=torch.float64, device=mpc.device) for sh in shapes(mpc) + ((mpc.B, mpc.n_p),)]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one stream: a chain of two nodes, no parallel branches
        mpc._call("mpcrl_cost_vjp", 0, gX, gU, *bufs[:5])
        mpc._call("mpcrl_cost_value_grad", 0, bufs[5])
    torch.cuda.synchronize()
    assert all(torch.all(t == 0) for t in bufs)      # captured, not run
    for _ in range(2):
        for t in bufs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same(bufs, want)


# ---------------------------------------------------------------------- 7. the layer
LAYER_ENTRIES = (3, 3 + 4 * 5 + 2, 28 + 2 * 5 + 2, 28 + 1 * 5 + 3, 53, 53 + 2 * 4 + 1, 69, 73, 75, 78, 79, 82)      # two per block


@pytest.mark.parametrize("with_bounds", [False, True])
def test_layer_cost_gradients_against_differences_of_its_forward_pass(g14, with_bounds):
    """MPCLayer(batch, cost_gradient=True), B 3, N 15, a shared theta: theta.grad on 12 entries of the cost block (two per block, off-
    diagonal entries of the weights among them) for a loss on u0 + V, a loss on (X, U) and q, against central differences of the
    layer's own forward pass.  x0.grad and the dynamics block of theta.grad are those of the default layer, whose cost block is
    exactly zero."""
    from mpc4rl_amd import BoxBounds, MPCLayer
    N, B = 15, 3
    ocp, _ = C.problem("cartpole", N)
    key = f"A_N{N}_"
    bounds = fixture_bounds(g14, key)
    x0 = torch.tensor(g14[key + "x0"][:B], device="cuda")
    u0q = torch.tensor([[0.4], [-0.3], [0.2]], dtype=torch.float64, device="cuda")
    theta0 = torch.tensor(perturbed_theta(ocp.p0, 1, [13, 0])[0], device="cuda")
    rng = np.random.default_rng(62)
    Wx, Wu = torch.tensor(rng.uniform(-1, 1, (B, N + 1, 4)), device="cuda"), torch.tensor(rng.uniform(-1, 1, (B, N, 1)), device="cuda")
    wu, wV = torch.tensor(rng.uniform(-1, 1, (B, 1)), device="cuda"), torch.tensor(rng.uniform(-1, 1, B), device="cuda")
    layer = MPCLayer(handle(ocp, B, bounds, tol=1e-10), cost_gradient=True, cold=True)
    plain = MPCLayer(handle(ocp, B, bounds, tol=1e-10), cold=True)

    def box():
        return BoxBounds(*(torch.tensor(b, dtype=torch.float64) for b in bounds)) if with_bounds else None

    def fwd_loss(lay, x, th):
        u0, V = lay(x, th, box())
        return (wu * u0).sum() + (wV * V).sum()

    def traj_loss(lay, x, th):
        X, U = lay.trajectory(x, th, box())
        return (Wx * X).sum() + (Wu * U).sum()

    def q_loss(lay, x, th):
        return (wV * lay.q(x, u0q, th)).sum()

    for name, loss in (("forward", fwd_loss), ("trajectory", traj_loss), ("q", q_loss)):
        x, theta = x0.clone().requires_grad_(True), theta0.clone().requires_grad_(True)
        loss(layer, x, theta).backward()
        assert layer.last_status.tolist() == [0] * B
        x2, theta2 = x0.clone().requires_grad_(True), theta0.clone().requires_grad_(True)
        loss(plain, x2, theta2).backward()
        assert torch.equal(x.grad, x2.grad) and torch.equal(theta.grad[:NDYN], theta2.grad[:NDYN])
        assert torch.all(theta2.grad[NDYN:] == 0)      # the default layer: exact zeros on the cost block
        fd = np.zeros(len(LAYER_ENTRIES))
        with torch.no_grad():
            for j, e in enumerate(LAYER_ENTRIES):
                f = []
                for sgn in (1.0, -1.0):
                    th = theta0.clone()
                    th[e] += sgn * 1e-5
                    f.append(float(loss(layer, x0, th)))
                    assert layer.last_status.tolist() == [0] * B
                fd[j] = (f[0] - f[1]) / 2e-5
        got = theta.grad[list(LAYER_ENTRIES)].cpu().numpy()
        err = scaled(got[None], fd[None])
        print(f"layer.{name} cartpole N {N} cost_gradient{' with bounds' if with_bounds else ''}: d loss/d (12 cost entries) {err:.1e}; "
              f"largest |gradient| {np.abs(fd).max():.2e}, smallest {np.abs(fd).min():.2e}")
        assert np.abs(fd).max() > 1e-2 and err <= 1e-5


def test_layer_per_instance_theta_staleness_and_failed_instance(g14):
    from mpc4rl_amd import MPCLayer
    N = 15
    ocp, _ = C.problem("cartpole", N)
    key = f"A_N{N}_"
    bounds = fixture_bounds(g14, key)
    x0 = torch.tensor(g14[key + "x0"][:2], device="cuda")
    theta = torch.tensor(perturbed_theta(ocp.p0, 2, [14, 0]), device="cuda")
    layer = MPCLayer(handle(ocp, 2, bounds, tol=1e-10), cost_gradient=True, cold=True)
    # theta [B, n_p]: a row per instance, and it is cost_vjp's + cost_value_grad's own numbers
    th = theta.clone().requires_grad_(True)
    X, U = layer.trajectory(x0, th)
    X.sum().backward()
    g_x0, g_th, _, _, g_c = layer.batch.cost_vjp(torch.ones_like(X), None)
    assert th.grad.shape == (2, NP) and torch.equal(th.grad, g_th + g_c)
    assert torch.all(th.grad[:, NDYN:].abs().amax(1) > 0)
    # the pass-counter rule covers the cost_vjp calls of both backward passes
    for f in (lambda: layer.trajectory(x0, th)[0].sum(), lambda: layer(x0, th)[0].sum()):
        out = f()
        layer(x0, theta)
        with pytest.raises(RuntimeError, match="one backward per forward"):
            out.backward()
    # an instance whose solve failed contributes exactly zero: the gradients are those of the other instance alone
    grads = []
    for xs in (x0[:1], torch.cat([x0[:1], torch.tensor([[0.1, 0.0, float("nan"), 0.0]], device="cuda")])):
        lay = MPCLayer(handle(ocp, len(xs), bounds, tol=1e-10), cost_gradient=True, cold=True)
        g = []
        for run in (lambda t: sum(torch.nan_to_num(o)[:1].sum() for o in lay.trajectory(xs, t)),
                    lambda t: sum(torch.nan_to_num(o).sum() for o in lay(xs, t)),
                    lambda t: torch.nan_to_num(lay.q(xs, torch.full((len(xs), 1), 0.2, dtype=torch.float64, device="cuda"), t)).sum()):
            t = theta[0].clone().requires_grad_(True)
            run(t).backward()
            assert lay.last_status.tolist() == [0, 1][:len(xs)]
            g.append(t.grad.clone())
        grads.append(g)
    assert all(torch.isfinite(t).all() and float(t[NDYN:].abs().max()) > 0 for t in grads[1]) and same(grads[0], grads[1])


MEASURED = """\
cost vjp set A N 2 B 5: du0*/dp 3.7e-08 -> bar 1.0e-06; g_cost 3.7e-07 6.0e-07 3.7e-08; dV/dcost 8.6e-11; largest |g_cost| 6.44e+01
cost vjp set A N 2 negative control (2 instances): nearest neighbour's reference at 1.1e+00
cost vjp set A N 2 B 1: du0*/dp 3.7e-08 -> bar 1.0e-06; g_cost 1.2e-08 6.3e-09 3.7e-08; dV/dcost 1.3e-13; largest |g_cost| 1.63e+01
cost vjp set A N 15 B 7: du0*/dp 9.0e-08 -> bar 1.0e-06; g_cost 5.3e-08 1.1e-07 7.2e-08; dV/dcost 4.2e-10; largest |g_cost| 4.41e+02
cost vjp set A N 15 B 7: active hard state row (2): g_cost 5.3e-08 1.1e-07 1.5e-09
cost vjp set A N 15 negative control (7 instances): nearest neighbour's reference at 4.7e-01
cost vjp set A N 15 B 1: du0*/dp 1.5e-11 -> bar 1.0e-06; g_cost 7.4e-09 9.9e-10 8.0e-09; dV/dcost 2.1e-10; largest |g_cost| 4.41e+02
cost vjp set A N 20 B 5: du0*/dp 4.6e-09 -> bar 1.0e-06; g_cost 3.1e-07 3.7e-07 6.6e-09; dV/dcost 3.9e-10; largest |g_cost| 5.52e+02
cost vjp set A N 20 B 5: active hard state row (1): g_cost 3.1e-07 3.7e-07 2.1e-10
cost vjp set A N 20 negative control (4 instances): nearest neighbour's reference at 2.9e-01
cost vjp set A N 20 B 1: du0*/dp 4.6e-09 -> bar 1.0e-06; g_cost 1.1e-09 1.9e-09 1.6e-09; dV/dcost 4.7e-11; largest |g_cost| 2.26e+02
cost vjp set A N 31 B 5: du0*/dp 2.3e-07 -> bar 1.0e-06; g_cost 3.0e-07 1.7e-07 1.6e-07; dV/dcost 2.4e-10; largest |g_cost| 5.59e+02
cost vjp set A N 31 B 5: active hard state row (2): g_cost 5.9e-08 1.7e-07 1.2e-10
cost vjp set A N 31 negative control (4 instances): nearest neighbour's reference at 1.0e+00
cost vjp set A N 31 B 1: du0*/dp 2.3e-07 -> bar 1.0e-06; g_cost 3.0e-07 1.9e-08 1.6e-07; dV/dcost 4.1e-11; largest |g_cost| 1.06e+02
cost vjp set A N 32 B 5: du0*/dp 3.6e-08 -> bar 1.0e-06; g_cost 5.1e-08 3.0e-08 1.9e-08; dV/dcost 3.6e-10; largest |g_cost| 6.58e+02
cost vjp set A N 32 B 5: active hard state row (1): g_cost 3.7e-10 2.7e-09 2.5e-10
cost vjp set A N 32 negative control (5 instances): nearest neighbour's reference at 7.2e-01
cost vjp set A N 32 B 1: du0*/dp 2.4e-08 -> bar 1.0e-06; g_cost 5.1e-08 3.0e-08 1.9e-08; dV/dcost 3.6e-10; largest |g_cost| 3.83e+02
cost vjp set A N 63 B 6: du0*/dp 5.6e-08 -> bar 1.0e-06; g_cost 2.8e-07 2.1e-07 6.3e-08; dV/dcost 7.4e-10; largest |g_cost| 1.43e+03
cost vjp set A N 63 B 6: active hard state row (2): g_cost 2.0e-08 2.1e-07 6.0e-10
cost vjp set A N 63 negative control (6 instances): nearest neighbour's reference at 8.1e-01
cost vjp set A N 63 B 1: du0*/dp 5.2e-08 -> bar 1.0e-06; g_cost 4.6e-09 9.1e-10 5.4e-09; dV/dcost 1.6e-10; largest |g_cost| 2.50e+02
cost vjp set B N 2 B 4: du0*/dp 1.5e-09 -> bar 1.0e-06; g_cost 2.5e-08 2.4e-08 5.8e-08; dV/dcost 3.8e-11; largest |g_cost| 4.76e+01
cost vjp set B N 2 negative control (4 instances): nearest neighbour's reference at 1.4e+00
cost vjp set B N 2 B 1: du0*/dp 4.5e-12 -> bar 1.0e-06; g_cost 4.2e-09 3.6e-09 1.3e-08; dV/dcost 1.3e-11; largest |g_cost| 3.85e+01
cost vjp set B N 15 B 4: du0*/dp 3.3e-08 -> bar 1.0e-06; g_cost 8.5e-08 2.1e-08 4.3e-09; dV/dcost 1.8e-10; largest |g_cost| 1.83e+02
cost vjp set B N 15 B 4: active hard state row (1): g_cost 8.5e-08 1.9e-08 5.5e-12
cost vjp set B N 15 negative control (4 instances): nearest neighbour's reference at 1.0e+00
cost vjp set B N 15 B 1: du0*/dp 2.5e-09 -> bar 1.0e-06; g_cost 8.1e-10 2.6e-09 3.6e-09; dV/dcost 7.3e-12; largest |g_cost| 5.91e+01
cost vjp set B N 20 B 4: du0*/dp 1.0e-07 -> bar 1.0e-06; g_cost 5.3e-09 2.5e-08 1.2e-08; dV/dcost 8.7e-11; largest |g_cost| 3.72e+02
cost vjp set B N 20 negative control (4 instances): nearest neighbour's reference at 1.4e+00
cost vjp set B N 20 B 1: du0*/dp 1.0e-07 -> bar 1.0e-06; g_cost 5.3e-09 1.4e-08 1.2e-08; dV/dcost 4.0e-11; largest |g_cost| 1.90e+02
cost vjp set B N 32 B 4: du0*/dp 3.3e-07 -> bar 1.3e-06; g_cost 1.2e-07 5.4e-07 9.7e-08; dV/dcost 2.3e-09; largest |g_cost| 1.48e+02
cost vjp set B N 32 B 4: active hard state row (1): g_cost 1.2e-07 2.9e-07 6.5e-08
cost vjp set B N 32 negative control (4 instances): nearest neighbour's reference at 1.1e+00
cost vjp set B N 32 B 1: du0*/dp 3.3e-07 -> bar 1.3e-06; g_cost 1.1e-07 5.4e-07 9.7e-08; dV/dcost 4.8e-12; largest |g_cost| 6.77e+01
cost value grad N 2 V mode against the closed form: 6.2e-17; largest 4.98e+00
cost value grad N 2 Q mode against the closed form: 1.0e-16; largest 4.98e+00
cost value grad N 20 V mode against the closed form: 4.7e-16; largest 8.80e+00
cost value grad N 20 Q mode against the closed form: 3.5e-16; largest 8.80e+00
cost vjp N 2 relation between the W and the yref rows of stage 0, stage N: 1.4e-15 6.7e-16
cost vjp N 20 relation between the W and the yref rows of stage 0, stage N: 1.0e-14 8.5e-16
cost value grad N 15 Q mode: dQ/d(W_0[0,4] W[2,2] W_e[1,3] yref_0[4] yref[2] yref_e[0]) against differences 1.6e-09; smallest column 1.98e-03, largest 3.63e+00
layer.forward cartpole N 15 cost_gradient: d loss/d (12 cost entries) 8.2e-11; largest |gradient| 6.23e+00, smallest 1.88e-03
layer.trajectory cartpole N 15 cost_gradient: d loss/d (12 cost entries) 5.8e-09; largest |gradient| 1.33e+01, smallest 0.00e+00
layer.q cartpole N 15 cost_gradient: d loss/d (12 cost entries) 2.6e-11; largest |gradient| 6.11e-01, smallest 6.61e-05
layer.forward cartpole N 15 cost_gradient with bounds: d loss/d (12 cost entries) 8.2e-11; largest |gradient| 6.23e+00, smallest 1.88e-03
layer.trajectory cartpole N 15 cost_gradient with bounds: d loss/d (12 cost entries) 5.8e-09; largest |gradient| 1.33e+01, smallest 0.00e+00
layer.q cartpole N 15 cost_gradient with bounds: d loss/d (12 cost entries) 2.6e-11; largest |gradient| 6.11e-01, smallest 6.61e-05
"""
