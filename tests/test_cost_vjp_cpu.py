"""The derivatives with respect to the cartpole's tracking cost without a GPU: the eighth header include/mpcrl_cost_ext.h parses into
a table of its own and the library exports it, the other seven tables are as they were, the fixture G14 (tests/golden/make_cost_vjp.py)
holds what its generator promises, ``cartpole_cost_of`` / ``cartpole_theta`` on hand-made tensors, and the layer's calls with and
without ``cost_gradient`` on a stub batch with CPU tensors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SETS = [("A", N) for N in (2, 15, 20, 31, 32, 63)] + [("B", N) for N in (2, 15, 20, 32)]
NP, NDYN = 83, 3
W_BLOCKS = ((3, 5), (28, 5), (53, 4))


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(GOLD, "g14_cost_vjp.npz"))


@pytest.fixture(scope="module")
def generator():
    sys.path.insert(0, GOLD)
    try:
        import make_cost_vjp
    finally:
        sys.path.remove(GOLD)
    return make_cost_vjp


# ---------------------------------------------------------------------- the eighth header and the library
def test_cost_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.COST_EXT_EXPORTS == ["mpcrl_cost_ext_version", "mpcrl_cost_value_grad", "mpcrl_cost_vjp"]
    assert _lib.COST_EXT_HEADER.constants == {"COST_EXT_VERSION": 1} and _lib.COST_EXT_VERSION == 1
    f = _lib.COST_EXT_HEADER.functions
    assert f["mpcrl_cost_ext_version"] == ("int", [])
    assert f["mpcrl_cost_value_grad"] == ("int", [("h", "handle"), ("flags", "int"), ("dV_dcost", "double*"), ("stream", "void*")])
    assert f["mpcrl_cost_vjp"] == ("int", [("h", "handle"), ("flags", "int"), ("gX", "double*"), ("gU", "double*"), ("g_x0", "double*"),
                                           ("g_theta", "double*"), ("g_lb", "double*"), ("g_ub", "double*"), ("g_cost", "double*"),
                                           ("stream", "void*")])
    assert not _lib.COST_EXT_HEADER.spec_fields
    assert os.path.basename(_lib.COST_EXT_HEADER_PATH) == "mpcrl_cost_ext.h"


def test_the_other_seven_tables_are_as_they_were():
    from mpc4rl_amd import _lib
    assert len(_lib.EXPORTS) == 68 and _lib.EXT_EXPORTS == ["mpcrl_ext_version", "mpcrl_state_sens"]
    assert _lib.CHAIN_EXT_EXPORTS == ["mpcrl_chain_ext_version", "mpcrl_chain_policy_state_sens"]
    assert _lib.TRAJ_EXT_EXPORTS == ["mpcrl_traj_ext_version", "mpcrl_traj_vjp"]
    assert _lib.CHAIN_TRAJ_EXT_EXPORTS == ["mpcrl_chain_traj_ext_version", "mpcrl_chain_traj_vjp"]
    assert _lib.BOUND_EXT_EXPORTS == ["mpcrl_bound_ext_version", "mpcrl_bound_value_grad", "mpcrl_bound_vjp", "mpcrl_chain_bound_vjp"]
    assert _lib.PROBE_EXT_EXPORTS[0] == "mpcrl_probe_ext_version"
    others = (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER, _lib.CHAIN_TRAJ_EXT_HEADER, _lib.BOUND_EXT_HEADER,
              _lib.PROBE_EXT_HEADER)
    for other in others:
        assert "COST_EXT_VERSION" not in other.constants and not set(_lib.COST_EXT_EXPORTS) & set(other.functions)
    assert _lib.ABI_VERSION == 132 and _lib.EXT_VERSION == 1 and _lib.CHAIN_EXT_VERSION == 1 and _lib.TRAJ_EXT_VERSION == 1
    assert _lib.CHAIN_TRAJ_EXT_VERSION == 1 and _lib.BOUND_EXT_VERSION == 1 and _lib.PROBE_EXT_VERSION == _lib.PROBE_EXT_HEADER.constants["PROBE_EXT_VERSION"]


def test_library_exports_every_symbol_of_the_cost_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.COST_EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_cost_ext.h but not exported"
    lib.mpcrl_cost_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_cost_ext_version() == _lib.COST_EXT_VERSION


def test_package_exports_the_cost_surface():
    import mpc4rl_amd
    assert mpc4rl_amd.CartpoleCost._fields == ("W_0", "W", "W_e", "yref_0", "yref", "yref_e")
    for name in ("CartpoleCost", "cartpole_cost_of", "cartpole_theta"):
        assert name in mpc4rl_amd.__all__ and hasattr(mpc4rl_amd, name)
    for name in ("cost_vjp", "cost_value_grad"):
        assert hasattr(mpc4rl_amd.MPCBatch, name)


# ---------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("which,N", SETS)
def test_fixture_shapes_gate_and_structure(g14, generator, which, N):
    k = f"{which}_N{N}_"
    nw = N + 4 * (N + 1)
    B = len(g14[k + "x0"])
    assert float(g14["gate"]) == 1e-6 == generator.GATE and float(g14["tol"]) == 1e-10
    assert g14[k + "x0"].shape == (B, 4) and g14[k + "p"].shape == (B, NP) and g14[k + "G"].shape == (B, 3, nw)
    assert g14[k + "g_cost"].shape == (B, 3, NP) and g14[k + "dV_dcost"].shape == (B, NP) and g14[k + "dpi_dp"].shape == (B, 1, NDYN)
    assert g14[k + "act_lb"].shape == g14[k + "act_ub"].shape == (B, N + 1, 5)
    assert np.isfinite(g14[k + "g_cost"]).all() and np.isfinite(g14[k + "dV_dcost"]).all()
    unit = np.zeros(nw)
    unit[0] = 1.0
    assert np.all(g14[k + "G"][:, 2] == unit)
    assert np.all(g14[k + "agree"] <= 1e-6) and np.all(g14[k + "agree_V"] <= 1e-6)
    # the exact zeros on the dynamics block, the same bits on W[a, b] and W[b, a]
    assert np.all(g14[k + "g_cost"][..., :NDYN] == 0) and np.all(g14[k + "dV_dcost"][:, :NDYN] == 0)
    for o, n in W_BLOCKS:
        for g in (g14[k + "g_cost"], g14[k + "dV_dcost"]):
            blk = g[..., o:o + n * n].reshape(g.shape[:-1] + (n, n))
            assert np.array_equal(blk, np.swapaxes(blk, -1, -2))
    # dV/dW[a, a] = sum c 1/2 r_a^2 > 0 on the state diagonal, and the gradients are not small
    assert np.all(g14[k + "dV_dcost"][:, [3, 53]] > 0)
    assert np.abs(g14[k + "g_cost"][:, :2]).max() >= 1.0
    # G13's bounds and classes
    ub = generator.bounded("cartpole", N).ubu[0]
    assert np.array_equal(g14[k + "ub"], [ub, 0.6, 1.0, 0.4, 1.5]) and np.array_equal(g14[k + "lb"], -g14[k + "ub"])
    assert np.array_equal(g14[k + "ube"], [0.6, 1.0, 0.4, 1.5]) and np.array_equal(g14[k + "lbe"], -g14[k + "ube"])
    assert np.array_equal(g14[k + "lb0"], g14[k + "lb"][:1]) and np.array_equal(g14[k + "ub0"], g14[k + "ub"][:1])
    act = g14[k + "act_lb"] | g14[k + "act_ub"]
    assert np.array_equal(g14[k + "interior"], ~act.any((1, 2))) and np.array_equal(g14[k + "act_u0"], act[:, 0, :1].any(1))
    assert np.array_equal(g14[k + "act_u"], act[:, 1:, :1].any((1, 2))) and np.array_equal(g14[k + "act_x"], act[:, :, 1:].any((1, 2)))


@pytest.mark.parametrize("which,N", SETS)
def test_fixture_counts_and_parameters(g14, generator, which, N):
    k = f"{which}_N{N}_"
    p0 = generator.bounded("cartpole", N).p0
    if which == "A":
        g13 = np.load(os.path.join(GOLD, "g13_bound_vjp.npz"))
        assert generator.REQUIRED_A == 5 and generator.ACT_X_AT == (15, 20, 32, 63) and generator.HORIZONS_A == (2, 15, 20, 31, 32, 63)
        assert len(g14[k + "x0"]) >= 5 and np.all(g14[k + "p"] == p0)
        rows = [int(np.where((g13[f"cartpole_N{N}_x0"] == x).all(1))[0][0]) for x in g14[k + "x0"]]      # G13's own instances
        assert rows == sorted(set(rows))
        for c in generator.CLASSES:
            assert np.array_equal(g14[k + c], g13[f"cartpole_N{N}_{c}"][rows])
        if N in (15, 20, 32, 63):
            assert g14[k + "act_x"].any()
    else:
        assert generator.REQUIRED_B == 3 and generator.DRAWS_B == 64 and generator.HORIZONS_B == (2, 15, 20, 32)
        assert len(g14[k + "x0"]) >= 3 and (g14[k + "act_u"] | g14[k + "act_u0"]).any()
        assert np.all(np.abs(g14[k + "x0"]) <= generator.X0_SCALE) and np.all(g14[k + "p"][:, :NDYN] == p0[:NDYN])
        for o, n in W_BLOCKS:      # not symmetric, not diagonal, positive definite in the symmetric part
            W = np.swapaxes(g14[k + "p"][:, o:o + n * n].reshape(-1, n, n), 1, 2)
            assert np.all(np.abs(W - np.swapaxes(W, 1, 2)).max((1, 2)) > 1e-3)
            assert np.all(np.linalg.eigvalsh(0.5 * (W + np.swapaxes(W, 1, 2))) > 0)
        assert np.all(np.abs(g14[k + "p"][:, 69:]).max(1) > 1e-2)


def test_unit_cotangent_row_is_zero_where_u0_sits_on_its_bound(g14):
    """u_0 on its bound does not move with the cost."""
    seen = 0
    for which, N in SETS:
        k = f"{which}_N{N}_"
        on = g14[k + "act_u0"]
        seen += int(on.sum())
        assert np.abs(g14[k + "g_cost"][on][:, 2]).max(initial=0.0) <= 1e-6
        assert np.all(np.abs(g14[k + "g_cost"][~on][:, 2]).max(1) > 1e-3)
    assert seen >= 10


# ---------------------------------------------------------------------- cartpole_cost_of / cartpole_theta
def test_cost_of_and_theta_round_trip_layout_and_gradient():
    from mpc4rl_amd import CartpoleCost, cartpole_cost_of, cartpole_theta
    theta = torch.arange(NP, dtype=torch.float64)
    c = cartpole_cost_of(theta)
    assert [tuple(t.shape) for t in c] == [(5, 5), (5, 5), (4, 4), (5,), (5,), (4,)]
    assert c.W_0[1, 2] == 3 + 2 * 5 + 1 and c.W[4, 0] == 28 + 4 and c.W_e[0, 3] == 53 + 3 * 4      # column-major: [a, b] at b n + a
    assert c.yref_0.tolist() == [69.0, 70.0, 71.0, 72.0, 73.0] and c.yref[0] == 74 and c.yref_e.tolist() == [79.0, 80.0, 81.0, 82.0]
    assert torch.equal(cartpole_theta(theta[:NDYN], c), theta)
    batched = torch.randn(2, 3, NP, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    cb = cartpole_cost_of(batched)
    assert cb.W_e.shape == (2, 3, 4, 4) and torch.equal(cb.W[1, 2], cartpole_cost_of(batched[1, 2]).W)
    assert torch.equal(cartpole_theta(batched[..., :NDYN], cb), batched)
    assert cartpole_theta(theta[:NDYN], tuple(cb)).shape == (2, 3, NP)      # a shared dynamics block broadcasts
    # differentiable both ways: a loss on W[a, b] lands on that entry of theta, and the other way round
    th = theta.clone().requires_grad_(True)
    cc = cartpole_cost_of(th)
    (2.0 * cc.W[1, 3] + 3.0 * cc.yref_e[2] + 5.0 * cc.W_e[2, 0]).backward()
    want = torch.zeros(NP, dtype=torch.float64)
    want[28 + 3 * 5 + 1], want[81], want[53 + 2] = 2.0, 3.0, 5.0
    assert torch.equal(th.grad, want)
    leaves = CartpoleCost(*(t.detach().clone().requires_grad_(True) for t in c))
    dyn = theta[:NDYN].clone().requires_grad_(True)
    w = torch.arange(NP, dtype=torch.float64) + 1.0
    (w * cartpole_theta(dyn, leaves)).sum().backward()
    assert torch.equal(dyn.grad, w[:NDYN]) and torch.equal(leaves.W.grad, cartpole_cost_of(w).W) and torch.equal(leaves.yref_0.grad, w[69:74])
    with pytest.raises(ValueError):
        cartpole_cost_of(theta[:-1])
    with pytest.raises(ValueError):
        cartpole_theta(theta[:2], c)
    with pytest.raises(ValueError):
        cartpole_theta(theta[:NDYN], c._replace(W_e=c.W))


# ---------------------------------------------------------------------- the layer, on a stub batch with CPU tensors
class StubBatch:
    """What the layer touches of an MPCBatch.  x_{k+1} = x_k + 1, u = 1; the derivative calls answer with recognisable numbers: g_theta
    ones, g_cost 3 on the cost block (entries 2 ..), dV/dcost 0.5 there, dV/dp ones, du0*/dp ones."""

    def __init__(self, name="cartpole", B=2, N=3, nx=2, nu=1, n_p=5):
        self.ocp = type("O", (), {"name": name})()
        self.B, self.N, self.nx, self.nu, self.n_p = B, N, nx, nu, n_p
        self.calls = []

    fail = 0

    def cost_block(self, v):
        g = torch.full((self.B, self.n_p), float(v), dtype=torch.float64)
        g[:, :2] = 0.0
        if self.fail:
            g[-1] = float("nan")      # what a failed instance leaves must never reach a gradient
        return g

    def set_theta(self, theta):
        self.theta = theta

    def set_bounds(self, which, lb, ub):
        self.calls.append(("set_bounds", which))

    def solve(self, x0, u0=None, **kw):
        self.x0 = x0
        self.calls.append(("solve", u0 is not None, kw))
        f64 = dict(dtype=torch.float64)
        return type("R", (), {"status": torch.tensor([0] * (self.B - 1) + [self.fail], dtype=torch.int32), "u0": torch.ones((self.B, self.nu), **f64),
                              "V": torch.ones(self.B, **f64), "dV_dp": torch.ones((self.B, self.n_p), **f64) if kw.get("sens_v") else None,
                              "dpi_dp": torch.ones((self.B, self.nu, self.n_p), **f64) if kw.get("sens_pi") else None})()

    def state_sens(self, **kw):
        self.calls.append(("state_sens", kw))
        f64 = dict(dtype=torch.float64)
        return type("S", (), {"dpi_dx0": torch.ones((self.B, self.nu, self.nx), **f64), "dV_dx0": torch.ones((self.B, self.nx), **f64),
                              "dQ_du0": torch.ones((self.B, self.nu), **f64)})()

    def get_iterate(self):
        X = self.x0[:, None, :] + torch.arange(self.N + 1, dtype=torch.float64)[None, :, None]
        return X, torch.ones((self.B, self.N, self.nu), dtype=torch.float64), None, None, None

    def trajectory_vjp(self, gX, gU, x0=True, theta=True):
        self.calls.append(("vjp", gX is not None, gU is not None, x0, theta))
        gx = torch.zeros((self.B, self.nx), dtype=torch.float64) if gX is None else gX.sum(1)
        return (gx if x0 else None), (torch.ones((self.B, self.n_p), dtype=torch.float64) if theta else None)

    def bound_value_grad(self, q_mode=False):
        self.calls.append(("bound_value_grad", q_mode))
        one = torch.ones((self.B, self.N + 1, self.nu + self.nx), dtype=torch.float64)
        return 0.5 * one, -0.25 * one

    def cost_value_grad(self):
        self.calls.append(("cost_value_grad",))
        return self.cost_block(0.5)

    def cost_vjp(self, gX, gU, x0=True, theta=True, bounds=False, cost=True):
        self.calls.append(("cost_vjp", gX is not None, gU is not None, x0, theta, bounds, cost))
        one = torch.ones((self.B, self.N + 1, self.nu + self.nx), dtype=torch.float64)
        gx = torch.zeros((self.B, self.nx), dtype=torch.float64) if gX is None else gX.sum(1)
        good = torch.tensor([True] * (self.B - 1) + [not self.fail]).reshape(-1, 1)      # MPCBatch.cost_vjp selects by status itself
        g_c = torch.where(good, self.cost_block(3.0), torch.zeros(())) if cost else None
        return ((gx if x0 else None), (torch.ones((self.B, self.n_p), dtype=torch.float64) if theta else None),
                (one if bounds else None), (2.0 * one if bounds else None), g_c)

    def fold_bound_grad(self, g):
        from mpc4rl_amd import MPCBatch
        return MPCBatch.fold_bound_grad(self, g)


def box(grad=("lb", "ub")):
    from mpc4rl_amd import BoxBounds
    v = dict(lb0=[-1.0], ub0=[1.0], lb=[-1.0, -2.0, -3.0], ub=[1.0, 2.0, 3.0], lbe=[-4.0, -5.0], ube=[4.0, 5.0])
    return BoxBounds(**{k: torch.tensor(x, dtype=torch.float64, requires_grad=k in grad) for k, x in v.items()})


def inputs(shared=True):
    x0 = torch.zeros((2, 2), dtype=torch.float64, requires_grad=True)
    theta = torch.ones(5 if shared else (2, 5), dtype=torch.float64, requires_grad=True)
    return x0, theta


def test_cost_gradient_is_opt_in_and_cartpole_only():
    from mpc4rl_amd import MPCLayer
    assert MPCLayer(StubBatch()).cost_gradient is False and MPCLayer(StubBatch(), cost_gradient=True).cost_gradient is True
    for name in ("linear_system", "chain_mass_3"):
        assert MPCLayer(StubBatch(name)).cost_gradient is False
        with pytest.raises(ValueError, match="cartpole"):
            MPCLayer(StubBatch(name), cost_gradient=True)


def test_layer_without_the_opt_in_makes_exactly_the_calls_it_made():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub, cold=True)
    x0, theta = inputs()
    X, U = layer.trajectory(x0, theta)
    X.sum().backward()
    assert stub.calls == [("solve", False, {"cold": True}), ("vjp", True, False, True, True)]
    stub.calls.clear()
    u0, V = layer(x0, theta)
    (u0.sum() + V.sum()).backward()
    assert stub.calls == [("solve", False, {"sens_v": True, "sens_pi": True, "cold": True}),
                          ("state_sens", {"q_mode": False, "value": True, "policy": True})]
    stub.calls.clear()
    layer.q(x0, torch.ones((2, 1), dtype=torch.float64), theta).sum().backward()
    assert stub.calls == [("solve", True, {"sens_v": True, "cold": True}), ("state_sens", {"q_mode": True, "value": True, "policy": False})]
    assert all(c[0] not in ("cost_vjp", "cost_value_grad") for c in stub.calls)


def test_layer_trajectory_with_cost_gradient_is_one_cost_vjp():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub, cost_gradient=True, cold=True)
    x0, theta = inputs()
    X, U = layer.trajectory(x0, theta)
    assert stub.calls == [("solve", False, {"cold": True})] and layer.pass_counter == 1
    (X.sum() + U.sum()).backward()
    assert stub.calls[1:] == [("cost_vjp", True, True, True, True, False, True)]      # ONE call for everything that requires a gradient
    # g_theta ones + g_cost 3 on the cost block, summed over the batch of 2
    assert theta.grad.tolist() == [2.0, 2.0, 8.0, 8.0, 8.0] and torch.all(x0.grad == 4.0)
    # with bounds: still one call, which serves them too
    stub.calls.clear()
    x0, theta = inputs(shared=False)
    b = box()
    X, U = layer.trajectory(x0, theta, b)
    assert [c[0] for c in stub.calls] == ["set_bounds"] * 3 + ["solve"]
    X.sum().backward()
    assert stub.calls[4:] == [("cost_vjp", True, False, True, True, True, True)]
    assert theta.grad.tolist() == [[1.0, 1.0, 4.0, 4.0, 4.0]] * 2      # a row per instance
    assert b.lb.grad.tolist() == [4.0] * 3 and b.ub.grad.tolist() == [8.0] * 3 and b.lb0.grad is None
    # theta without a gradient: the cost output is not asked for
    stub.calls.clear()
    X, U = layer.trajectory(x0, theta.detach())
    U.sum().backward()
    assert stub.calls[-1] == ("cost_vjp", False, True, True, False, False, False)


def test_layer_forward_and_q_with_cost_gradient():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub, cost_gradient=True)
    x0, theta = inputs()
    u0, V = layer(x0, theta)
    assert [c[0] for c in stub.calls] == ["solve", "state_sens", "cost_value_grad"]      # dV/dcost in forward: theta needs a gradient
    (3.0 * u0.sum() + 2.0 * V.sum()).backward()
    assert stub.calls[3:] == [("cost_vjp", False, True, False, False, False, True)]      # g_u on stage 0 of U*
    # MPCFunction's terms 3 + 2 = 5 per instance; the cost block adds 3 (vjp) + 2 * 0.5 (value) = 4; two instances
    assert theta.grad.tolist() == [10.0, 10.0, 18.0, 18.0, 18.0] and torch.all(x0.grad == 5.0)
    # the loss reads V alone: no adjoint solve
    stub.calls.clear()
    x0, theta = inputs()
    u0, V = layer(x0, theta)
    V.sum().backward()
    assert all(c[0] != "cost_vjp" for c in stub.calls) and theta.grad.tolist() == [2.0, 2.0, 3.0, 3.0, 3.0]
    # bounds as well: the one cost_vjp serves both
    stub.calls.clear()
    x0, theta = inputs()
    b = box()
    u0, V = layer(x0, theta, b)
    assert [c[0] for c in stub.calls] == ["set_bounds"] * 3 + ["solve", "state_sens", "bound_value_grad", "cost_value_grad"]
    (3.0 * u0.sum() + 2.0 * V.sum()).backward()
    assert stub.calls[7:] == [("cost_vjp", False, True, False, False, True, True)]
    assert theta.grad.tolist() == [10.0, 10.0, 18.0, 18.0, 18.0]
    assert b.lb.grad.tolist() == [8.0] * 3 and b.ub.grad.tolist() == [6.0] * 3      # the numbers of MPCBoundedFunction (test_bound_vjp_cpu.py)
    # theta without a gradient, no bounds: neither call
    stub.calls.clear()
    u0, V = layer(x0, theta.detach())
    (u0.sum() + V.sum()).backward()
    assert [c[0] for c in stub.calls] == ["solve", "state_sens"]
    # q: g_Q dQ/dcost on top of g_Q dQ/dp
    stub.calls.clear()
    x0, theta = inputs()
    Q = layer.q(x0, torch.ones((2, 1), dtype=torch.float64), theta)
    assert [c[0] for c in stub.calls] == ["solve", "state_sens", "cost_value_grad"]
    (2.0 * Q).sum().backward()
    assert theta.grad.tolist() == [4.0, 4.0, 6.0, 6.0, 6.0] and len(stub.calls) == 3


def test_a_failed_instance_contributes_zero():
    """Its rows (NaN in the stub) are selected out, not multiplied by zero."""
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    stub.fail = 4
    layer = MPCLayer(stub, cost_gradient=True)
    x0, theta = inputs()
    u0, V = layer(x0, theta)
    (3.0 * u0.sum() + 2.0 * V.sum()).backward()
    assert theta.grad.tolist() == [5.0, 5.0, 9.0, 9.0, 9.0]      # the other instance alone
    x0, theta = inputs(shared=False)
    X, U = layer.trajectory(x0, theta)
    X.sum().backward()
    assert theta.grad[1, 2:].tolist() == [1.0] * 3 and theta.grad[0].tolist() == [1.0, 1.0, 4.0, 4.0, 4.0]      # (g_theta is the stub's own ones)
    x0, theta = inputs()
    layer.q(x0, torch.ones((2, 1), dtype=torch.float64), theta).sum().backward()
    assert theta.grad.tolist() == [1.0, 1.0, 1.5, 1.5, 1.5]


def test_pass_counter_rule_covers_the_cost_paths():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub, cost_gradient=True)
    x0, theta = inputs()
    for first in ("trajectory", "forward"):
        out = layer.trajectory(x0, theta) if first == "trajectory" else layer(x0, theta)
        seen = layer.pass_counter
        layer.trajectory(x0.detach(), theta.detach())      # another pass: the handle's iterate is no longer this one's
        assert layer.pass_counter == seen + 1
        n = len(stub.calls)
        with pytest.raises(RuntimeError, match="one backward per forward"):
            out[0].sum().backward()
        assert all(c[0] != "cost_vjp" for c in stub.calls[n:])      # refused before the library is asked
