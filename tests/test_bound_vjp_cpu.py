"""The derivatives with respect to the box bounds without a GPU: the sixth header include/mpcrl_bound_ext.h parses into a table of its
own and the library exports it, the other five tables are as they were, the fixture G13 (tests/golden/make_bound_vjp.py) holds what
its generator promises, ``fold_bound_grad`` on a hand-made tensor, and the layer's calls on a stub batch with CPU tensors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
DIMS = {"cartpole": (4, 1, 83), "linear": (2, 1, 12)}
CHAIN_SETS = {"m3_N10_act_": (3, 10), "m3_N10_x0_": (3, 10), "m5_N8_ss_": (5, 8)}
SMALL = [(m, N) for m in HORIZONS for N in HORIZONS[m]]


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLD, "g13_bound_vjp.npz"))


@pytest.fixture(scope="module")
def generator():
    sys.path.insert(0, GOLD)
    try:
        import make_bound_vjp
    finally:
        sys.path.remove(GOLD)
    return make_bound_vjp


# ---------------------------------------------------------------------- the sixth header and the library
def test_bound_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.BOUND_EXT_EXPORTS == ["mpcrl_bound_ext_version", "mpcrl_bound_value_grad", "mpcrl_bound_vjp", "mpcrl_chain_bound_vjp"]
    assert _lib.BOUND_EXT_HEADER.constants["BOUND_EXT_VERSION"] == _lib.BOUND_EXT_VERSION == 1
    f = _lib.BOUND_EXT_HEADER.functions
    assert f["mpcrl_bound_ext_version"] == ("int", [])
    assert f["mpcrl_bound_value_grad"] == ("int", [("h", "handle"), ("flags", "int"), ("dV_dlb", "double*"), ("dV_dub", "double*"),
                                                   ("stream", "void*")])
    assert f["mpcrl_bound_vjp"] == ("int", [("h", "handle"), ("flags", "int"), ("gX", "double*"), ("gU", "double*"), ("g_x0", "double*"),
                                            ("g_theta", "double*"), ("g_lb", "double*"), ("g_ub", "double*"), ("stream", "void*")])
    assert f["mpcrl_chain_bound_vjp"] == ("int", [("h", "handle"), ("flags", "int"), ("status", "int32*"), ("gX", "double*"),
                                                  ("gU", "double*"), ("g_x0", "double*"), ("g_theta", "double*"), ("g_lb", "double*"),
                                                  ("g_ub", "double*"), ("stream", "void*")])
    assert not _lib.BOUND_EXT_HEADER.spec_fields
    assert os.path.basename(_lib.BOUND_EXT_HEADER_PATH) == "mpcrl_bound_ext.h"


def test_the_other_five_tables_are_as_they_were():
    from mpc4rl_amd import _lib
    assert len(_lib.EXPORTS) == 68 and _lib.EXT_EXPORTS == ["mpcrl_ext_version", "mpcrl_state_sens"]
    assert _lib.CHAIN_EXT_EXPORTS == ["mpcrl_chain_ext_version", "mpcrl_chain_policy_state_sens"]
    assert _lib.TRAJ_EXT_EXPORTS == ["mpcrl_traj_ext_version", "mpcrl_traj_vjp"]
    assert _lib.CHAIN_TRAJ_EXT_EXPORTS == ["mpcrl_chain_traj_ext_version", "mpcrl_chain_traj_vjp"]
    others = (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER, _lib.CHAIN_TRAJ_EXT_HEADER)
    for other in others:
        assert "BOUND_EXT_VERSION" not in other.constants and not set(_lib.BOUND_EXT_EXPORTS) & set(other.functions)
    assert _lib.ABI_VERSION == 132 and _lib.EXT_VERSION == 1 and _lib.CHAIN_EXT_VERSION == 1
    assert _lib.TRAJ_EXT_VERSION == 1 and _lib.CHAIN_TRAJ_EXT_VERSION == 1


def test_library_exports_every_symbol_of_the_bound_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.BOUND_EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_bound_ext.h but not exported"
    lib.mpcrl_bound_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_bound_ext_version() == _lib.BOUND_EXT_VERSION


def test_package_exports_the_bound_surface():
    import mpc4rl_amd
    assert mpc4rl_amd.BoxBounds._fields == ("lb0", "ub0", "lb", "ub", "lbe", "ube") and "BoxBounds" in mpc4rl_amd.__all__
    for name in ("bound_vjp", "bound_value_grad", "fold_bound_grad"):
        assert hasattr(mpc4rl_amd.MPCBatch, name)


# ---------------------------------------------------------------------- the fixture
def check_set(g13, generator, k, N, nx, nu, gate):
    nv, nw = nu + nx, N * nu + (N + 1) * nx
    B = len(g13[k + "x0"])
    assert g13[k + "G"].shape == (B, 3, nw) and g13[k + "x0"].shape == (B, nx)
    for name in ("g_lb", "g_ub"):
        assert g13[k + name].shape == (B, 3, N + 1, nv) and np.isfinite(g13[k + name]).all()
    for name in ("dV_dlb", "dV_dub", "act_lb", "act_ub"):
        assert g13[k + name].shape == (B, N + 1, nv)
    assert g13[k + "lb0"].shape == g13[k + "ub0"].shape == (nu,) and g13[k + "lb"].shape == g13[k + "ub"].shape == (nv,)
    assert g13[k + "lbe"].shape == g13[k + "ube"].shape == (nx,)
    unit = np.zeros(nw)
    unit[0] = 1.0
    assert np.all(g13[k + "G"][:, 2] == unit)
    # the exact zeros: no row on the states of stage 0, on the controls of stage N, and where the bound is absent
    for name, side, sign in (("g_lb", "lb", 1.0), ("g_ub", "ub", -1.0)):
        g, dV = g13[k + name], g13[k + "dV_d" + side]
        assert np.all(g[:, :, 0, nu:] == 0) and np.all(g[:, :, N, :nu] == 0) and np.all(dV[:, 0, nu:] == 0) and np.all(dV[:, N, :nu] == 0)
        absent = np.abs(g13[k + side]) >= 1e29
        assert np.all(g[:, :, 1:N, absent] == 0) and np.all(dV[:, 1:N, absent] == 0)
        absent_e = np.abs(g13[k + side + "e"]) >= 1e29
        assert np.all(g[:, :, N, nu:][:, :, absent_e] == 0) and np.all(dV[:, N, nu:][:, absent_e] == 0)
        assert np.all(sign * dV >= 0)      # dV/dlb = lam_l >= 0, dV/dub = -lam_u <= 0
    soft, agree, agree_V = g13[k + "soft"], g13[k + "agree"], g13[k + "agree_V"]
    assert np.all(agree[~soft] <= gate) and np.all(agree_V[~soft] <= gate) and np.all(np.isnan(agree[soft]))
    # an active row is a row with a multiplier; the classes are what the masks say
    act = g13[k + "act_lb"] | g13[k + "act_ub"]
    assert np.array_equal(g13[k + "interior"], ~act.any((1, 2))) and np.array_equal(g13[k + "act_u0"], act[:, 0, :nu].any(1))
    assert np.array_equal(g13[k + "act_u"], act[:, 1:, :nu].any((1, 2)))
    return soft, act


@pytest.mark.parametrize("model,N", SMALL)
def test_fixture_shapes_gate_counts_and_magnitude(g13, generator, model, N):
    nx, nu, n_p = DIMS[model]
    k = f"{model}_N{N}_"
    assert float(g13["gate_small"]) == 1e-7 == generator.GATE["small"] and float(g13["tol"]) == 1e-10
    soft, act = check_set(g13, generator, k, N, nx, nu, 1e-7)
    assert g13[k + "dpi_dp"].shape == (len(soft), nu, n_p)
    assert generator.REQUIRED == {"interior": 2, "act_u": 3, "act_u0": 1} and generator.REQUIRED_X == {"act_x": 1}
    need = {**generator.REQUIRED, **(generator.REQUIRED_X if model == "cartpole" and N >= 15 else {}), **generator.REQUIRED_AT.get((model, N), {})}
    for c, n in need.items():
        assert int((g13[k + c] & ~soft).sum()) >= n, (model, N, c)
    big = max(np.abs(g13[k + "g_lb"][~soft][:, :2]).max(), np.abs(g13[k + "g_ub"][~soft][:, :2]).max())
    assert big >= 0.1, (model, N, big)
    # the bounds of the sets
    if model == "linear":
        assert np.array_equal(g13[k + "lb"], [-0.3, -1.0, -1.0]) and np.array_equal(g13[k + "ub"], [0.3, 1.0, 1.0])
        assert np.all(g13[k + "lbe"] <= -1e29) and np.all(g13[k + "ube"] >= 1e29)
        assert np.all((g13[k + "x0"] >= [0.1, -0.4]) & (g13[k + "x0"] <= [0.9, 0.4]))
    else:
        ub = generator.U_BOUND_AT.get((model, N), 8.0)
        assert (ub == 8.0) == (N != 2)
        assert np.array_equal(g13[k + "ub"], [ub, 0.6, 1.0, 0.4, 1.5]) and np.array_equal(g13[k + "lb"], -g13[k + "ub"])
        assert np.array_equal(g13[k + "ube"], [0.6, 1.0, 0.4, 1.5]) and np.array_equal(g13[k + "lbe"], -g13[k + "ube"])
    assert np.array_equal(g13[k + "lb0"], g13[k + "lb"][:nu]) and np.array_equal(g13[k + "ub0"], g13[k + "ub"][:nu])


@pytest.mark.parametrize("k", list(CHAIN_SETS))
def test_fixture_chain_sets(g13, generator, k):
    n_mass, N = CHAIN_SETS[k]
    nx, nu = (2 * (n_mass - 2) + 1) * 3, 3
    g12 = np.load(os.path.join(GOLD, "g12_chain_traj_vjp.npz"))
    assert float(g13["gate_chain"]) == 1e-6 == generator.GATE["chain"]
    soft, act = check_set(g13, generator, k, N, nx, nu, 1e-6)
    assert not soft.any() and np.array_equal(g13[k + "x0"], g12[k + "x0"])
    assert np.array_equal(g13[k + "lb"][:nu], [-1.0] * 3) and np.array_equal(g13[k + "ub"][:nu], [1.0] * 3)
    assert np.all(np.abs(g13[k + "lb"][nu:]) >= 1e29) and np.all(np.abs(g13[k + "ube"]) >= 1e29)
    have = int(act.any((1, 2)).sum())
    assert have >= {"m3_N10_act_": 4, "m3_N10_x0_": 1, "m5_N8_ss_": 0}[k]
    if have:
        assert max(np.abs(g13[k + "g_lb"][:, :2]).max(), np.abs(g13[k + "g_ub"][:, :2]).max()) >= 0.1


@pytest.mark.parametrize("model,N", SMALL)
def test_unit_cotangent_rows_summed_per_shared_vector_are_the_differences_of_u0(g13, generator, model, N):
    """G = e_{u_0}: the rows of g_lb / g_ub summed over the stages that share a bound vector are d u_0* / d (that bound), which the
    gate's central differences of the port measured directly; the same for dV/db against the differences of V.  Firm instances."""
    k = f"{model}_N{N}_"
    firm = ~g13[k + "soft"]
    vec = generator.shared_vectors(generator.bounded(model, N))
    g = (g13[k + "g_lb"][firm][:, 2], g13[k + "g_ub"][firm][:, 2])
    dV = (g13[k + "dV_dlb"][firm], g13[k + "dV_dub"][firm])
    summed = np.stack([g[side][:, list(stages), cv].sum(1) for _, _, side, stages, cv in vec], 1)
    summed_V = np.stack([dV[side][:, list(stages), cv].sum(1) for _, _, side, stages, cv in vec], 1)
    assert g13[k + "fd_u0"].shape == (len(firm), len(vec), 1)
    assert np.abs(summed - g13[k + "fd_u0"][firm][:, :, 0]).max() <= 1e-7
    assert (np.abs(summed_V - g13[k + "fd_V"][firm]) / np.maximum(np.abs(g13[k + "fd_V"][firm]), 1.0)).max() <= 1e-7
    # the known answer: u_0 on its bound moves with that bound one to one, and not with the other side
    on_lb, on_ub = g13[k + "act_lb"][firm][:, 0, 0], g13[k + "act_ub"][firm][:, 0, 0]
    assert (on_lb | on_ub).any() and not (on_lb & on_ub).any()
    assert np.abs(g[0][on_lb][:, 0, 0] - 1.0).max(initial=0.0) <= 1e-6 and np.abs(g[1][on_ub][:, 0, 0] - 1.0).max(initial=0.0) <= 1e-6
    assert np.abs(g[1][on_lb][:, 0, 0]).max(initial=0.0) <= 1e-6 and np.abs(g[0][on_ub][:, 0, 0]).max(initial=0.0) <= 1e-6


# ---------------------------------------------------------------------- fold_bound_grad
def test_fold_bound_grad_on_a_hand_made_tensor():
    from mpc4rl_amd import MPCBatch
    stub = type("S", (), {"N": 3, "nu": 1, "nx": 2})()
    g = torch.arange(2 * 4 * 3, dtype=torch.float64).reshape(2, 4, 3)      # [B 2, N + 1 = 4, nu + nx = 3]
    u0, stage, term = MPCBatch.fold_bound_grad(stub, g)
    assert u0.tolist() == [[0.0], [12.0]]                                   # the control of stage 0
    assert stage.tolist() == [[3.0 + 6.0, 4.0 + 7.0, 5.0 + 8.0], [15.0 + 18.0, 16.0 + 19.0, 17.0 + 20.0]]      # stages 1 and 2
    assert term.tolist() == [[10.0, 11.0], [22.0, 23.0]]                    # the states of stage 3
    with pytest.raises(ValueError):
        MPCBatch.fold_bound_grad(stub, g[:, :3])


# ---------------------------------------------------------------------- the layer, on a stub batch with CPU tensors
class StubBatch:
    """What the layer touches of an MPCBatch.  x_{k+1} = x_k + 1, u = 1; the VJPs answer with recognisable numbers."""

    class ocp:
        name = "linear"

    def __init__(self, B=2, N=3, nx=2, nu=1, n_p=4):
        self.B, self.N, self.nx, self.nu, self.n_p = B, N, nx, nu, n_p
        self.calls = []

    def set_theta(self, theta):
        self.theta = theta

    def set_bounds(self, which, lb, ub):
        assert isinstance(lb, np.ndarray) and isinstance(ub, np.ndarray)      # host arrays
        self.calls.append(("set_bounds", which, lb.tolist(), ub.tolist()))

    def solve(self, x0, **kw):
        self.x0 = x0
        self.calls.append(("solve", kw))
        f64 = dict(dtype=torch.float64)
        return type("R", (), {"status": torch.tensor([0] * (self.B - 1) + [self.fail], dtype=torch.int32), "u0": torch.ones((self.B, self.nu), **f64),
                              "V": torch.ones(self.B, **f64), "dV_dp": torch.ones((self.B, self.n_p), **f64) if kw.get("sens_v") else None,
                              "dpi_dp": torch.ones((self.B, self.nu, self.n_p), **f64) if kw.get("sens_pi") else None})()

    fail = 0

    def state_sens(self, **kw):
        self.calls.append(("state_sens", kw))
        f64 = dict(dtype=torch.float64)
        return type("S", (), {"dpi_dx0": torch.ones((self.B, self.nu, self.nx), **f64), "dV_dx0": torch.ones((self.B, self.nx), **f64)})()

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

    def bound_vjp(self, gX, gU, x0=True, theta=True, bounds=True):
        self.calls.append(("bound_vjp", gX is not None, gU is not None, x0, theta, bounds))
        one = torch.ones((self.B, self.N + 1, self.nu + self.nx), dtype=torch.float64)
        gx = torch.zeros((self.B, self.nx), dtype=torch.float64) if gX is None else gX.sum(1)
        return ((gx if x0 else None), (torch.ones((self.B, self.n_p), dtype=torch.float64) if theta else None),
                (one if bounds else None), (2.0 * one if bounds else None))

    def fold_bound_grad(self, g):
        from mpc4rl_amd import MPCBatch
        return MPCBatch.fold_bound_grad(self, g)


def box(grad=("lb0", "ub", "lbe"), dtype=torch.float64):
    from mpc4rl_amd import BoxBounds
    v = dict(lb0=[-1.0], ub0=[1.0], lb=[-1.0, -2.0, -3.0], ub=[1.0, 2.0, 3.0], lbe=[-4.0, -5.0], ube=[4.0, 5.0])
    return BoxBounds(**{k: torch.tensor(x, dtype=dtype, requires_grad=k in grad) for k, x in v.items()})


def test_layer_without_bounds_makes_exactly_the_calls_it_made():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub, cold=True)
    x0 = torch.zeros((2, 2), dtype=torch.float64, requires_grad=True)
    theta = torch.ones(4, dtype=torch.float64, requires_grad=True)
    X, U = layer.trajectory(x0, theta)
    X.sum().backward()
    assert stub.calls == [("solve", {"cold": True}), ("vjp", True, False, True, True)]
    stub.calls.clear()
    u0, V = layer(x0, theta)
    (u0.sum() + V.sum()).backward()
    assert stub.calls == [("solve", {"sens_v": True, "sens_pi": True, "cold": True}), ("state_sens", {"q_mode": False, "value": True, "policy": True})]
    stub.calls.clear()
    X, U = layer.trajectory(x0, theta, bounds=None)
    (X.sum() + U.sum()).backward()
    assert stub.calls == [("solve", {"cold": True}), ("vjp", True, True, True, True)]


def test_layer_trajectory_with_bounds_on_a_stub():
    from mpc4rl_amd import MPCLayer, _lib
    stub = StubBatch()
    layer = MPCLayer(stub, cold=True)
    x0 = torch.zeros((2, 2), dtype=torch.float32, requires_grad=True)
    theta = torch.ones(4, dtype=torch.float64, requires_grad=True)
    b = box()
    X, U = layer.trajectory(x0, theta, b)
    assert layer.pass_counter == 1 and X.dtype == torch.float32
    assert stub.calls == [("set_bounds", _lib.BOUNDS_U0, [-1.0], [1.0]), ("set_bounds", _lib.BOUNDS_STAGE, [-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]),
                          ("set_bounds", _lib.BOUNDS_TERMINAL, [-4.0, -5.0], [4.0, 5.0]), ("solve", {"cold": True})]
    (X.sum() + U.sum()).backward()
    assert stub.calls[4:] == [("bound_vjp", True, True, True, True, True)]      # ONE call for everything that requires a gradient
    assert torch.all(x0.grad == 4.0) and torch.all(theta.grad == 2.0)
    # folded and summed over the batch of 2: lb rows are ones, ub rows twos; stages 1 .. N-1 are two stages
    assert b.lb0.grad.tolist() == [2.0] and b.ub.grad.tolist() == [8.0] * 3 and b.lbe.grad.tolist() == [2.0] * 2
    assert b.ub0.grad is None and b.lb.grad is None and b.ube.grad is None      # members that do not require a gradient get none
    # nothing but a bound requires a gradient: only the bound outputs are asked for
    stub.calls.clear()
    b = box(grad=("ube",), dtype=torch.float32)
    X, U = layer.trajectory(x0.detach(), theta.detach(), b)
    U.sum().backward()
    assert stub.calls[-1] == ("bound_vjp", False, True, False, False, True) and b.ube.grad.dtype == torch.float32
    assert b.ube.grad.tolist() == [4.0] * 2
    # no bound requires a gradient: the bound outputs are not asked for
    stub.calls.clear()
    X, U = layer.trajectory(x0, theta.detach(), box(grad=()))
    X.sum().backward()
    assert stub.calls[-1] == ("bound_vjp", True, False, True, False, False)


def test_layer_forward_with_bounds_on_a_stub():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub)
    x0 = torch.zeros((2, 2), dtype=torch.float64, requires_grad=True)
    theta = torch.ones(4, dtype=torch.float64, requires_grad=True)
    b = box(grad=("lb", "ub"))
    u0, V = layer(x0, theta, b)
    assert [c[0] for c in stub.calls] == ["set_bounds"] * 3 + ["solve", "state_sens", "bound_value_grad"]
    (3.0 * u0.sum() + 2.0 * V.sum()).backward()
    assert stub.calls[6:] == [("bound_vjp", False, True, False, False, True)]
    # per instance and stage: lb 1 (vjp) + 2 * 0.5 (value) = 2, ub 2 - 2 * 0.25 = 1.5; two stages, two instances
    assert b.lb.grad.tolist() == [8.0] * 3 and b.ub.grad.tolist() == [6.0] * 3
    assert torch.all(x0.grad == 5.0) and torch.all(theta.grad == 10.0)      # MPCFunction's terms, unchanged
    # the loss reads V alone: no adjoint solve, the multipliers are the whole gradient; a failed instance contributes zero
    stub.calls.clear()
    stub.fail = 4
    b = box(grad=("lb0",))
    u0, V = layer(x0.detach(), theta.detach(), b)
    V.sum().backward()
    assert all(c[0] != "bound_vjp" for c in stub.calls) and b.lb0.grad.tolist() == [0.5]


def test_pass_counter_rule_covers_the_bound_paths():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub)
    x0 = torch.zeros((2, 2), dtype=torch.float64, requires_grad=True)
    theta = torch.ones(4, dtype=torch.float64)
    for first in ("trajectory", "forward"):
        b = box()
        out = layer.trajectory(x0, theta, b) if first == "trajectory" else layer(x0, theta, b)
        seen = layer.pass_counter
        layer.trajectory(x0.detach(), theta)      # another pass: the handle's iterate is no longer this one's
        assert layer.pass_counter == seen + 1
        n = len(stub.calls)
        with pytest.raises(RuntimeError, match="one backward per forward"):
            out[0].sum().backward()
        assert all(c[0] != "bound_vjp" for c in stub.calls[n:])      # refused before the library is asked
