"""The trajectory vector-Jacobian product without a GPU: the fourth header include/mpcrl_traj_ext.h parses into a table of its own and
the library exports it, the other three tables are as they were, the fixture G11 (tests/golden/make_traj_vjp.py) holds what its
generator promises, and the pass-counter rule of MPCTrajectoryFunction on a stub batch with CPU tensors."""
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
GATE = 1e-7


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(GOLD, "g11_traj_vjp.npz"))


@pytest.fixture(scope="module")
def g9():
    return np.load(os.path.join(GOLD, "g9_state_sens.npz"))


@pytest.fixture(scope="module")
def generator():
    sys.path.insert(0, GOLD)
    try:
        import make_traj_vjp
    finally:
        sys.path.remove(GOLD)
    return make_traj_vjp


# ---------------------------------------------------------------------- the fourth header and the library
def test_traj_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.TRAJ_EXT_EXPORTS == ["mpcrl_traj_ext_version", "mpcrl_traj_vjp"]
    assert _lib.TRAJ_EXT_HEADER.constants["TRAJ_EXT_VERSION"] == _lib.TRAJ_EXT_VERSION == 1
    ret, params = _lib.TRAJ_EXT_HEADER.functions["mpcrl_traj_vjp"]
    assert ret == "int" and params == [("h", "handle"), ("flags", "int"), ("gX", "double*"), ("gU", "double*"), ("g_x0", "double*"),
                                       ("g_theta", "double*"), ("stream", "void*")]
    assert _lib.TRAJ_EXT_HEADER.functions["mpcrl_traj_ext_version"] == ("int", [])
    assert not _lib.TRAJ_EXT_HEADER.spec_fields
    assert os.path.basename(_lib.TRAJ_EXT_HEADER_PATH) == "mpcrl_traj_ext.h"


def test_the_other_three_tables_are_as_they_were():
    from mpc4rl_amd import _lib
    assert len(_lib.EXPORTS) == 68 and _lib.EXT_EXPORTS == ["mpcrl_ext_version", "mpcrl_state_sens"]
    assert _lib.CHAIN_EXT_EXPORTS == ["mpcrl_chain_ext_version", "mpcrl_chain_policy_state_sens"]
    assert not set(_lib.TRAJ_EXT_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.CHAIN_EXT_EXPORTS))
    for other in (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER):
        assert "TRAJ_EXT_VERSION" not in other.constants
    assert _lib.ABI_VERSION == 132 and _lib.EXT_VERSION == 1 and _lib.CHAIN_EXT_VERSION == 1


def test_library_exports_every_symbol_of_the_traj_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.TRAJ_EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_traj_ext.h but not exported"
    lib.mpcrl_traj_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_traj_ext_version() == _lib.TRAJ_EXT_VERSION


def test_package_exports_the_trajectory_function():
    import mpc4rl_amd
    assert hasattr(mpc4rl_amd, "MPCTrajectoryFunction") and hasattr(mpc4rl_amd.MPCLayer, "trajectory")
    assert hasattr(mpc4rl_amd.MPCBatch, "trajectory_vjp")


# ---------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]])
def test_fixture_shapes_gate_and_class_minimums(g11, g9, generator, model, N):
    nx, nu, n_p = DIMS[model]
    k = f"{model}_N{N}_"
    nw = N * nu + (N + 1) * nx
    idx = g11[k + "idx"]
    B = len(idx)
    assert g11[k + "G"].shape == (B, 3, nw) and g11[k + "g_theta"].shape == (B, 3, n_p) and g11[k + "g_x0"].shape == (B, 3, nx)
    assert np.array_equal(g11[k + "x0"], g9[k + "x0"][idx]) and np.array_equal(g11[k + "cls"], g9[k + "cls"][idx])
    assert np.array_equal(g11[k + "soft"], g9[k + "soft"][idx]) and np.all(np.diff(idx) > 0)
    for name in ("G", "g_theta", "g_x0"):
        assert np.isfinite(g11[k + name]).all()
    # the third cotangent is the unit vector on component 0 of u_0; the cartpole's cost block has no gradient
    unit = np.zeros(nw)
    unit[0] = 1.0
    assert np.all(g11[k + "G"][:, 2] == unit)
    if model == "cartpole":
        assert np.all(g11[k + "g_theta"][:, :, 3:] == 0)
    soft, agree = g11[k + "soft"], g11[k + "agree"]
    assert float(g11["gate"]) == GATE == generator.GATE
    assert np.all(agree[~soft] <= GATE) and np.all(np.isnan(agree[soft]))
    need = {**generator.REQUIRED, **generator.REQUIRED_AT.get((model, N), {})}
    assert generator.REQUIRED == {0: 4, 1: 3}
    for c, n in need.items():
        assert int((g11[k + "cls"] == c).sum()) >= n, (model, N, c)
    assert not (soft & (g11[k + "cls"] == 0)).any()


@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_fixture_per_instance_theta_set(g11, g9, generator, model):
    nx, nu, n_p = DIMS[model]
    k = f"{model}_th_"
    idx = g11[k + "idx"]
    assert len(idx) >= generator.TH_MIN and np.array_equal(g11[k + "theta"], g9[k + "theta"][idx])
    assert np.array_equal(g11[k + "x0"], g9[k + "x0"][idx]) and np.all(g11[k + "agree"] <= GATE)
    assert g11[k + "g_theta"].shape == (len(idx), 3, n_p) and g11[k + "g_x0"].shape == (len(idx), 3, nx)


@pytest.mark.parametrize("model,N", [(m, N) for m in HORIZONS for N in HORIZONS[m]] + [("cartpole", "th"), ("linear", "th")])
def test_unit_cotangent_rows_are_the_dense_solve_of_g9(g11, g9, model, N):
    """G = e_{u_0}: g_theta is row 0 of the mirror's du0*/dp and g_x0 row 0 of its du0*/dx0 — the same dense solve."""
    k = f"{model}_{N}_" if N == "th" else f"{model}_N{N}_"
    idx = g11[k + "idx"]
    ref_x = g9[k + ("dpi_dx0_mirror" if N != "th" else "dpi_dx0")][idx][:, 0]
    assert np.abs(g11[k + "g_theta"][:, 2] - g9[k + "dpi_dp"][idx][:, 0]).max() <= 1e-12
    assert np.abs(g11[k + "g_x0"][:, 2] - ref_x).max() <= 1e-12


# ---------------------------------------------------------------------- the pass counter, on a stub batch with CPU tensors
class StubBatch:
    """What MPCTrajectoryFunction touches of an MPCBatch: x_{k+1} = x_k + theta_0 u, u = 1, so X, U are known in closed form and
    trajectory_vjp answers with recognisable numbers."""

    class ocp:
        name = "linear"

    def __init__(self, B=2, N=3, nx=2, nu=1, n_p=4):
        self.B, self.N, self.nx, self.nu, self.n_p = B, N, nx, nu, n_p
        self.calls = []

    def set_theta(self, theta):
        self.theta = theta

    def solve(self, x0, **kw):
        self.x0 = x0
        self.calls.append(("solve", kw))
        return type("R", (), {"status": torch.zeros(self.B, dtype=torch.int32)})()

    def get_iterate(self):
        X = self.x0[:, None, :] + torch.arange(self.N + 1, dtype=torch.float64)[None, :, None]
        return X, torch.ones((self.B, self.N, self.nu), dtype=torch.float64), None, None, None

    def trajectory_vjp(self, gX, gU, x0=True, theta=True):
        self.calls.append(("vjp", gX is not None, gU is not None, x0, theta))
        gx = torch.zeros((self.B, self.nx), dtype=torch.float64) if gX is None else gX.sum(1)
        return (gx if x0 else None), (torch.ones((self.B, self.n_p), dtype=torch.float64) if theta else None)


def test_pass_counter_rule_of_the_trajectory_function():
    from mpc4rl_amd import MPCLayer
    stub = StubBatch()
    layer = MPCLayer(stub, cold=True)
    assert layer.pass_counter == 0
    x0 = torch.zeros((2, 2), dtype=torch.float32, requires_grad=True)
    theta = torch.ones(4, dtype=torch.float64, requires_grad=True)
    X, U = layer.trajectory(x0, theta)
    assert layer.pass_counter == 1 and X.shape == (2, 4, 2) and U.shape == (2, 3, 1) and X.dtype == torch.float32
    assert stub.calls == [("solve", {"cold": True})]      # one plain solve: no sens_v, no sens_pi
    X.sum().backward()                                    # g_U never arrives: None means NULL
    assert stub.calls[-1] == ("vjp", True, False, True, True)
    assert x0.grad.dtype == torch.float32 and torch.all(x0.grad == 4.0)              # N + 1 stages of ones
    assert theta.grad.shape == (4,) and torch.all(theta.grad == 2.0)                # shared theta: summed over the batch
    # per-instance theta keeps its rows; x0 without a gradient is not asked for
    theta_b = torch.ones((2, 4), dtype=torch.float64, requires_grad=True)
    X, U = layer.trajectory(x0.detach(), theta_b)
    (X.sum() + U.sum()).backward()
    assert stub.calls[-1] == ("vjp", True, True, False, True) and theta_b.grad.shape == (2, 4) and torch.all(theta_b.grad == 1.0)
    # every forward, q and trajectory of the layer moves the counter: a backward pass that finds another value raises
    for other in ("forward", "q", "trajectory"):
        X, U = layer.trajectory(x0, theta)
        seen = layer.pass_counter
        if other == "trajectory":
            layer.trajectory(x0.detach(), theta.detach())
        else:      # (the stub cannot run them: the counter moves before the function is applied)
            with pytest.raises(Exception):
                layer(x0.detach(), theta.detach()) if other == "forward" else layer.q(x0.detach(), x0.detach(), theta.detach())
        assert layer.pass_counter == seen + 1
        n = len(stub.calls)
        with pytest.raises(RuntimeError, match="one backward per forward"):
            X.sum().backward()
        assert all(c[0] != "vjp" for c in stub.calls[n:])      # refused before the library is asked
