"""The chain's trajectory vector-Jacobian product without a GPU: the fifth header include/mpcrl_chain_traj_ext.h parses into a table
of its own and the library exports it, the other four tables are as they were, the fixture G12 (tests/golden/make_chain_traj_vjp.py)
holds what its generator promises, and MPCTrajectoryFunction picks the chain method by the OCP's name (stub batches, CPU tensors)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G10_SETS = ((3, 1, "ss"), (3, 2, "ss"), (3, 10, "ss"), (3, 10, "x0"), (4, 3, "ss"), (5, 8, "ss"), (6, 3, "ss"), (7, 5, "ss"))
SETS = G10_SETS + ((3, 10, "act"),)
GATE = 1e-6


@pytest.fixture(scope="module")
def g12():
    return np.load(os.path.join(GOLD, "g12_chain_traj_vjp.npz"))


@pytest.fixture(scope="module")
def g10():
    return np.load(os.path.join(GOLD, "g10_chain_state_sens.npz"))


@pytest.fixture(scope="module")
def generator():
    sys.path.insert(0, GOLD)
    try:
        import make_chain_traj_vjp
    finally:
        sys.path.remove(GOLD)
    return make_chain_traj_vjp


def dims(n_mass):
    nx = (2 * (n_mass - 2) + 1) * 3
    return nx, 3, 10 * (n_mass - 1) + nx * nx + 9 + 3 * (n_mass - 2)


# ---------------------------------------------------------------------- the fifth header and the library
def test_chain_traj_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.CHAIN_TRAJ_EXT_EXPORTS == ["mpcrl_chain_traj_ext_version", "mpcrl_chain_traj_vjp"]
    assert _lib.CHAIN_TRAJ_EXT_HEADER.constants["CHAIN_TRAJ_EXT_VERSION"] == _lib.CHAIN_TRAJ_EXT_VERSION == 1
    ret, params = _lib.CHAIN_TRAJ_EXT_HEADER.functions["mpcrl_chain_traj_vjp"]
    assert ret == "int" and params == [("h", "handle"), ("flags", "int"), ("status", "int32*"), ("gX", "double*"), ("gU", "double*"),
                                       ("g_x0", "double*"), ("g_theta", "double*"), ("stream", "void*")]
    assert _lib.CHAIN_TRAJ_EXT_HEADER.functions["mpcrl_chain_traj_ext_version"] == ("int", [])
    assert not _lib.CHAIN_TRAJ_EXT_HEADER.spec_fields
    assert os.path.basename(_lib.CHAIN_TRAJ_EXT_HEADER_PATH) == "mpcrl_chain_traj_ext.h"


def test_the_other_four_tables_are_as_they_were():
    from mpc4rl_amd import _lib
    assert len(_lib.EXPORTS) == 68 and _lib.EXT_EXPORTS == ["mpcrl_ext_version", "mpcrl_state_sens"]
    assert _lib.CHAIN_EXT_EXPORTS == ["mpcrl_chain_ext_version", "mpcrl_chain_policy_state_sens"]
    assert _lib.TRAJ_EXT_EXPORTS == ["mpcrl_traj_ext_version", "mpcrl_traj_vjp"]
    others = set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.CHAIN_EXT_EXPORTS) | set(_lib.TRAJ_EXT_EXPORTS)
    assert not set(_lib.CHAIN_TRAJ_EXT_EXPORTS) & others
    for other in (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER):
        assert "CHAIN_TRAJ_EXT_VERSION" not in other.constants
    assert _lib.ABI_VERSION == 132 and _lib.EXT_VERSION == 1 and _lib.CHAIN_EXT_VERSION == 1 and _lib.TRAJ_EXT_VERSION == 1


def test_library_exports_every_symbol_of_the_chain_traj_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.CHAIN_TRAJ_EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_chain_traj_ext.h but not exported"
    lib.mpcrl_chain_traj_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_chain_traj_ext_version() == _lib.CHAIN_TRAJ_EXT_VERSION


def test_package_exports_the_chain_method():
    import mpc4rl_amd
    assert hasattr(mpc4rl_amd.MPCBatch, "chain_trajectory_vjp") and hasattr(mpc4rl_amd.MPCBatch, "trajectory_vjp")
    assert hasattr(mpc4rl_amd, "MPCTrajectoryFunction") and hasattr(mpc4rl_amd.MPCLayer, "trajectory")


# ---------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_fixture_shapes_and_gate(g12, generator, n_mass, N, base):
    nx, nu, n_p = dims(n_mass)
    k = f"m{n_mass}_N{N}_{base}_"
    nw = N * nu + (N + 1) * nx
    assert g12[k + "x0"].shape == (4, nx) and g12[k + "G"].shape == (4, 3, nw)
    assert g12[k + "g_theta"].shape == (4, 3, n_p) and g12[k + "g_x0"].shape == (4, 3, nx) and g12[k + "active"].shape == (4, N, nu)
    for name in ("x0", "G", "g_theta", "g_x0", "agree", "nb_theta", "nb_x0"):
        assert np.isfinite(g12[k + name]).all()
    unit = np.zeros(nw)
    unit[0] = 1.0
    assert np.all(g12[k + "G"][:, 2] == unit)      # the third cotangent: component 0 of u_0
    assert float(g12["gate"]) == GATE == generator.GATE and float(g12["tol"]) == generator.TOL == 1e-10
    assert np.all(g12[k + "agree"] <= GATE) and np.all(g12[k + "draw"] < generator.DRAWS)
    # the negative control of the GPU test has something to see: the neighbours' rows are at least 10 gates away
    assert g12[k + "nb_theta"].min() >= 10 * GATE and g12[k + "nb_x0"].min() >= 10 * GATE
    # the differences ran over x0 and an entry of every block of p: m, D, L, C, Q, R (and w)
    dp, nl = generator.diff_p(n_mass), n_mass - 1
    assert np.array_equal(g12[f"diff_p_m{n_mass}"], dp)
    edges = [0, nl, 4 * nl, 7 * nl, 10 * nl, 10 * nl + nx * nx, 10 * nl + nx * nx + nu * nu, n_p]
    assert all(((dp >= lo) & (dp < hi)).any() for lo, hi in zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("n_mass,N,base", G10_SETS)
def test_unit_cotangent_rows_are_the_dense_solve_of_g10(g12, g10, n_mass, N, base):
    """G = e_{u_0}: g_theta is row 0 of the mirror's du0*/dp and g_x0 row 0 of its du0*/dx0, on G10's own x0."""
    k = f"m{n_mass}_N{N}_{base}_"
    idx = g12[k + "idx"]
    assert len(idx) == 4 and np.array_equal(g12[k + "x0"], g10[k + "x0"][idx])
    assert np.abs(g12[k + "g_theta"][:, 2] - g10[k + "dpi_dp"][idx][:, 0]).max() <= 1e-12
    assert np.abs(g12[k + "g_x0"][:, 2] - g10[k + "dpi_dx0"][idx][:, 0]).max() <= 1e-12
    assert np.array_equal(g12[k + "active"][:, 0], g10[k + "active"][idx])
    assert not g12[k + "active"][:, 1:].any()      # none of G10's instances has a control row active past stage 0


def test_active_set_has_a_bound_row_inside_the_sweep(g12, generator):
    """m3_N10_act: every instance holds a control row on its bound at a stage >= 1 — where a barrier term meets a non-zero right-hand
    side inside the adjoint sweep; x0 is spread 0.2 around the problem's default start."""
    k = "m3_N10_act_"
    assert generator.ACT_SET == (3, 10, "act") and generator.ACTIVE == 1e-8 and float(g12["sigma_act"]) == generator.SIGMA_ACT == 0.2
    assert np.all(g12[k + "active"][:, 1:].sum((1, 2)) >= 1)


# ---------------------------------------------------------------------- the dispatch, on stub batches with CPU tensors
class StubBatch:
    """What MPCTrajectoryFunction touches of an MPCBatch; each VJP method answers with numbers of its own."""

    def __init__(self, name, B=2, N=3, nx=2, nu=1, n_p=4):
        self.ocp = type("ocp", (), {"name": name})
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

    def _answer(self, which, value, gX, gU, x0, theta):
        self.calls.append((which, gX is not None, gU is not None, x0, theta))
        return (torch.full((self.B, self.nx), value, dtype=torch.float64) if x0 else None,
                torch.full((self.B, self.n_p), value, dtype=torch.float64) if theta else None)

    def trajectory_vjp(self, gX, gU, x0=True, theta=True):
        return self._answer("vjp", 1.0, gX, gU, x0, theta)

    def chain_trajectory_vjp(self, gX, gU, x0=True, theta=True):
        return self._answer("chain_vjp", 3.0, gX, gU, x0, theta)


@pytest.mark.parametrize("name,method,value", [("chain_mass", "chain_vjp", 3.0), ("linear", "vjp", 1.0)])
def test_backward_dispatches_on_the_name_of_the_ocp(name, method, value):
    from mpc4rl_amd import MPCLayer
    stub = StubBatch(name)
    layer = MPCLayer(stub, cold=True)
    x0 = torch.zeros((2, 2), dtype=torch.float32, requires_grad=True)
    theta = torch.ones(4, dtype=torch.float64, requires_grad=True)
    X, U = layer.trajectory(x0, theta)
    assert stub.calls == [("solve", {"cold": True})]      # one plain solve: no sens_v, no sens_pi, on the chain too
    (X.sum() + U.sum()).backward()
    assert stub.calls[1:] == [(method, True, True, True, True)]
    assert torch.all(x0.grad == value) and torch.all(theta.grad == 2 * value)      # shared theta: summed over the batch
    X, U = layer.trajectory(x0.detach(), theta)
    X.sum().backward()
    assert stub.calls[-1] == (method, True, False, False, True)
