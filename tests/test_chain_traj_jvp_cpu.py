"""The chain's trajectory Jacobian-vector product without a GPU: the header include/mpcrl_chain_traj_jvp_ext.h parses into a table of
its own and the library exports it, the tables of the neighbouring headers are as they were, the fixture G16
(tests/golden/make_chain_traj_jvp.py) holds what its generator promises and is the transpose of G12 (both are the same dense
Jacobians), and ``chain_jacobian_entries`` — what ``MPCBatch.chain_trajectory_jacobian`` resolves its ``entries`` with — agrees with
``chain_param_layout``."""
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
GATE, R = 1e-6, 3


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(GOLD, "g16_chain_traj_jvp.npz"))


@pytest.fixture(scope="module")
def g12():
    return np.load(os.path.join(GOLD, "g12_chain_traj_vjp.npz"))


@pytest.fixture(scope="module")
def generator():
    sys.path.insert(0, GOLD)
    try:
        import make_chain_traj_jvp
    finally:
        sys.path.remove(GOLD)
    return make_chain_traj_jvp


def dims(n_mass):
    nx = (2 * (n_mass - 2) + 1) * 3
    return nx, 3, 10 * (n_mass - 1) + nx * nx + 9 + 3 * (n_mass - 2)


# ---------------------------------------------------------------------- the header and the library
def test_chain_traj_jvp_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.CHAIN_TRAJ_JVP_EXT_EXPORTS == ["mpcrl_chain_traj_jvp_ext_version", "mpcrl_chain_traj_jvp"]
    assert _lib.CHAIN_TRAJ_JVP_EXT_HEADER.constants["CHAIN_TRAJ_JVP_EXT_VERSION"] == _lib.CHAIN_TRAJ_JVP_EXT_VERSION == 1
    ret, params = _lib.CHAIN_TRAJ_JVP_EXT_HEADER.functions["mpcrl_chain_traj_jvp"]
    assert ret == "int" and params == [("h", "handle"), ("flags", "int"), ("status", "int32*"), ("ndir", "int"), ("dx0", "double*"),
                                       ("dtheta", "double*"), ("dX", "double*"), ("dU", "double*"), ("stream", "void*")]
    assert _lib.CHAIN_TRAJ_JVP_EXT_HEADER.functions["mpcrl_chain_traj_jvp_ext_version"] == ("int", [])
    assert not _lib.CHAIN_TRAJ_JVP_EXT_HEADER.spec_fields
    assert os.path.basename(_lib.CHAIN_TRAJ_JVP_EXT_HEADER_PATH) == "mpcrl_chain_traj_jvp_ext.h"


def test_the_neighbouring_tables_are_as_they_were():
    from mpc4rl_amd import _lib
    assert _lib.CHAIN_TRAJ_EXT_EXPORTS == ["mpcrl_chain_traj_ext_version", "mpcrl_chain_traj_vjp"]
    assert _lib.TRAJ_JVP_EXT_EXPORTS == ["mpcrl_traj_jvp_ext_version", "mpcrl_traj_jvp"]
    others = (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER, _lib.CHAIN_TRAJ_EXT_HEADER, _lib.BOUND_EXT_HEADER,
              _lib.COST_EXT_HEADER, _lib.TRAJ_JVP_EXT_HEADER, _lib.PROBE_EXT_HEADER)
    for other in others:
        assert not set(_lib.CHAIN_TRAJ_JVP_EXT_EXPORTS) & set(other.functions)
        assert "CHAIN_TRAJ_JVP_EXT_VERSION" not in other.constants
    assert _lib.CHAIN_TRAJ_EXT_VERSION == 1 and _lib.TRAJ_JVP_EXT_VERSION == 1


def test_library_exports_every_symbol_of_the_chain_traj_jvp_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.CHAIN_TRAJ_JVP_EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_chain_traj_jvp_ext.h but not exported"
    lib.mpcrl_chain_traj_jvp_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_chain_traj_jvp_ext_version() == _lib.CHAIN_TRAJ_JVP_EXT_VERSION


def test_package_exports_the_chain_methods():
    import mpc4rl_amd
    assert hasattr(mpc4rl_amd.MPCBatch, "chain_trajectory_jvp") and hasattr(mpc4rl_amd.MPCBatch, "chain_trajectory_jacobian")
    assert hasattr(mpc4rl_amd.MPCBatch, "trajectory_jvp") and hasattr(mpc4rl_amd.MPCBatch, "trajectory_jacobian")
    assert mpc4rl_amd.ChainTrajectoryJacobian._fields == ("dX_dx0", "dU_dx0", "dX_dtheta", "dU_dtheta", "entries")


# ---------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_fixture_shapes_gate_and_directions(g16, g12, generator, n_mass, N, base):
    nx, nu, n_p = dims(n_mass)
    k = f"m{n_mass}_N{N}_{base}_"
    idx = g16[k + "idx"]
    n = len(idx)
    # all four instances of the eight G10-derived sets, at least three of the four of m3_N10_act; the rows of G12 they are
    assert n == 4 if base != "act" else n >= 3
    assert np.array_equal(idx, np.unique(idx)) and idx.min() >= 0 and idx.max() < 4
    assert np.array_equal(g16[k + "x0"], g12[k + "x0"][idx])
    assert g16[k + "vx"].shape == (n, R, nx) and g16[k + "vp"].shape == (n, R, n_p)
    assert g16[k + "dX"].shape == (n, R, N + 1, nx) and g16[k + "dU"].shape == (n, R, N, nu)
    for name in ("x0", "vx", "vp", "dX", "dU", "agree"):
        assert np.isfinite(g16[k + name]).all()
    assert float(g16["gate"]) == GATE == generator.GATE and float(g16["tol"]) == generator.TOL == 1e-10
    assert np.all(g16[k + "agree"] <= GATE) and np.all(g16[k + "draw"] < generator.DRAWS) and generator.R == R
    # x_0 = x0: row 0 of dX is the direction itself — to the gate in the gate's own scale, not to the bit: the mirror pins x_0 by a
    # pair of bound rows of finite stiffness
    scale = np.maximum(np.abs(g16[k + "dX"]).max((2, 3)), 1.0)
    assert (np.abs(g16[k + "dX"][:, :, 0] - g16[k + "vx"]).max(2) / scale).max() <= GATE
    # direction 0 moves x0 and every entry of p; direction 1 the dynamics block and w only; direction 2 x0 only
    vx, vp = g16[k + "vx"], g16[k + "vp"]
    off_q, off_w = 10 * (n_mass - 1), 10 * (n_mass - 1) + nx * nx + nu * nu
    assert np.all(vx[:, 0] != 0) and np.all(vp[:, 0] != 0)
    assert np.all(vx[:, 1] == 0) and np.all(vp[:, 1, off_q:off_w] == 0) and np.all(vp[:, 1, :off_q] != 0) and np.all(vp[:, 1, off_w:] != 0)
    assert np.all(vx[:, 2] != 0) and np.all(vp[:, 2] == 0)
    # the first draw is the generator's seed rule
    for j, i in enumerate(idx):
        if g16[k + "draw"][j] == 0:
            rng = np.random.default_rng([16000 + 100 * n_mass + N, int(i)])
            assert np.array_equal(rng.standard_normal((R, nx))[0], vx[j, 0])


@pytest.mark.parametrize("n_mass,N,base", SETS)
def test_fixture_is_the_transpose_of_g12(g16, g12, n_mass, N, base):
    """<G, dW> = g_x0 . vx + g_theta . vp with G12's cotangents on the same instances: both fixtures contract the same dense
    Jacobians, so the identity holds to the rounding of two dense solves."""
    k = f"m{n_mass}_N{N}_{base}_"
    idx = g16[k + "idx"]
    nU = N * 3
    worst = 0.0
    for j, i in enumerate(idx):
        dW = np.concatenate([g16[k + "dU"][j].reshape(R, -1), g16[k + "dX"][j].reshape(R, -1)], 1)      # [R, nw], the mirror's order
        assert dW.shape[1] == g12[k + "G"].shape[2] and nU == g16[k + "dU"][j][0].size
        for c in range(3):
            G = g12[k + "G"][i, c]
            for r in range(R):
                lhs = float(G @ dW[r])
                rhs = float(g12[k + "g_x0"][i, c] @ g16[k + "vx"][j, r] + g12[k + "g_theta"][i, c] @ g16[k + "vp"][j, r])
                worst = max(worst, abs(lhs - rhs) / max(float(np.abs(G * dW[r]).sum()), 1.0))
    assert worst <= 1e-9, (k, worst)


# ---------------------------------------------------------------------- entries of the Jacobian
@pytest.mark.parametrize("n_mass", [3, 5, 7])
def test_jacobian_entries_follow_the_parameter_layout(n_mass):
    from mpc4rl_amd.batch import chain_jacobian_entries
    from mpc4rl_amd.problems import chain_param_layout
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    assert n_p == dims(n_mass)[2]
    default = chain_jacobian_entries(n_mass)
    assert default.dtype == np.int64 and np.array_equal(default, np.arange(10 * nl))      # m, D, L, C lead p
    assert np.array_equal(default, chain_jacobian_entries(n_mass, ("m", "D", "L", "C")))
    for name, (lo, hi) in off.items():
        assert np.array_equal(chain_jacobian_entries(n_mass, name), np.arange(lo, hi))
        assert np.array_equal(chain_jacobian_entries(n_mass, (name,)), np.arange(lo, hi))
    got = chain_jacobian_entries(n_mass, ("w", "m"))      # the order given
    assert np.array_equal(got, np.concatenate([np.arange(*off["w"]), np.arange(*off["m"])]))
    for idx in ([0, n_p - 1, 5], np.array([3, 3, 1]), torch.tensor([2, 7])):
        assert np.array_equal(chain_jacobian_entries(n_mass, idx), np.asarray(idx, dtype=np.int64))
    for bad in (("m", "K"), [n_p], [-1], [], np.zeros((2, 2), dtype=int), [0.5]):
        with pytest.raises(ValueError):
            chain_jacobian_entries(n_mass, bad)


class StubBatch:
    """What chain_trajectory_jacobian touches of an MPCBatch: the JVP answers with the directions it was given."""

    def __init__(self, n_mass, B=2, N=2):
        nx, nu, n_p = dims(n_mass)
        self._is_chain, self.B, self.N, self.nx, self.nu, self.n_p, self.device = True, B, N, nx, nu, n_p, torch.device("cpu")

    def chain_trajectory_jvp(self, dx0, dtheta):
        self.dx0, self.dtheta = dx0, dtheta
        R_ = dx0.shape[1]
        col = torch.arange(R_, dtype=torch.float64)
        return (col.reshape(1, R_, 1, 1).expand(self.B, R_, self.N + 1, self.nx).clone(),
                -col.reshape(1, R_, 1, 1).expand(self.B, R_, self.N, self.nu).clone())


def test_jacobian_is_one_call_with_unit_directions_on_a_stub():
    from mpc4rl_amd import MPCBatch
    from mpc4rl_amd.problems import chain_param_layout
    stub = StubBatch(4)
    off = chain_param_layout(4)[4]
    J = MPCBatch.chain_trajectory_jacobian(stub, ("C", "w"))
    want = np.concatenate([np.arange(*off["C"]), np.arange(*off["w"])])
    ne, nx = len(want), stub.nx
    assert J.entries.tolist() == want.tolist()
    assert stub.dx0.shape == (2, nx + ne, nx) and stub.dtheta.shape == (2, nx + ne, stub.n_p)
    assert torch.equal(stub.dx0[0, :nx], torch.eye(nx, dtype=torch.float64)) and torch.all(stub.dx0[:, nx:] == 0)
    assert torch.all(stub.dtheta[:, :nx] == 0) and torch.all(stub.dtheta.sum(2)[:, nx:] == 1)
    assert stub.dtheta[1, nx + torch.arange(ne), torch.as_tensor(want)].tolist() == [1.0] * ne
    # compact blocks: column j is direction nx + j
    assert J.dX_dx0.shape == (2, 3, nx, nx) and J.dU_dx0.shape == (2, 2, 3, nx)
    assert J.dX_dtheta.shape == (2, 3, nx, ne) and J.dU_dtheta.shape == (2, 2, 3, ne)
    assert J.dX_dtheta[0, 0, 0].tolist() == list(range(nx, nx + ne)) and J.dU_dx0[1, 1, 2].tolist() == [-float(c) for c in range(nx)]
    by_index = MPCBatch.chain_trajectory_jacobian(stub, want)
    assert by_index.entries.tolist() == want.tolist() and torch.equal(by_index.dX_dtheta, J.dX_dtheta)
    stub._is_chain = False
    with pytest.raises(RuntimeError, match="chain of masses"):
        MPCBatch.chain_trajectory_jacobian(stub)
