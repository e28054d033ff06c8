"""State sensitivities without a GPU: the fixture G9 (tests/golden/make_state_sens.py) holds what its generator promises, the second
header include/mpcrl_ext.h parses into a table of its own and the library exports it, and the backward contraction of the autograd
layer (mpc4rl_amd/autograd.py mpc_backward_terms) equals torch.autograd on a differentiable stand-in."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g9_state_sens.npz")
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
BATCH = {"cartpole": 13, "linear": 25}
GATE = 1e-7


@pytest.fixture(scope="module")
def g9():
    return np.load(GOLD)


def scaled(a, b):
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    return float((np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)).max())


# ---------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_fixture_classes_counts_and_agreements(g9, model):
    nx = 4 if model == "cartpole" else 2
    for N in HORIZONS[model]:
        k = f"{model}_N{N}_"
        cls, soft, B = g9[k + "cls"], g9[k + "soft"], BATCH[model]
        assert g9[k + "x0"].shape == (B, nx) and g9[k + "dpi_dx0"].shape == (B, 1, nx) and g9[k + "dV_dx0"].shape == (B, nx)
        assert (cls == 0).sum() >= 4 and (cls == 1).sum() >= 3 and (cls == 2).sum() >= 1, (model, N, np.bincount(cls))
        assert not soft[cls == 0].any()
        du, dV = g9[k + "agree_du"], g9[k + "agree_dV"]
        # compared with the differences wherever the mirror is not the definition (positive slack) or the zero (u_0 on its bound)
        assert np.array_equal(np.isnan(dV), soft) and np.array_equal(np.isnan(du), soft | (cls == 2))
        assert np.nanmax(dV) <= GATE and np.nanmax(du) <= GATE
        assert np.all(g9[k + "dpi_dx0"][cls == 2] == 0.0)
        assert np.isfinite(g9[k + "dpi_dx0"]).all() and np.isfinite(g9[k + "dV_dx0"]).all()
    q = f"{model}_q_"
    assert g9[q + "x0"].shape == (BATCH[model], nx) and g9[q + "dQ_du0"].shape == (BATCH[model], 1)
    for name in ("agree_dV", "agree_dQ"):
        assert np.nanmax(g9[q + name]) <= GATE
    th = f"{model}_th_"
    assert g9[th + "theta"].shape[0] == 3 and np.nanmax(g9[th + "agree_du"]) <= GATE and np.nanmax(g9[th + "agree_dV"]) <= GATE
    from oracle.problems import make_cartpole, make_linear_system
    p0 = (make_cartpole() if model == "cartpole" else make_linear_system()).p0
    dev = np.abs(g9[th + "theta"] - p0)
    assert np.all(dev <= 0.05 * np.abs(p0) + 1e-15) and np.all(dev.max(1) > 0)      # +-5 % of p0, per instance


@pytest.mark.parametrize("model", ["cartpole", "linear"])
def test_envelope_identity(g9, model):
    """Q(x0, u0*) = V(x0) and dQ/du0 = 0 there, so dQ/dx0 at u0 = u0* equals dV/dx0: rows 0..3 of the Q-mode set pin the u0* of
    interior instances of the V-mode set at N = 20 (``vrow``).  Both sides passed the 1e-7 gate against differences: that is the bar."""
    v, q = f"{model}_N20_", f"{model}_q_"
    vrow = g9[q + "vrow"]
    assert np.all(vrow[:4] >= 0) and np.all(vrow[4:] == -1) and np.all(g9[v + "cls"][vrow[:4]] == 0)
    assert np.array_equal(g9[q + "x0"][:4], g9[v + "x0"][vrow[:4]]) and np.array_equal(g9[q + "u0fix"][:4], g9[v + "u0"][vrow[:4]])
    assert scaled(g9[q + "dV_dx0"][:4], g9[v + "dV_dx0"][vrow[:4]]) <= GATE
    assert scaled(g9[q + "V"][:4, None], g9[v + "V"][vrow[:4], None]) <= GATE
    assert np.abs(g9[q + "dQ_du0"][:4]).max() <= GATE * np.maximum(np.abs(g9[v + "dV_dx0"][vrow[:4]]).max(), 1.0)


# ---------------------------------------------------------------------- the second header and the library
def test_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.EXT_EXPORTS == ["mpcrl_ext_version", "mpcrl_state_sens"]
    assert _lib.EXT_HEADER.constants["EXT_VERSION"] == _lib.EXT_VERSION == 1 and _lib.STATE_Q_MODE == 1
    ret, params = _lib.EXT_HEADER.functions["mpcrl_state_sens"]
    assert ret == "int" and params == [("h", "handle"), ("flags", "int"), ("dV_dx0", "double*"), ("dQ_du0", "double*"),
                                       ("dpi_dx0", "double*"), ("stream", "void*")]
    assert _lib.EXT_HEADER.functions["mpcrl_ext_version"] == ("int", [])
    assert not _lib.EXT_HEADER.spec_fields


def test_exports_still_describe_mpcrl_h_alone():
    from mpc4rl_amd import _lib
    assert len(_lib.EXPORTS) == 68 and not set(_lib.EXPORTS) & set(_lib.EXT_EXPORTS)
    assert "EXT_VERSION" not in _lib.HEADER.constants and _lib.ABI_VERSION == 132
    assert os.path.basename(_lib.HEADER_PATH) == "mpcrl.h" and os.path.basename(_lib.EXT_HEADER_PATH) == "mpcrl_ext.h"


def test_library_exports_every_symbol_of_the_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_ext.h but not exported"
    lib.mpcrl_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_ext_version() == _lib.EXT_VERSION


# ---------------------------------------------------------------------- the backward contraction
def stand_in(x0, theta):
    """A smooth (u0 [B, 2], V [B]) of x0 [B, 3] and theta [5] or [B, 5], instance by instance."""
    th = theta if theta.dim() == 2 else theta.expand(x0.shape[0], -1)
    u = torch.stack([torch.tanh(x0[:, 0] * th[:, 0] + x0[:, 1] * th[:, 1]), x0[:, 2] * th[:, 2] ** 2 + torch.sin(th[:, 3])], 1)
    V = 0.5 * (x0 ** 2).sum(1) * th[:, 4] + (u ** 2).sum(1) + x0[:, 0] * th[:, 1]
    return u, V


@pytest.mark.parametrize("shared", [True, False])
def test_backward_terms_equal_autograd(shared):
    from mpc4rl_amd.autograd import mpc_backward_terms
    gen = torch.Generator().manual_seed(3)
    B = 6
    x0 = torch.randn(B, 3, dtype=torch.float64, generator=gen, requires_grad=True)
    theta = torch.randn(*((5,) if shared else (B, 5)), dtype=torch.float64, generator=gen, requires_grad=True)
    g_u = torch.randn(B, 2, dtype=torch.float64, generator=gen)
    g_V = torch.randn(B, dtype=torch.float64, generator=gen)
    status = torch.tensor([0, 2, 0, 1, 0, 4], dtype=torch.int32)
    good = status == 0
    # the Jacobians of every instance, one instance at a time
    J = [torch.autograd.functional.jacobian(lambda a, b: stand_in(a[None], b if shared else b[None]),
                                            (x0[i].detach(), theta.detach() if shared else theta[i].detach())) for i in range(B)]
    du_dx0 = torch.stack([j[0][0][0] for j in J])
    du_dp = torch.stack([j[0][1][0] for j in J])
    dV_dx0 = torch.stack([j[1][0][0] for j in J])
    dV_dp = torch.stack([j[1][1][0] for j in J])
    for t in (du_dx0, du_dp, dV_dx0, dV_dp):      # what an unsolved instance left behind must not matter, NaN included
        t[~good] = float("nan")
    g_x0, g_th = mpc_backward_terms(g_u, g_V, status, du_dx0, dV_dx0, du_dp, dV_dp, shared)
    u, V = stand_in(x0, theta)
    loss = (g_u[good] * u[good]).sum() + (g_V[good] * V[good]).sum()
    want_x0, want_th = torch.autograd.grad(loss, (x0, theta))
    assert g_x0.shape == x0.shape and g_th.shape == theta.shape
    assert torch.allclose(g_x0, want_x0, rtol=1e-12, atol=1e-13) and torch.allclose(g_th, want_th, rtol=1e-12, atol=1e-13)
    assert torch.all(g_x0[~good] == 0.0) and (shared or torch.all(g_th[~good] == 0.0))
    # one side only, and an output the loss does not depend on
    only_x, none_th = mpc_backward_terms(None, g_V, status, du_dx0, dV_dx0, None, None, shared)
    want = torch.autograd.grad((g_V[good] * stand_in(x0, theta)[1][good]).sum(), x0)[0]
    assert none_th is None and torch.allclose(only_x, want, rtol=1e-12, atol=1e-13)
    assert mpc_backward_terms(None, None, status, du_dx0, dV_dx0, du_dp, dV_dp, shared) == (None, None)
