"""The CPU side of the trajectory JVP (include/mpcrl_traj_jvp_ext.h): the fixture G15 (tests/golden/make_traj_jvp.py) against itself
and against G11, and the binding of the ninth header.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
DIMS = {"cartpole": (4, 1, 83, 3), "linear": (2, 1, 12, 12)}      # nx, nu, np, differentiated entries of p
R = 3


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(GOLD, "g11_traj_vjp.npz"))


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLD, "g15_traj_jvp.npz"))


def keys():
    return [(m, f"{m}_N{N}_", N) for m in HORIZONS for N in HORIZONS[m]] + [(m, f"{m}_th_", 20) for m in HORIZONS]


# ---------------------------------------------------------------------- the fixture
def test_fixture_shapes_and_instances_are_those_of_g11(g11, g15):
    assert float(g15["gate"]) == 1e-7 and float(g15["tol"]) == 1e-10 and float(g15["gamma"]) == float(g11["gamma"])
    for model, key, N in keys():
        nx, nu, n_p, nd = DIMS[model]
        idx = g15[key + "idx"]
        B = len(idx)
        assert B >= 2 and np.all(np.diff(idx) > 0) and idx.max() < len(g11[key + "x0"])
        assert np.array_equal(g15[key + "x0"], g11[key + "x0"][idx])
        assert g15[key + "vx"].shape == (B, R, nx) and g15[key + "vp"].shape == (B, R, n_p)
        assert g15[key + "dX"].shape == (B, R, N + 1, nx) and g15[key + "dU"].shape == (B, R, N, nu)
        assert g15[key + "agree"].shape == (B,)
        assert np.all(g15[key + "vx"][:, 1] == 0) and np.all(g15[key + "vp"][:, 2] == 0)      # theta only, x0 only
        assert np.all(g15[key + "vp"][..., nd:] == 0) and np.all(g15[key + "vp"][:, :2, :nd] != 0) and np.all(g15[key + "vx"][:, ::2] != 0)
        assert np.isfinite(g15[key + "dX"]).all() and np.isfinite(g15[key + "dU"]).all()
        if key.endswith("_th_"):
            assert np.array_equal(g15[key + "theta"], g11[key + "theta"][idx])
        else:
            assert np.array_equal(g15[key + "cls"], g11[key + "cls"][idx]) and np.array_equal(g15[key + "soft"], g11[key + "soft"][idx])


def test_fixture_counts_and_gate(g11, g15):
    """Per (model, N) at least 2 instances of class 0 and 3 of class 1, counted as G11 counts them; none of class 0 at linear N 31,
    32 and 63, where G11 has none; both instances of each per-instance-theta set.  Every compared instance is within the gate, and an
    instance is not compared (agree NaN) exactly where a soft slack is positive."""
    gate = float(g15["gate"])
    compared = 0
    for model, key, N in keys():
        agree = g15[key + "agree"]
        if key.endswith("_th_"):
            assert len(agree) == 2 == len(g11[key + "x0"]) and np.all(agree <= gate)
            compared += 2
            continue
        cls, soft = g15[key + "cls"], g15[key + "soft"]
        assert np.array_equal(np.isnan(agree), soft) and np.all(agree[~soft] <= gate)
        compared += int((~soft).sum())
        need0 = 0 if (model == "linear" and N in (31, 32, 63)) else 2
        assert (cls == 0).sum() >= need0 and (cls == 1).sum() >= 3, (model, N)
        if need0 == 0:
            assert (g11[key + "cls"] == 0).sum() == 0 and (cls == 0).sum() == 0
    assert compared == 96      # of 99: cartpole N 15 row 9 and linear N 20 rows 2, 3 miss the gate (make_traj_jvp.py)
    assert 9 not in g15["cartpole_N15_idx"] and not {2, 3} & set(g15["linear_N20_idx"].tolist())


def test_fixture_stage_zero_row_is_the_direction_in_x0(g15):
    """x_0 = x0, so dX[:, r, 0, :] is vx[r].  The mirror pins x_0 with a pair of bound rows (lbx0 = ubx0 = x0), not by elimination,
    so its row holds vx up to the error of its barrier system; the differences the gate compared it with hold vx exactly (the port's
    x_0 is x0).  The bar is therefore the gate's: gate x max(|dW row|, 1), on the instances the gate compared.  Where a soft slack is
    positive the mirror's row is its own definition (quirk q1 of make_traj_vjp.py) and is not compared.  Measured: at most 1.5e-7
    absolute (cartpole N 31), 0.09 of the bar."""
    gate, worst = float(g15["gate"]), 0.0
    for model, key, N in keys():
        firm = ~g15[key + "soft"] if key + "soft" in g15.files else np.ones(len(g15[key + "idx"]), bool)
        dX, dU, vx = g15[key + "dX"][firm], g15[key + "dU"][firm], g15[key + "vx"][firm]
        if not len(vx):
            continue
        size = np.maximum(np.maximum(np.abs(dX).max((2, 3)), np.abs(dU).max((2, 3))), 1.0)      # [B, R]
        ratio = np.abs(dX[:, :, 0] - vx).max(2) / (gate * size)
        worst = max(worst, float(ratio.max()))
    print(f"stage-0 row against vx: {worst:.2f} of the gate's bar")
    assert worst <= 1.0


def test_unit_cotangent_of_g11_against_the_directions_of_g15(g11, g15):
    """G11's third cotangent is the unit vector on component 0 of u_0, so dU[i, r, 0, 0] = g_x0[i, 2] . vx[r] + g_theta[i, 2] . vp[r]
    with G11's row idx[i]: both sides are products of the same two dense solves.  Measured here: 3.6e-15 relative to
    max(|right-hand side|, 1) over all 14 sets; the bar is ten times that."""
    worst = 0.0
    for model, key, N in keys():
        idx = g15[key + "idx"]
        assert np.all(g11[key + "G"][idx][:, 2, 0] == 1.0) and np.all(g11[key + "G"][idx][:, 2, 1:] == 0.0)
        lhs = g15[key + "dU"][:, :, 0, 0]
        rhs = np.einsum("ij,irj->ir", g11[key + "g_x0"][idx][:, 2], g15[key + "vx"]) \
            + np.einsum("ij,irj->ir", g11[key + "g_theta"][idx][:, 2], g15[key + "vp"])
        worst = max(worst, float((np.abs(lhs - rhs) / np.maximum(np.abs(rhs), 1.0)).max()))
    print(f"G11's unit cotangent against G15's directions: {worst:.1e}")
    assert worst <= 3.6e-14


def test_generator_states_the_recipe():
    sys.path.insert(0, GOLD)
    try:
        import make_traj_jvp as mk
    finally:
        sys.path.remove(GOLD)
    assert (mk.TOL, mk.GATE, mk.R) == (1e-10, 1e-7, 3) and mk.HORIZONS == HORIZONS
    assert mk.REQUIRED == {0: 2, 1: 3} and mk.REQUIRED_AT == {("linear", N): {0: 0} for N in (31, 32, 63)}
    fx = dict(np.load(os.path.join(GOLD, "g15_traj_jvp.npz")))
    assert mk.shortfalls(fx) == []
    fx["cartpole_N15_cls"] = np.where(fx["cartpole_N15_cls"] == 1, 3, fx["cartpole_N15_cls"])
    assert mk.shortfalls(fx) == ["cartpole N 15: 0 of 3 instances of class 1 in the fixture"]


# ---------------------------------------------------------------------- the ninth header and the library
def test_traj_jvp_ext_header_parses_into_its_own_table():
    from mpc4rl_amd import _lib
    assert _lib.TRAJ_JVP_EXT_EXPORTS == ["mpcrl_traj_jvp_ext_version", "mpcrl_traj_jvp"]
    assert _lib.TRAJ_JVP_EXT_HEADER.constants == {"TRAJ_JVP_EXT_VERSION": 1} and _lib.TRAJ_JVP_EXT_VERSION == 1
    f = _lib.TRAJ_JVP_EXT_HEADER.functions
    assert f["mpcrl_traj_jvp_ext_version"] == ("int", [])
    assert f["mpcrl_traj_jvp"] == ("int", [("h", "handle"), ("flags", "int"), ("ndir", "int"), ("dx0", "double*"), ("dtheta", "double*"),
                                           ("dX", "double*"), ("dU", "double*"), ("stream", "void*")])
    assert len(f["mpcrl_traj_jvp"][1]) == 8
    assert not _lib.TRAJ_JVP_EXT_HEADER.spec_fields
    assert os.path.basename(_lib.TRAJ_JVP_EXT_HEADER_PATH) == "mpcrl_traj_jvp_ext.h"
    others = (_lib.HEADER, _lib.EXT_HEADER, _lib.CHAIN_EXT_HEADER, _lib.TRAJ_EXT_HEADER, _lib.CHAIN_TRAJ_EXT_HEADER, _lib.BOUND_EXT_HEADER,
              _lib.COST_EXT_HEADER, _lib.PROBE_EXT_HEADER)
    for other in others:
        assert "TRAJ_JVP_EXT_VERSION" not in other.constants and not set(_lib.TRAJ_JVP_EXT_EXPORTS) & set(other.functions)


def test_library_exports_every_symbol_of_the_traj_jvp_ext_header():
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _lib.TRAJ_JVP_EXT_EXPORTS:
        assert hasattr(lib, s), f"{s} declared in include/mpcrl_traj_jvp_ext.h but not exported"
    lib.mpcrl_traj_jvp_ext_version.restype = ctypes.c_int
    assert lib.mpcrl_traj_jvp_ext_version() == _lib.TRAJ_JVP_EXT_VERSION


def test_package_exports_the_jvp_surface():
    import mpc4rl_amd
    assert mpc4rl_amd.TrajectoryJacobian._fields == ("dX_dx0", "dU_dx0", "dX_dtheta", "dU_dtheta")
    assert "TrajectoryJacobian" in mpc4rl_amd.__all__
    for name in ("trajectory_jvp", "trajectory_jacobian", "n_diff"):
        assert callable(getattr(mpc4rl_amd.MPCBatch, name))
