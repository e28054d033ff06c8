"""The reference the dynamics-jet probe is measured against (tests/model_jet_cases.py), checked on the CPU: the 50-digit second-order
forward mode against numerical differentiation of the plain RK4 map, the closed-form Jacobian columns the kernels rely on
(CartpoleDev::lin_trivial), the float64 yardstick's own error, and the fixed list of evaluation points."""
import re
import os

import mpmath
import numpy as np
import pytest
from mpmath import mp, mpf

import model_jet_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_probe_is_declared_and_bound():
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    assert "mpcrl_debug_model_jets" in hdr and "mpcrl_debug_model_jets" in _lib.EXPORTS
    assert int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 132    # additions do not bump it


def _rel(a, b):
    """max |a - b| over the block relative to its largest |b| (mpmath numbers)"""
    scale = max(abs(v) for v in b)
    worst = max(abs(x - y) for x, y in zip(a, b))
    return worst / scale if scale else worst


@pytest.mark.parametrize("name,point", [("cartpole", 1), ("cartpole", 30), ("cartpole_2step", 45), ("linear", 40)])
def test_reference_against_numerical_differentiation(name, point):
    """mpmath.diff (central differences at raised working precision) of the plain map, every first and second partial derivative over
    (u, x, theta), against the forward-mode class: 1e-25 of each block's largest entry.  Blocks: per output, the gradient and the
    Hessian."""
    assert mp.dps == 50
    cs = S.case_set(name)
    z = S._z(cs, point)
    n = len(z)
    F = S.reference(name)["jets"][point]
    plain = S.plain_map_mp(cs.model, z, cs.h, cs.rk_steps)
    for m in range(cs.dims.nx):
        f = lambda *a: S.plain_map_mp(cs.model, a, cs.h, cs.rk_steps)[m]
        assert abs(plain[m] - F[m].v) <= mpf(10) ** -45 * max(1, abs(plain[m]))
        grad = [mpmath.diff(f, tuple(z), tuple(int(k == i) for k in range(n))) for i in range(n)]
        assert _rel(F[m].g, grad) < mpf(10) ** -25, (name, point, m, "gradient")
        pairs = [(i, j) for i in range(n) for j in range(i + 1)]
        hess = [mpmath.diff(f, tuple(z), tuple(int(k == i) + int(k == j) for k in range(n))) for i, j in pairs]
        assert _rel([F[m].hess(i, j) for i, j in pairs], hess) < mpf(10) ** -25, (name, point, m, "hessian")


@pytest.mark.parametrize("name", ["cartpole", "cartpole_2step"])
def test_closed_form_columns_hold_in_the_reference(name):
    """dF/dx_0 = e_0 and dF/dx_1 = [T, 1, 0, 0]' with T = h rk_steps at every cartpole point, to 45 digits: what lin_trivial fills in"""
    cs = S.case_set(name)
    T = mpf(cs.h) * cs.rk_steps
    tol = mpf(10) ** -45
    for F in S.reference(name)["jets"]:
        for m in range(4):
            assert abs(F[m].g[1] - (1 if m == 0 else 0)) <= tol
            assert abs(F[m].g[2] - (T if m == 0 else 1 if m == 1 else 0)) <= tol
            for j in range(8):      # and so the second derivatives along x_0, x_1 vanish
                assert abs(F[m].hess(1, j)) <= tol and abs(F[m].hess(2, j)) <= tol


@pytest.mark.parametrize("name", S.CASE_SETS)
def test_yardstick_is_usable_as_a_bound(name):
    ref, yard = S.reference(name), S.yardstick(name)
    for b in yard:
        err, _ = S.block_errors(yard[b], ref[b])
        print(f"{name} {b}: yardstick error max {err.max():.3e} at point {err.argmax()}")
        assert err.max() < 1e-11, (name, b, int(err.argmax()))


def test_block_errors_floor_and_zero_blocks():
    hi, lo = np.array([[1.0, 2.0], [0.0, 0.0]]), np.zeros((2, 2))
    err, _ = S.block_errors(np.array([[1.0, 2.0 + 2.0 ** -51], [0.0, 1e-200]]), (hi, lo))
    assert err[0] == 2.0 ** -52 and err[1] > 1e90       # the floor of an all-zero point is 2 x 1e-300
    err, _ = S.block_errors(np.array([[0.0, 1e-300]]), (np.zeros((1, 2)), np.zeros((1, 2))))
    assert np.isinf(err[0])
    err, _ = S.block_errors(np.zeros((1, 2)), (np.zeros((1, 2)), np.zeros((1, 2))))
    assert err[0] == 0.0
    # the low word counts: a device value equal to hi is off by lo
    err, _ = S.block_errors(np.array([[1.0]]), (np.array([[1.0]]), np.array([[1e-20]])))
    assert err[0] == 1e-20


def test_case_list_is_fixed():
    for name in S.CASE_SETS:
        cs = S.case_set(name)
        assert cs.n == 67 and cs.x.shape == (67, cs.dims.nx) and cs.u.shape == (67, 1) and cs.th.shape == (67, cs.dims.ntd)
        assert cs.nu.shape == (67, cs.dims.nx) and cs.y.shape == (67, cs.dims.nx + 1)
    x, u, th = S.cartpole_points()
    x2, u2, th2 = S.cartpole_points()
    assert np.array_equal(x, x2) and np.array_equal(u, u2) and np.array_equal(th, th2)
    assert all(np.array_equal(a, b) for a, b in zip(S.linear_points(), S.linear_points()))
    pi = float(np.pi)
    angles = [0.0, pi / 2, pi, 2 * pi, 7 * pi, -7 * pi, 25 * pi, -25 * pi]
    for a in angles + [a + 1e-8 for a in angles] + [a - 1e-8 for a in angles]:
        assert a in x[:, 2], a
    assert np.sum((x[:, 2] > 0.9 * pi) & (x[:, 2] < 1.1 * pi)) >= 10 + 3        # the reset range (and pi, pi +- 1e-8)
    for r in (0.0, 15.0, -15.0):
        assert r in x[:, 3]
    assert np.abs(x[:, 3]).max() == 15.0
    for c in (0.0, 30.0, -30.0):
        assert c in u[:, 0]
    assert np.abs(u).max() == 30.0
    for t in ((1.0, 0.1, 0.5), (1.5, 0.15, 0.75), (0.5, 0.05, 0.25), (1.0, 0.01, 0.5), (1.0, 0.1, 0.1)):
        assert any(np.array_equal(row, np.array(t)) for row in th), t
    assert not x[0].any() and not u[0].any()                                     # the origin
    assert (S.case_set("cartpole").h, S.case_set("cartpole").rk_steps) == (0.025, 1)
    assert (S.case_set("cartpole_2step").h, S.case_set("cartpole_2step").rk_steps) == (0.05, 2)
    # linear system: the parameters of linear_system_ocp() and random ones; order 1 and order 1e3
    from mpc4rl_amd import linear_system_ocp
    xl, ul, thl = S.linear_points()
    assert np.array_equal(thl[0], linear_system_ocp().p0[:8]) and np.array_equal(thl[0], np.array(S.LINEAR_REFERENCE_THETA))
    assert np.sum((thl == thl[0]).all(axis=1)) == 34
    assert np.abs(xl[0::2]).max() < 10 and np.abs(xl[1::2]).max() > 1e3 and np.abs(ul[1::2]).max() > 1e3
    # reciprocal inputs
    r = S.rcp_inputs()
    assert r.size == 4096 and np.array_equal(r, S.rcp_inputs())
    m, e = np.frexp(r)
    assert e.min() == -19 and e.max() == 21 and (r > 0).any() and (r < 0).any()      # frexp: mantissa in [0.5, 1)
    for k in range(-20, 21):
        assert 2.0 ** k in r and -(2.0 ** k) in r


def test_rcp_ulp_measure():
    x = np.array([3.0, 4.0, -3.0])
    exact = np.array([1.0 / 3.0, 0.25, -1.0 / 3.0])
    assert S.rcp_ulp_errors(x, exact).max() <= 0.5
    off = np.nextafter(exact, np.inf)
    e = S.rcp_ulp_errors(x, off)
    assert 0.5 <= e[0] <= 1.5 and e[1] == 1.0 and 0.5 <= e[2] <= 1.5
