"""The conditions tests/test_gpu_small_modes.py relies on, held on the CPU port alone (no GPU): every case of tests/small_mode_cases.py
converges where the GPU tests say it does, the bounds set after creation are active on enough instances, a warm start is warm, and every
option a GPU test sets changes the port's answer by more than the comparison bar, so that no GPU test can pass vacuously."""
import numpy as np
import pytest

import small_mode_cases as C

CASES = [("cartpole", N) for N in C.CP_N] + [("linear", N) for N in C.LIN_N]
WARM = [("cartpole", N) for N in C.CP_WARM_N] + [("linear", N) for N in C.LIN_WARM_N]
BOUNDS = [("cartpole", N) for N in C.CP_BOUNDS_N] + [("linear", N) for N in C.LIN_BOUNDS_N]


@pytest.mark.parametrize("model,N", CASES)
def test_cold_cases_converge(oracle_port, model, N):
    c = C.case(oracle_port, model, N)
    assert c.B == (C.CP_B if model == "cartpole" else C.LIN_B)
    assert np.all(c.ref_v.status == 0) and np.all(c.ref_q.status == 0)
    for r in (c.ref_v, c.ref_q):
        assert all(np.all(np.isfinite(a)) for a in (r.u0, r.V, r.dV, r.dpi, r.X, r.U, r.PI))
    # row 0 is pinned at its own u0*: Q = V, and the other rows are pinned somewhere else
    assert abs(c.ref_q.V[0] - c.ref_v.V[0]) < 1e-9 * max(1.0, abs(c.ref_v.V[0]))
    assert np.abs(c.u0[1:] - c.ref_v.u0[1:]).min() > 1e-3 and C.largest_error({"V": c.ref_q.V}, c.ref_v, fields=("V",), rows=np.arange(1, c.B)) > C.RTOL
    if model == "linear":
        # no soft-bound slack anywhere: du0*/dp is well defined on every instance (the `strict` filter of test_linear_system_vs_oracle)
        assert np.abs(c.ref_v.BND[:, 4:6]).max() < 1e-9 and np.abs(c.ref_q.BND[:, 4:6]).max() < 1e-9
        assert np.all(c.ref_v.sqp_iter <= 2)
    # the NaN case of the GPU tests: instance 1 alone ends with status 1
    x0 = c.x0.copy()
    x0[1] = np.nan
    assert list(oracle_port.solve(c.P, x0).status) == [0, 1] + [0] * (c.B - 2)


@pytest.mark.parametrize("model,N", WARM)
def test_warm_cases(oracle_port, model, N):
    c, w = C.case(oracle_port, model, N), C.warm_case(oracle_port, model, N)
    for r in (w.ref_w, w.ref_wq, w.ref_wv, w.ref_cold):
        assert np.all(r.status == 0)
    if model == "cartpole":      # a warm start is warm (the linear system converges in one iteration either way)
        assert w.ref_w.sqp_iter.mean() < w.ref_cold.sqp_iter.mean(), (w.ref_w.sqp_iter, w.ref_cold.sqp_iter)
    else:                        # ... but its interior point starts elsewhere: the cold mask of the GPU test has something to select
        print(f"[small modes cpu] linear N {N}: interior-point iterations warm {w.ref_w.ipm_iter}, cold {w.ref_cold.ipm_iter}")
        assert not np.array_equal(w.ref_w.ipm_iter, w.ref_cold.ipm_iter)
    # x1 is another problem than x0, and the Q-mode call another one than the V-mode calls around it
    assert C.largest_error({"V": w.ref_w.V}, c.ref_v, fields=("V",)) > C.RTOL
    assert C.largest_error({"V": w.ref_wq.V}, w.ref_w, fields=("V",)) > C.RTOL
    # a warm and a cold solve end at the same point
    assert C.largest_error({"V": w.ref_w.V, "u0": w.ref_w.u0}, w.ref_cold, fields=("V", "u0")) < C.RTOL
    assert C.largest_error({"V": w.ref_wv.V, "u0": w.ref_wv.u0}, w.ref_cold, fields=("V", "u0")) < C.RTOL


@pytest.mark.parametrize("model,N", BOUNDS)
def test_bounds_cases(oracle_port, model, N):
    c, b = C.case(oracle_port, model, N), C.bounds_case(oracle_port, model, N)
    assert np.all(b.ref.status == 0)
    control, stage, terminal = C.active_rows(b.ref.BND, N, c.ocp.nu)
    print(f"[small modes cpu] {model} N {N}: active control {control.sum()}, stage {stage.sum()}, terminal {terminal.sum()} of {c.B}")
    if model == "cartpole":
        assert (stage | terminal).sum() >= c.B / 4
        assert np.abs(b.ref.U).max() <= C.CP_U_BOUND + 1e-9
        assert np.all(np.isfinite(b.ref.dpi))
    else:
        assert control.sum() > c.B / 4 and stage.sum() >= 1
        if N in (7, 8):
            assert terminal.all()
        assert np.abs(b.ref.BND[:, 4:6]).max() < 1e-9
    assert C.largest_error({"V": b.ref.V}, c.ref_v, fields=("V",)) > C.RTOL
    # the BOUNDS_U0-only call: the level cuts some free u_0 and lies below a later control
    assert (np.abs(c.ref_v.U[:, 0]) > b.b0 + 1e-3).any() and np.abs(c.ref_v.U[:, 1:]).max() > b.b0 + 1e-3


@pytest.mark.parametrize("N", C.LIN_GAMMA_N)
def test_gamma_changes_the_linear_value(oracle_port, N):
    c = C.case(oracle_port, "linear", N)
    r = oracle_port.solve(c.P, c.x0, gamma=0.9)
    assert np.all(r.status == 0)
    rel = np.abs(r.V - c.ref_v.V) / np.abs(c.ref_v.V)
    print(f"[small modes cpu] linear N {N}: V(0.9) against V(0.99), relative difference {rel.min():.3f} .. {rel.max():.3f}")
    assert rel.min() > 0.01


@pytest.mark.parametrize("model,N", [("cartpole", C.CP_TOL_N), ("linear", C.LIN_TOL_N)])
def test_tolerance_is_felt(oracle_port, model, N):
    """At the default tol = 1e-6 some residual stays above 1e-9: a solve that ignored set_options(tol=1e-9) would not get below it."""
    c = C.case(oracle_port, model, N)
    r = oracle_port.solve(c.P, c.x0, tol=1e-9)
    assert np.all(r.status == 0) and r.res.max() < 1e-9
    print(f"[small modes cpu] {model} N {N}: residuals at tol 1e-6 up to {c.ref_v.res.max():.2e}, at 1e-9 up to {r.res.max():.2e}")
    print(f"[small modes cpu] interior-point iterations at tol 1e-6 {c.ref_v.ipm_iter.sum()}, at 1e-9 {r.ipm_iter.sum()}")
    assert c.ref_v.res.max() > 1e-9


@pytest.mark.parametrize("N", C.CP_MAXITER_N)
def test_max_iter_two_is_status_two(oracle_port, N):
    c = C.case(oracle_port, "cartpole", N)
    r = oracle_port.solve(c.P, c.x0, max_iter=2)
    assert np.all(r.status == 2) and np.all(r.sqp_iter == 2)
    assert C.largest_error({"X": r.X}, c.ref_v, fields=("X",)) > C.RTOL
