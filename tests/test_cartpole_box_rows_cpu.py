"""Keeps tests/test_gpu_cartpole_box_rows.py from passing vacuously: on the C++ CPU port the batch of tests/cartpole_box_cases.py
converges on every instance and has active rows of both kinds — the control row (the force at +-9) and a state row (the cart
position at +-2.4) — and its iteration counts do not move under perturbations of the starts at the precision of a double."""
import numpy as np

import cartpole_box_cases as BC
import small_mode_cases as C


def test_active_case_converges_with_a_control_row_and_a_state_row_active(oracle_port):
    a = BC.active_case(oracle_port)
    ref = a.ref
    assert np.all(ref.status == 0), ref.status
    control, state = BC.active_rows(ref.BND, BC.ACTIVE_N, a.ocp.nu)
    print("[box rows] control multipliers", np.round(control, 4).tolist(), "cart-position multipliers", np.round(state, 3).tolist())
    assert (control > C.ACTIVE).sum() >= BC.ACTIVE_B // 2, control
    assert (state > BC.STATE_ACTIVE).sum() >= BC.ACTIVE_B // 2, state
    assert ((control > C.ACTIVE) & (state > BC.STATE_ACTIVE)).any()      # both kinds in one instance
    # on the bound, not just near it
    assert np.abs(ref.U).max() > BC.ACTIVE_U - 1e-6 and np.abs(ref.U).max() <= BC.ACTIVE_U + 1e-9
    assert np.abs(ref.X[:, :, 0]).max() > BC.TRACK - 1e-6 and np.abs(ref.X[:, :, 0]).max() <= BC.TRACK + 1e-9
    # the tightened bounds are still the full-box pattern: u_0's bounds are the interior control bounds
    assert np.all(np.isfinite(a.lb)) and np.all(np.abs(a.lb) < 1e29) and np.all(np.abs(a.ub) < 1e29)


def test_port_counts_do_not_move_over_starts_one_unit_in_the_last_place_apart(oracle_port):
    """The port on x0 and on its ten one-ulp neighbours (cartpole_box_cases.port_counts): every run converges and every instance keeps
    its SQP count and its interior-point count — the counts the GPU test asserts exactly are numbers the reference determines."""
    status, sqp, ipm = BC.port_counts(oracle_port)
    assert status.shape == (11, BC.ACTIVE_B) and np.all(status == 0)
    print("[box rows] port counts over one-ulp neighbours: sqp", sqp[0].tolist(), "ipm", ipm[0].tolist())
    assert np.all(sqp == sqp[0]) and np.all(ipm == ipm[0]), (sqp.max(0) - sqp.min(0), ipm.max(0) - ipm.min(0))
