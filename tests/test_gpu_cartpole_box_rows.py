"""The cartpole solve kernels with the full-box bound pattern compiled in (csrc/small_kernel.hpp, BOX; chosen by launch_small from the
handle's bounds, reported by mpcrl_query_box_rows) against the generic kernels (a handle created under MPCRL_GENERIC_ROWS=1) and against
the C++ CPU port.

Shapes: N = 12, 20, 31, 32 (four, three, two and one instance per wavefront; the short reduction tree up to N = 31, the full one at
N = 32), 7 and 13 instances (partial wavefronts), the plain and the time-sliced launch (illegal at N = 31: the request falls back to the
plain kernel).  Per shape: a cold solve with sensitivities, a warm call from its iterate, a Q-mode call from that one; at N = 20 also a
call with a per-instance cold mask.  Inputs and references: tests/small_mode_cases.py (the port solves every instance on its own, so
one reference per horizon serves both batch sizes).

Asserted: the BOX handle and the generic handle are torch.equal on every output and on the stored iterate (x, u, pi, bnd, res);
statuses, SQP and interior-point iteration counts equal the port's; values inside RTOL = 1e-6 of small_mode_cases.compare.

Active rows (tests/cartpole_box_cases.py, checked on the port by tests/test_cartpole_box_rows_cpu.py): control bounds tightened to +-9
through set_bounds on stage 0 and the interior stages alike, starts with the cart 0.2 m from an end of its track and moving towards
it — the force row (coordinate 0) and the cart-position row (coordinate 1) are active at the solutions.

Fallback: bounds outside the pattern (an absent interior bound; terminal bounds that differ from the interior ones; bounds of u_0 that
differ from the interior control bounds) make the query 0 and the results the port's; the original bounds make it 1 again and return the
first call's bits.  mpcrl_create needs a device, so the host predicate is tested here and not in a CPU test.

Measured on an MI355X (largest error): 4.1e-14 over the sixteen shapes' cold, warm, Q-mode and cold-mask calls, every iteration count
equal; 4.0e-8 with an absent interior bound (the generic kernels); active rows 7.3e-11, every count equal."""
import dataclasses

import numpy as np
import pytest
import torch

import cartpole_box_cases as BC
import small_mode_cases as C
from small_mode_cases import bit_equal, compare, outputs, raw_solve

pytestmark = pytest.mark.gpu

HORIZONS = (12, 20, 31, 32)
BATCHES = (7, 13)
MODES = (-1, 1)               # set_launch_mode: plain, time-sliced where legal
SLICING_ILLEGAL = (31,)
PORT_FIELDS = ("u0", "V", "dV", "dpi", "X", "U", "PI", "BND", "status", "sqp_iter", "ipm_iter")


def rows(ref, B):
    """The first B instances of a port result, as the dict small_mode_cases.compare takes."""
    return {f: np.asarray(getattr(ref, f))[:B] for f in PORT_FIELDS}


def flags(cold):
    from mpc4rl_amd import _lib
    return _lib.SENS_V | _lib.SENS_PI | (_lib.COLD if cold else 0)


def handle(monkeypatch, ocp, N, B, mode, generic):
    from mpc4rl_amd import MPCBatch
    if generic:
        monkeypatch.setenv("MPCRL_GENERIC_ROWS", "1")
    else:
        monkeypatch.delenv("MPCRL_GENERIC_ROWS", raising=False)
    mpc = MPCBatch(ocp, B)
    monkeypatch.delenv("MPCRL_GENERIC_ROWS", raising=False)
    mpc.set_launch_mode(mode)
    assert mpc.lib.mpcrl_query_box_rows(mpc._h) == (0 if generic else 1)
    expect = 1 if (mode == 1 and N not in SLICING_ILLEGAL) else 0
    assert mpc.lib.mpcrl_query_time_sliced(mpc._h, flags(True), mpc._stream()) == expect
    return mpc


def pair(monkeypatch, ocp, N, B, mode):
    return handle(monkeypatch, ocp, N, B, mode, False), handle(monkeypatch, ocp, N, B, mode, True)


def same_counts(got, ref, what):
    print(f"[box rows] {what}: status {got['status'].tolist()} sqp {got['iters'][:, 0].tolist()} / port {ref['sqp_iter'].tolist()} "
          f"ipm {got['iters'][:, 1].tolist()} / port {ref['ipm_iter'].tolist()}")
    assert np.array_equal(got["status"], ref["status"]), what
    assert np.array_equal(got["iters"][:, 0], ref["sqp_iter"]), what
    assert np.array_equal(got["iters"][:, 1], ref["ipm_iter"]), what


def same_bits(box, rb, gen, rg):
    """The two handles bit for bit: what the calls returned and what they left behind."""
    bit_equal(rb, rg)
    for name, t1, t2 in zip(("x", "u", "pi", "bnd", "res"), box.get_iterate(), gen.get_iterate()):
        assert torch.equal(t1, t2), name
    assert torch.equal(box.get_lagrangian(), gen.get_lagrangian())


def both(box, gen, x0, u0=None, cold=True):
    rb, rg = raw_solve(box, x0, u0, flags=flags(cold)), raw_solve(gen, x0, u0, flags=flags(cold))
    same_bits(box, rb, gen, rg)
    return rb, outputs(box, rb)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", HORIZONS)
def test_box_rows_equal_generic_rows_and_the_port(oracle_port, monkeypatch, N, B, mode):
    c, w = C.case(oracle_port, "cartpole", N), C.warm_case(oracle_port, "cartpole", N)
    what = f"cartpole N {N} B {B} mode {mode:+d}"
    box, gen = pair(monkeypatch, c.ocp, N, B, mode)
    # cold V mode with sensitivities
    ref = rows(c.ref_v, B)
    assert np.all(ref["status"] == 0)
    _, got = both(box, gen, c.x0[:B])
    same_counts(got, ref, what + " cold V")
    compare(got, ref, False, tag=what + ": cold V", suite="box rows")
    # warm V mode from that iterate
    ref = rows(w.ref_w, B)
    _, got = both(box, gen, w.x1[:B], cold=False)
    same_counts(got, ref, what + " warm V")
    compare(got, ref, False, tag=what + ": warm V", suite="box rows")
    # warm Q mode from that one: u_0 pinned (no control rows on stage 0), du0*/dp exact zeros over the NaN fill
    ref = rows(w.ref_wq, B)
    rq, got = both(box, gen, w.x1[:B], c.u0[:B], cold=False)
    same_counts(got, ref, what + " warm Q")
    assert bool((rq.dpi_dp == 0.0).all())
    compare(got, ref, False, fields=("u0",) + C.Q_FIELDS, tag=what + ": warm Q", suite="box rows")
    if N == 20:
        # a per-instance cold mask on a V-mode call from the Q-mode iterate: masked instances as the port's cold solve at x1, the others
        # as its warm one
        mask = torch.arange(B, device="cuda") % 3 == 0
        kw = dict(sens_v=True, sens_pi=True, reorder=False, cold_mask=mask)
        rb, rg = box.solve(w.x1[:B], **kw), gen.solve(w.x1[:B], **kw)
        same_bits(box, rb, gen, rg)
        got = outputs(box, rb)
        m = mask.cpu().numpy()
        for sel, r, name in ((m, rows(w.ref_cold, B), "masked (cold)"), (~m, rows(w.ref_wv, B), "unmasked (warm)")):
            same_counts({k: got[k][sel] for k in ("status", "iters")}, {k: v[sel] for k, v in r.items()}, f"{what} cold mask, {name}")
            err = C.largest_error(got, r, rows=sel)
            C.report(f"{what}: cold mask, {name}", err, suite="box rows")
            assert err < C.RTOL


@pytest.mark.parametrize("mode", MODES)
def test_active_control_and_state_rows(oracle_port, monkeypatch, mode):
    """Rows active at the solution (tests/cartpole_box_cases.py): the force row (coordinate 0 of v = [u; x]) on +-9 on the first stages,
    the cart-position row (coordinate 1) on +-2.4 on later ones; N = 20, 13 instances.

    The batch is drawn so that the port's iteration counts do not move over starts one unit in the last place apart
    (cartpole_box_cases.ACTIVE_SEED): statuses, SQP and interior-point counts are asserted equal to the port's, as in every other case."""
    from mpc4rl_amd import _lib
    a = BC.active_case(oracle_port)
    N, B, nu = BC.ACTIVE_N, BC.ACTIVE_B, a.ocp.nu
    box, gen = pair(monkeypatch, a.ocp, N, B, mode)
    for mpc, expect in ((box, 1), (gen, 0)):
        mpc.set_bounds(_lib.BOUNDS_U0, a.lb[:nu], a.ub[:nu])
        mpc.set_bounds(_lib.BOUNDS_STAGE, a.lb, a.ub)
        assert mpc.lib.mpcrl_query_box_rows(mpc._h) == expect      # still the full-box pattern
    ref = rows(a.ref, B)
    assert np.all(ref["status"] == 0)
    _, got = both(box, gen, a.x0)
    what = f"cartpole N {N} B {B} mode {mode:+d} active rows"
    same_counts(got, ref, what)
    compare(got, ref, False, tag=what, suite="box rows")
    for bnd in (got["BND"], ref["BND"]):
        control, state = BC.active_rows(bnd, N, nu)
        assert (control > C.ACTIVE).sum() >= B // 2 and (state > BC.STATE_ACTIVE).sum() >= B // 2, (control, state)
    assert np.abs(got["U"]).max() <= BC.ACTIVE_U + 1e-9 and np.abs(got["X"][:, :, 0]).max() <= BC.TRACK + 1e-9


def test_bounds_outside_the_pattern_run_the_generic_kernels(oracle_port, monkeypatch):
    from mpc4rl_amd import _lib
    N, B = 20, C.CP_B
    c, b = C.case(oracle_port, "cartpole", N), C.bounds_case(oracle_port, "cartpole", N)
    nu = c.ocp.nu
    orig = C.original_bounds(c.ocp)
    mpc = handle(monkeypatch, c.ocp, N, B, 1, False)
    query = lambda: mpc.lib.mpcrl_query_box_rows(mpc._h)

    def set_all(lb0, ub0, lb, ub, lbe, ube):
        mpc.set_bounds(_lib.BOUNDS_U0, lb0, ub0)
        mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
        mpc.set_bounds(_lib.BOUNDS_TERMINAL, lbe, ube)

    def snap(r):
        return r, mpc.get_iterate(), mpc.get_lagrangian()

    first = snap(raw_solve(mpc, c.x0))
    same_counts(outputs(mpc, first[0]), rows(c.ref_v, B), "fallback: original bounds")
    # an interior bound absent (the cart velocity has no upper bound on the stages and at the terminal stage)
    set_all(b.lb0, b.ub0, b.lb, b.ub, b.lbe, b.ube)
    assert query() == 0
    got = outputs(mpc, raw_solve(mpc, c.x0))
    same_counts(got, rows(b.ref, B), "fallback: absent interior bound")
    compare(got, rows(b.ref, B), False, tag="cartpole N 20: absent interior bound", suite="box rows")
    set_all(*orig)
    assert query() == 1
    # every bound present, the terminal ones tighter than the interior ones
    lbe, ube = 0.75 * orig[4], 0.75 * orig[5]
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, lbe, ube)
    assert query() == 0
    P = dataclasses.replace(c.P, lbx_e=lbe.copy(), ubx_e=ube.copy())
    ref = rows(oracle_port.solve(P, c.x0), B)
    got = outputs(mpc, raw_solve(mpc, c.x0))
    same_counts(got, ref, "fallback: terminal bounds differ")
    compare(got, ref, False, tag="cartpole N 20: terminal bounds differ", suite="box rows")
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, orig[4], orig[5])
    assert query() == 1
    # the bounds of u_0 differ from the interior control bounds
    mpc.set_bounds(_lib.BOUNDS_U0, 0.5 * orig[0], 0.5 * orig[1])
    assert query() == 0
    mpc.set_bounds(_lib.BOUNDS_U0, orig[0], orig[1])
    assert query() == 1
    # a refused call changes nothing
    with pytest.raises(RuntimeError, match="mpcrl_set_bounds failed"):
        mpc.set_bounds(_lib.BOUNDS_TERMINAL, orig[5], orig[4])
    assert query() == 1
    # the original bounds again: the BOX kernels, and the first call's bits
    again = snap(raw_solve(mpc, c.x0))
    bit_equal(first[0], again[0])
    for name, t1, t2 in zip(("x", "u", "pi", "bnd", "res"), first[1], again[1]):
        assert torch.equal(t1, t2), name
    assert torch.equal(first[2], again[2])


def test_generic_rows_switch_and_other_models(monkeypatch):
    """The query is 0 for a model without BOX kernels whatever its bounds are, and for a cartpole handle created under MPCRL_GENERIC_ROWS=1
    even after set_bounds re-evaluates the pattern."""
    from mpc4rl_amd import MPCBatch, _lib, linear_system_ocp
    lin = MPCBatch(linear_system_ocp(N=8), 5)
    assert lin.lib.mpcrl_query_box_rows(lin._h) == 0
    ocp = C.problem("cartpole", 20)[0]
    gen = handle(monkeypatch, ocp, 20, 5, -1, True)
    orig = C.original_bounds(ocp)
    gen.set_bounds(_lib.BOUNDS_STAGE, orig[2], orig[3])
    assert gen.lib.mpcrl_query_box_rows(gen._h) == 0
    assert gen.lib.mpcrl_query_box_rows(None) < 0
