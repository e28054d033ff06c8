"""The cartpole and linear-system kernels (small_solve_kernel, small_solve_sliced_kernel, small_sens_kernel, lq_solve_kernel<3, 8>,
<3, 16>, <4, 16>) at every horizon where their lane layout or their kernel changes, in the modes the chain kernels are held to in
tests/test_gpu_chain_modes.py: cold V and Q mode, full-SQP warm starts, bounds / discount factor / tolerance / iteration cap set after
creation, and a NaN instance among its wavefront's neighbours.

Reference: the C++ CPU port (oracle/cpu) on the inputs of tests/small_mode_cases.py, whose docstring states the lane layouts and the
comparison rule (statuses equal, SQP iteration counts within one, 1e-6 on every output and on the stored iterate; the looser bars of
test_linear_kernel_three_stages_per_lane_vs_one for at most one instance of an lq_solve_kernel case that stopped one interior-point
iteration apart from the port).  torch.equal wherever two device calls run the same instructions on the same data: the two launch
shapes of the cartpole solve (set_launch_mode -1 / 1), a batch and its reverse, a call before and after a refused or undone setter, the
neighbours of a NaN instance.  tests/test_small_modes_cpu.py holds the port to the conditions that keep these tests from passing
vacuously (statuses, active rows, an effect of every setter above the comparison bar).

Measured on an MI355X (largest error per family; no instance needed the looser bar): cold V 1.4e-13 / 9.3e-10 (cartpole / linear), cold Q
6.1e-15 / 5.9e-10; warm V 1.7e-13 / 1.6e-11, warm V -> Q 5.7e-15 / 5.2e-12, warm Q -> V 1.1e-13 / 5.8e-7, 4.1e-7, 3.8e-9, 2.5e-9 at linear
N = 7, 8, 24, 48; bounds 3.7e-7 / 1.3e-9; a stored iterate without multipliers against a cold solve 6.4e-7 (u0); tol = 1e-9: 1.8e-14 /
1.1e-11, residuals up to 8.3e-10 / 6.0e-10.

The warm V-mode call after a warm Q-mode call FOUND a fault of the port: after a warm call it handed on, for the rows the call did not
have (the bounds of u_0 in Q mode), the multipliers its warm start held, where the kernels store the cold iterate's lam = 0, t = 1.  The
next V-mode call then started its interior point elsewhere on the two sides (35 against 20 interior-point iterations on one instance at
linear N = 48) and stopped 3.1e-6 (X) from the kernel's answer, both 1e-5 from the solution along a weakly active row; cartpole 7.8e-8.
The port now stores the cold values for such rows (oracle/cpu/mpc_oracle.cpp), and the counts are equal on every instance."""
import os

import numpy as np
import pytest
import torch

import launch_plan_cases as P
import small_mode_cases as C
from small_mode_cases import RTOL, bit_equal, compare, outputs, raw_solve, same_bits, same_statuses, snapshot

pytestmark = pytest.mark.gpu

CARTPOLE_MODES = (-1, 1)      # set_launch_mode: plain, time-sliced where legal
SLICING_ILLEGAL = (31, 63)    # launch_plan.hpp, candidate: no spare lane beside the resident slots (2 x 32 and 1 x 64 lanes)


def shapes(model, horizons):
    """(model, N, launch mode) of every case: both launch shapes for cartpole, the library's own choice (None) for the linear system."""
    return [(model, N, m) for N in horizons for m in (CARTPOLE_MODES if model == "cartpole" else (None,))]


def handle(c, mode, ocp=None):
    from mpc4rl_amd import MPCBatch
    mpc = MPCBatch(c.ocp if ocp is None else ocp, c.B)
    if mode is not None:
        mpc.set_launch_mode(mode)
    return mpc


def sens_flags(cold):
    from mpc4rl_amd import _lib
    return _lib.SENS_V | _lib.SENS_PI | (_lib.COLD if cold else 0)


def tag(c, mode, what):
    return f"{c.model} N {c.N}{'' if mode is None else ' mode %+d' % mode}: {what}"


def q_mode_checks(c, r, got, ref, what, mode, cold):
    """A Q-mode call: du0*/dp is exact zeros over the NaN fill, the rest as the port's.  u0_out is the iterate's u_0: from the cold
    start (u = 0) the pinned value bit for bit; from a stored iterate the stored u_0 plus the steps to the pin, i.e. the pinned value
    to rounding, compared like every other output (as test_warm_between_v_and_q_mode of the chain does)."""
    same_statuses(got, ref)
    pinned = torch.as_tensor(c.u0, device=r.u0.device)
    if cold:
        assert torch.equal(r.u0, pinned)
    else:
        assert float((r.u0 - pinned).abs().max()) <= 4 * 2.0 ** -52 * float(pinned.abs().max())
    assert bool((r.dpi_dp == 0.0).all())
    compare(got, ref, c.lq, fields=("u0",) + C.Q_FIELDS, tag=tag(c, mode, what))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. horizons, cold, V mode and Q mode
# ---------------------------------------------------------------------------------------------------------------------------------
def horizon_case(c, mode):
    """Cold V-mode and Q-mode calls on fresh handles against the port, and the reversed batch bit for bit.  Returns both snapshots."""
    snaps = []
    for u0, ref in ((None, c.ref_v), (c.u0, c.ref_q)):
        mpc = handle(c, mode)
        if c.model == "cartpole":      # the launch shape this call takes (read off the launch plan's rule, not found out by running)
            expect = 1 if (mode == 1 and c.N not in SLICING_ILLEGAL) else 0
            assert mpc.lib.mpcrl_query_time_sliced(mpc._h, sens_flags(True), mpc._stream()) == expect
        r = raw_solve(mpc, c.x0, u0)
        got = outputs(mpc, r)
        if u0 is None:
            same_statuses(got, ref)
            compare(got, ref, c.lq, tag=tag(c, mode, "cold V"))
        else:
            q_mode_checks(c, r, got, ref, "cold Q", mode, cold=True)
            assert abs(got["V"][0] - c.ref_v.V[0]) < RTOL * max(1.0, abs(c.ref_v.V[0]))      # row 0 is pinned at its own u0*
        snaps.append(snapshot(mpc, r))
        rev = handle(c, mode)
        rr = raw_solve(rev, c.x0[::-1].copy(), None if u0 is None else u0[::-1].copy())
        same_bits(snaps[-1], snapshot(rev, rr), reverse=True)
    return snaps


@pytest.mark.parametrize("N", C.CP_N)
def test_cartpole_horizons(oracle_port, N):
    c = C.case(oracle_port, "cartpole", N)
    plain, sliced = horizon_case(c, -1), horizon_case(c, 1)
    for a, b in zip(plain, sliced):      # the time-sliced launch (its fallback at N = 31, 63) is bit for bit the plain one
        same_bits(a, b)


@pytest.mark.parametrize("N", C.LIN_N)
def test_linear_horizons(oracle_port, N):
    horizon_case(C.case(oracle_port, "linear", N), None)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. warm full SQP against the port
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,mode", shapes("cartpole", C.CP_WARM_N) + shapes("linear", C.LIN_WARM_N))
def test_warm_full_sqp_vs_port(oracle_port, model, N, mode):
    """Cold at x0; a full SQP from the stored iterate at x1 = x0 + N(0, 0.02); a Q-mode call from that iterate; a V-mode call after it:
    each against the port warm-started from its own previous result.  Then a stored iterate without multipliers."""
    c, w = C.case(oracle_port, model, N), C.warm_case(oracle_port, model, N)
    mpc = handle(c, mode)
    r0 = mpc.solve(c.x0, cold=True)
    same_statuses(outputs(mpc, r0), c.ref_v)
    r1 = raw_solve(mpc, w.x1, flags=sens_flags(False))
    got = outputs(mpc, r1)
    same_statuses(got, w.ref_w)
    compare(got, w.ref_w, c.lq, tag=tag(c, mode, "warm V"))
    x, u, pi = [t.clone() for t in mpc.get_iterate()[:3]]
    rq = raw_solve(mpc, w.x1, c.u0, flags=sens_flags(False))
    q_mode_checks(c, rq, outputs(mpc, rq), w.ref_wq, "warm V -> Q", mode, cold=False)
    rv = raw_solve(mpc, w.x1, flags=sens_flags(False))
    got = outputs(mpc, rv)
    same_statuses(got, w.ref_wv)
    compare(got, w.ref_wv, c.lq, tag=tag(c, mode, "warm Q -> V"))
    # x, u, pi of the solution without bound multipliers (MPCRL_COLD_DUAL): the same solution as a cold solve, and not a cold solve
    p = handle(c, mode)
    p.set_iterate(x, u, pi)
    assert not p.duals_valid
    rp = raw_solve(p, w.x1, flags=sens_flags(False))
    assert bool((rp.status == 0).all())
    have = {"u0": rp.u0.cpu().numpy(), "V": rp.V.cpu().numpy()}
    compare(have, w.ref_cold, False, fields=("u0", "V"), tag=tag(c, mode, "set_iterate without multipliers against cold"))
    if model == "cartpole":
        assert float(rp.iters[:, 0].double().mean()) < float(w.ref_cold.sqp_iter.mean()), (rp.iters[:, 0], w.ref_cold.sqp_iter)


@pytest.mark.parametrize("N", [N for N in C.LIN_WARM_N if C.uses_lq_kernel("linear", N)])
def test_linear_cold_mask(oracle_port, N):
    """mpcrl_set_cold_mask in lq_solve_kernel (test_per_instance_cold_mask: cartpole N = 20): masked instances are bit for bit those of
    a cold call, the others bit for bit those of a plain warm call."""
    c, w = C.case(oracle_port, "linear", N), C.warm_case(oracle_port, "linear", N)
    mask = torch.arange(c.B, device="cuda") % 3 == 0
    kw = dict(sens_v=True, sens_pi=True, reorder=False)
    a = handle(c, None)
    a.solve(c.x0, cold=True, reorder=False)
    ra = a.solve(w.x1, cold_mask=mask, **kw)
    cold = handle(c, None).solve(w.x1, cold=True, **kw)
    warm = handle(c, None)
    warm.solve(c.x0, cold=True, reorder=False)
    rw = warm.solve(w.x1, **kw)
    assert bool((ra.status == 0).all())
    bit_equal(ra, cold, mask)
    bit_equal(ra, rw, ~mask)
    assert not torch.equal(cold.iters[:, 1], rw.iters[:, 1])      # a warm call is not a cold call: the mask has something to select


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. bounds after creation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,mode", shapes("cartpole", C.CP_BOUNDS_N) + shapes("linear", C.LIN_BOUNDS_N))
def test_bounds_after_creation(oracle_port, model, N, mode):
    """mpcrl_set_bounds on a small-model handle: control rows, a one-sided state row on the stages and at the terminal stage (the
    bounds of small_mode_cases.bounds_case), against the port on a problem that has them from the start; refused calls change nothing;
    BOUNDS_U0 reaches stage 0 only; the original bounds return the original bits."""
    from mpc4rl_amd import _lib
    c, b = C.case(oracle_port, model, N), C.bounds_case(oracle_port, model, N)
    nu, B = c.ocp.nu, c.B
    orig = C.original_bounds(c.ocp)

    def set_all(lb0, ub0, lb, ub, lbe, ube):
        mpc.set_bounds(_lib.BOUNDS_U0, lb0, ub0)
        mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
        mpc.set_bounds(_lib.BOUNDS_TERMINAL, lbe, ube)

    mpc = handle(c, mode)
    first = snapshot(mpc, raw_solve(mpc, c.x0))
    same_statuses(outputs(mpc, first[0]), c.ref_v)
    # the new bounds against the port
    set_all(b.lb0, b.ub0, b.lb, b.ub, b.lbe, b.ube)
    r = raw_solve(mpc, c.x0)
    got = outputs(mpc, r)
    same_statuses(got, b.ref)
    compare(got, b.ref, c.lq, tag=tag(c, mode, "bounds after creation"))
    for bnd in (got["BND"], b.ref.BND):
        control, stage, terminal = C.active_rows(bnd, N, nu)
        if model == "cartpole":
            assert (stage | terminal).sum() >= B / 4, (stage, terminal)
        else:
            assert control.sum() > B / 4 and stage.sum() >= 1, (control, stage)
            assert N not in (7, 8) or terminal.all(), terminal
    assert np.abs(got["U"]).max() <= float(b.ub0[0]) + 1e-9
    assert got["X"][:, 1:N, 1].min() > b.lb[nu + 1] - 1e-7 and got["X"][:, N, 1].min() > b.lbe[1] - 1e-7
    bounded = snapshot(mpc, r)
    # refused calls: lb > ub, and a soft row made one-sided
    lb, ub = b.lb.copy(), b.ub.copy()
    lb[0], ub[0] = 1.0, -1.0
    with pytest.raises(RuntimeError, match="mpcrl_set_bounds failed"):
        mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
    if model == "linear":
        lb, ub = b.lb.copy(), b.ub.copy()
        ub[nu + 0] = 1e30
        with pytest.raises(RuntimeError, match="mpcrl_set_bounds failed"):
            mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
    same_bits(snapshot(mpc, raw_solve(mpc, c.x0)), bounded)
    # BOUNDS_U0 alone, below the free solution's largest later control: stage 0 obeys it, a later stage does not
    set_all(*orig)
    mpc.set_bounds(_lib.BOUNDS_U0, np.full(nu, -b.b0), np.full(nu, b.b0))
    r = raw_solve(mpc, c.x0)
    U = mpc.get_iterate()[1]
    assert bool((r.status == 0).all())
    assert float(r.u0.abs().max()) <= b.b0 + 1e-9 and float(U[:, 0].abs().max()) <= b.b0 + 1e-9
    assert float(U[:, 1:].abs().max()) > b.b0 + 1e-3
    # the original bounds again: the same request as the first one
    set_all(*orig)
    same_bits(snapshot(mpc, raw_solve(mpc, c.x0)), first)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. discount factor, tolerance, iteration cap after creation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.LIN_GAMMA_N)
def test_linear_discount_factor_after_creation(oracle_port, N):
    c = C.case(oracle_port, "linear", N)
    a = handle(c, None)
    a.set_discount_factor(0.9)
    ra = raw_solve(a, c.x0)
    created = handle(c, None, ocp=C.problem("linear", N, gamma=0.9)[0])
    same_bits(snapshot(a, ra), snapshot(created, raw_solve(created, c.x0)))
    ref = oracle_port.solve(c.P, c.x0, gamma=0.9)
    got = outputs(a, ra)
    same_statuses(got, ref)
    compare(got, ref, c.lq, tag=tag(c, None, "set_discount_factor(0.9)"))
    rel = np.abs(got["V"] - c.ref_v.V) / np.abs(c.ref_v.V)
    assert rel.min() > 0.01, rel      # (the port: about 0.2)


@pytest.mark.parametrize("mode", CARTPOLE_MODES)
def test_cartpole_discount_factor_is_not_used(oracle_port, mode):
    """The NLS cost has no discount: mpcrl_set_gamma changes no bit."""
    c = C.case(oracle_port, "cartpole", 16)
    a, b = handle(c, mode), handle(c, mode)
    b.set_discount_factor(0.5)
    same_bits(snapshot(a, raw_solve(a, c.x0)), snapshot(b, raw_solve(b, c.x0)))


@pytest.mark.parametrize("model,N,mode", shapes("cartpole", (C.CP_TOL_N,)) + shapes("linear", (C.LIN_TOL_N,)))
def test_tolerance_after_creation(oracle_port, model, N, mode):
    c = C.case(oracle_port, model, N)
    mpc = handle(c, mode)
    mpc.set_options(tol=1e-9)
    r = raw_solve(mpc, c.x0)
    ref = oracle_port.solve(c.P, c.x0, tol=1e-9)
    got = outputs(mpc, r)
    same_statuses(got, ref)
    res = mpc.get_iterate()[4]
    print(f"[small modes] {tag(c, mode, 'tol 1e-9')}: residuals up to {float(res.max()):.3e}")
    assert float(res.max()) < 1e-9
    compare(got, ref, c.lq, tag=tag(c, mode, "set_options(tol=1e-9)"))


@pytest.mark.parametrize("model,N,mode", shapes("cartpole", C.CP_MAXITER_N))
def test_iteration_cap_after_creation(oracle_port, model, N, mode):
    """Status 2 at max_iter = 2: the iterate two full steps from the cold start, as the port's (test_status_max_iter of the chain)."""
    c = C.case(oracle_port, model, N)
    mpc = handle(c, mode)
    mpc.set_options(max_iter=2)
    r = raw_solve(mpc, c.x0)
    ref = oracle_port.solve(c.P, c.x0, max_iter=2)
    assert np.all(ref.status == 2) and np.all(ref.sqp_iter == 2)
    assert bool((r.status == 2).all()) and bool((r.iters[:, 0] == 2).all())
    compare(outputs(mpc, r), ref, False, fields=("X", "U", "PI"), tag=tag(c, mode, "set_options(max_iter=2)"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a NaN instance leaves its wavefront's neighbours alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,mode", shapes("cartpole", C.CP_NAN_N) + shapes("linear", C.LIN_NAN_N))
def test_nan_instance_leaves_its_neighbours_alone(oracle_port, model, N, mode):
    c = C.case(oracle_port, model, N)
    clean = handle(c, mode)
    rc = raw_solve(clean, c.x0)
    same_statuses(outputs(clean, rc), c.ref_v)
    x0 = c.x0.copy()
    x0[1] = np.nan
    mpc = handle(c, mode)
    r = raw_solve(mpc, x0)
    assert r.status.tolist() == [0, 1] + [0] * (c.B - 2)
    assert bool((r.dV_dp[1] == 0.0).all()) and bool((r.dpi_dp[1] == 0.0).all())
    others = torch.arange(c.B, device="cuda") != 1
    same_bits(snapshot(mpc, r), snapshot(clean, rc), rows=others, lagrangian=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the query, the launch plan and the launch are one decision
# ---------------------------------------------------------------------------------------------------------------------------------
QUERY_B = 8
QUERY_SLICED = {("cartpole", 20): 1, ("cartpole", 31): 0, ("cartpole", 40): 1, ("linear", 7): 0, ("linear", 8): 0}      # in mode 1; mode -1: never


@pytest.mark.parametrize("model,N", sorted(QUERY_SLICED))
def test_query_is_the_plan_and_the_launch(model, N):
    """mpcrl_query_time_sliced of a handle = `family == SLICED` of mpcrl_debug_launch_plan (and of its restatement) for the handle's
    numbers, outside a stream capture and inside one, where the query adds nothing to the graph; the solve after the query returns the
    bits of the other launch mode's.  Cartpole with the parked instance in LDS (N = 20), without a spare lane (31), on the full tree
    (40); the linear system either side of its kernel change; cold and warm calls."""
    from mpc4rl_amd import MPCBatch, _lib
    ocp = C.problem(model, N)[0]
    x0, _, step = C.inputs(model)
    points = {True: x0[:QUERY_B], False: x0[:QUERY_B] + step[:QUERY_B]}
    n_simd = 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    spl = 1 if os.environ.get("MPCRL_LINEAR_SPL", "").startswith("1") else 3
    side, marker = torch.cuda.Stream(), torch.zeros(1, device="cuda")
    snaps = {}
    for mode in CARTPOLE_MODES:
        mpc = MPCBatch(ocp, QUERY_B)
        mpc.set_launch_mode(mode)
        for cold in (True, False):
            flags = sens_flags(cold)
            args = (N, QUERY_B, n_simd, flags, mode, mpc.lib.mpcrl_query_box_rows(mpc._h), spl, P.TUNE_SLICED)
            out = (_lib.C.c_int32 * 12)()
            assert mpc.lib.mpcrl_debug_launch_plan(P.MODELS[model]["id"], *args, out) == 0
            assert list(out) == P.expected(model, *args)
            want = int(out[0] == P.SLICED)
            assert want == (QUERY_SLICED[model, N] if mode == 1 else 0)
            assert mpc.lib.mpcrl_query_time_sliced(mpc._h, flags, mpc._stream()) == want
            # inside a capture: the same answer, and a graph that holds the marker's increment alone — replaying it leaves the handle as it was
            before = [t.clone() for t in mpc.get_iterate()]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                captured = mpc.lib.mpcrl_query_time_sliced(mpc._h, flags, mpc._stream())
                marker.add_(1.0)
            assert captured == want
            count = float(marker)
            g.replay()
            torch.cuda.synchronize()
            assert float(marker) == count + 1.0
            assert all(torch.equal(a, b) for a, b in zip(before, mpc.get_iterate()))
            r = raw_solve(mpc, points[cold], flags=flags)
            assert bool((r.status == 0).all())
            snaps[mode, cold] = snapshot(mpc, r)
    for cold in (True, False):
        same_bits(snaps[-1, cold], snaps[1, cold])
    assert not torch.equal(snaps[1, True][0].V, snaps[1, False][0].V)      # the warm call was another problem than the cold one
