"""The cartpole kernels on both forms of their segmented reductions (csrc/small_kernel.hpp seg_reduce, chosen per horizon by
launch_small): cold solves + sensitivities at batch sizes that leave partial wavefronts (7 and 13 instances), in both launch shapes, at

    N = 12   13 lanes per instance   four instances per wavefront
    N = 20   21                      the benchmark's layout, three per wavefront
    N = 30   31                      two per wavefront
    N = 31   32                      edge of the short tree (no level at distance 32)
    N = 32   33                      first horizon on the full tree

and one warm call and one Q-mode call at N = 20.  Reference: the C++ CPU port on the inputs of tests/small_mode_cases.py (the first 7
or all 13 of its instances; the port solves every instance on its own, so one reference per horizon serves both batch sizes).
Statuses, SQP and interior-point iteration counts equal the port's; values inside RTOL = 1e-6 of small_mode_cases.compare; the plain and
the time-sliced launch bit for bit (torch.equal) on outputs and stored iterates; dV/dp asked for alone is bit for bit the dV/dp of the
combined request."""
import numpy as np
import pytest
import torch

import small_mode_cases as C
from small_mode_cases import bit_equal, compare, outputs, raw_solve

pytestmark = pytest.mark.gpu

HORIZONS = (12, 20, 30, 31, 32)
BATCHES = (7, 13)
MODES = (-1, 1)               # set_launch_mode: plain, time-sliced where legal
SLICING_ILLEGAL = (31,)       # two 32-lane slots: no spare lane for the parked instance
PORT_FIELDS = ("u0", "V", "dV", "dpi", "X", "U", "PI", "status", "sqp_iter", "ipm_iter")


def rows(ref, B):
    """The first B instances of a port result, as the dict small_mode_cases.compare takes."""
    return {f: np.asarray(getattr(ref, f))[:B] for f in PORT_FIELDS}


def flags(cold, v=True, pi=True):
    from mpc4rl_amd import _lib
    return (_lib.SENS_V if v else 0) | (_lib.SENS_PI if pi else 0) | (_lib.COLD if cold else 0)


def handle(c, B, mode):
    from mpc4rl_amd import MPCBatch
    mpc = MPCBatch(c.ocp, B)
    mpc.set_launch_mode(mode)
    expect = 1 if (mode == 1 and c.N not in SLICING_ILLEGAL) else 0
    assert mpc.lib.mpcrl_query_time_sliced(mpc._h, flags(True), mpc._stream()) == expect
    return mpc


def same_counts(got, ref, what):
    print(f"[reduce paths] {what}: status {got['status'].tolist()} sqp {got['iters'][:, 0].tolist()} / port {ref['sqp_iter'].tolist()} "
          f"ipm {got['iters'][:, 1].tolist()} / port {ref['ipm_iter'].tolist()}")
    assert np.array_equal(got["status"], ref["status"]), what
    assert np.array_equal(got["iters"][:, 0], ref["sqp_iter"]), what
    assert np.array_equal(got["iters"][:, 1], ref["ipm_iter"]), what


def same_iterates(a, b):
    for name, t1, t2 in zip(("x", "u", "pi", "bnd", "res"), a.get_iterate(), b.get_iterate()):
        assert torch.equal(t1, t2), name


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", HORIZONS)
def test_cold_solves_and_sensitivities(oracle_port, N, B):
    c = C.case(oracle_port, "cartpole", N)
    ref = rows(c.ref_v, B)
    assert np.all(ref["status"] == 0)
    done = []
    for mode in MODES:
        mpc = handle(c, B, mode)
        r = raw_solve(mpc, c.x0[:B], flags=flags(True))
        got = outputs(mpc, r)
        same_counts(got, ref, f"N {N} B {B} mode {mode:+d} cold V")
        compare(got, ref, False, tag=f"cartpole N {N} B {B} mode {mode:+d}: cold V", suite="reduce paths")
        done.append((mpc, r))
    (pm, pr), (sm, sr) = done
    bit_equal(pr, sr)
    same_iterates(pm, sm)


@pytest.mark.parametrize("mode", MODES)
def test_warm_and_q_mode_at_the_benchmark_horizon(oracle_port, mode):
    c, w = C.case(oracle_port, "cartpole", 20), C.warm_case(oracle_port, "cartpole", 20)
    mpc = handle(c, c.B, mode)
    r0 = raw_solve(mpc, c.x0, flags=flags(True))
    same_counts(outputs(mpc, r0), rows(c.ref_v, c.B), f"N 20 mode {mode:+d} cold V")
    r1 = raw_solve(mpc, w.x1, flags=flags(False))
    got = outputs(mpc, r1)
    same_counts(got, rows(w.ref_w, c.B), f"N 20 mode {mode:+d} warm V")
    compare(got, rows(w.ref_w, c.B), False, tag=f"cartpole N 20 mode {mode:+d}: warm V", suite="reduce paths")
    q = handle(c, c.B, mode)
    rq = raw_solve(q, c.x0, c.u0, flags=flags(True))
    got = outputs(q, rq)
    same_counts(got, rows(c.ref_q, c.B), f"N 20 mode {mode:+d} cold Q")
    assert torch.equal(rq.u0, torch.as_tensor(c.u0, device=rq.u0.device))
    assert bool((rq.dpi_dp == 0.0).all())      # du0*/dp of a pinned u0: zeros over the NaN fill
    compare(got, rows(c.ref_q, c.B), False, fields=C.Q_FIELDS, tag=f"cartpole N 20 mode {mode:+d}: cold Q", suite="reduce paths")


def test_warm_and_q_mode_plain_equals_time_sliced(oracle_port):
    c, w = C.case(oracle_port, "cartpole", 20), C.warm_case(oracle_port, "cartpole", 20)
    res = []
    for mode in MODES:
        mpc = handle(c, c.B, mode)
        raw_solve(mpc, c.x0, flags=flags(True))
        rw = raw_solve(mpc, w.x1, flags=flags(False))
        q = handle(c, c.B, mode)
        res.append((mpc, rw, q, raw_solve(q, c.x0, c.u0, flags=flags(True))))
    (pm, pw, pq, prq), (sm, sw, sq, srq) = res
    bit_equal(pw, sw)
    same_iterates(pm, sm)
    bit_equal(prq, srq)
    same_iterates(pq, sq)


@pytest.mark.parametrize("B", BATCHES)
def test_dv_alone_is_the_dv_of_the_combined_request(oracle_port, B):
    """dV/dp asked for alone against the dV/dp of the combined request, bit for bit.

    Before this test the two differed by up to 4.441e-16 (one unit in the last place, 22 of 39 entries at B = 13): with du0*/dp the
    pass took dF/dtheta from the first-order part of its second-order jet evaluation of the map, without it from a first-order
    evaluation — the same formulas compiled into different instruction sequences.  A request for dV/dp alone now runs the combined
    request's evaluation with a zero direction and without the adjoint solve (small_kernel.hpp, SmallSolver::sensitivities)."""
    c = C.case(oracle_port, "cartpole", 20)
    both = raw_solve(handle(c, B, 1), c.x0[:B], flags=flags(True))
    alone = raw_solve(handle(c, B, 1), c.x0[:B], flags=flags(True, pi=False))
    d = (alone.dV_dp - both.dV_dp).abs().max().item()
    print(f"[reduce paths] dV/dp alone vs combined, B {B}: largest difference {d:.3e}")
    assert torch.equal(alone.u0, both.u0) and torch.equal(alone.V, both.V)
    assert torch.equal(alone.dV_dp, both.dV_dp)
