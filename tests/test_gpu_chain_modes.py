"""The chain-of-masses kernels in the modes and at the horizons the rest of the suite runs on the small models only: Q mode (u_0
pinned), full-SQP warm starts, bounds changed after creation (a state row among them), the status codes, horizons from N = 1
over the 16-stage batches of the corrector's matrix-core pass, and the two stores of the interior point's bound rows on both sides
of their 128-row switch.

Reference: the C++ CPU port (oracle/cpu) on the same inputs; the autograd mirror of the reference's NLP (oracle/from_iterate.certify)
is the independent leg for the two things the port itself is held to nowhere else, Q mode and a state bound (the same two
certifications run on the port's own iterates in tests/test_oracle.py).  Tolerance: RTOL = 1e-6, every instance's row scaled by
max(|reference row|, 1) — the bar of test_gpu_parity; statuses equal, SQP iteration counts within one, and torch.equal wherever two
device calls run the same instructions on the same data.  No instance is left out of a comparison: every one ends with status 0 on
both sides unless the case is about a status.

Every group runs its comparison once more against a deliberately wrong reference (the port with the pinned u_0 or a bound moved by
1e-3) and requires the same helper to report more than RTOL: the check can fail.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from small_mode_cases import bit_equal, largest_error, outputs, raw_solve, report, same_statuses

pytestmark = pytest.mark.gpu

RTOL = 1e-6
FIELDS = ("u0", "V", "dV", "dpi", "X", "U", "PI")


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU only; computed once per shape and shared)
# ---------------------------------------------------------------------------------------------------------------------------------
def chain_x0(ocp, B, seed):
    """ocp.x0 tiled + N(0, 1e-2) on the 3 M velocity entries.  Returns the generator as well: the pinned u_0 continues its stream."""
    M = (ocp.nx // 3 - 1) // 2
    rng = np.random.default_rng(seed)
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 3 * (M + 1):] += rng.normal(0.0, 1e-2, (B, 3 * M))
    return x0, rng


def pinned_u0(rng, B, u0_star):
    """uniform(-0.9, 0.9); row 0 = that instance's own V-mode u0* (then Q = V), row 1 on the control bounds."""
    u0 = rng.uniform(-0.9, 0.9, (B, 3))
    u0[0] = u0_star[0]
    if B > 1:
        u0[1] = [1.0, -1.0, 0.3]
    return u0


def with_control_bounds(P, b):
    return dataclasses.replace(P, lbu=-b * np.ones(P.nu), ubu=b * np.ones(P.nu))


def with_state_bound(P, ix, lo):
    """A lower bound on state ix at stages 1 .. N and at the terminal stage."""
    one = lambda v, dt=float: np.array([v], dt)
    return dataclasses.replace(P, idxbx=one(ix, int), lbx=one(lo), ubx=one(1e30), idxbx_e=one(ix, int), lbx_e=one(lo), ubx_e=one(1e30))


def state_bound_level(ocp, ref_free, ix):
    """Halfway between the initial value of the coordinate and the smallest value it takes in the unconstrained solution of the batch."""
    return 0.5 * (float(ocp.x0[ix]) + float(ref_free.X[:, :, ix].min()))


@dataclasses.dataclass
class Case:
    ocp: object
    P: object
    x0: np.ndarray
    u0: np.ndarray          # pinned u_0 of the Q-mode calls
    ref_v: object           # port, V mode, cold
    ref_q: object           # port, Q mode, cold
    tol: float = None


@functools.lru_cache(maxsize=None)
def case(port, n_mass, N, B, seed, tol=None):
    from mpc4rl_amd import chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp = chain_mass_ocp(n_mass=n_mass, N=N) if tol is None else chain_mass_ocp(n_mass=n_mass, N=N, tol=tol)
    P = make_chain_mass(n_mass=n_mass, N=N)
    x0, rng = chain_x0(ocp, B, seed)
    ref_v = port.solve(P, x0, tol=tol)
    u0 = pinned_u0(rng, B, ref_v.u0)
    ref_q = port.solve(P, x0, u0fix=u0, tol=tol)
    return Case(ocp, P, x0, u0, ref_v, ref_q, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------------------
# raw_solve, outputs, largest_error, same_statuses, report, bit_equal: tests/small_mode_cases.py (shared with test_gpu_small_modes.py)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. horizons x sizes, V mode and Q mode
# ---------------------------------------------------------------------------------------------------------------------------------
# N = 1 has no interior stage; 2, 3 are shorter than one group of chain_sens_ad_kernel at n_mass 3; 15 / 16 / 17 and 31 / 33 sit on
# both sides of the 16-stage batches of the corrector's matrix-core pass (N + 1 stages: 16, 17, 18, 32, 34) and leave ragged stage
# groups at every chain size (4, 2, 1 stages per wavefront at n_mass 3, 5, 7)
SHAPES = [(n_mass, N) for n_mass in (3, 5, 7) for N in (1, 2, 3, 15, 16, 17, 31, 33)]


@pytest.mark.parametrize("n_mass,N", SHAPES)
def test_horizons_v_mode(oracle_port, n_mass, N):
    from mpc4rl_amd import MPCBatch
    c = case(oracle_port, n_mass, N, 3, N)
    mpc = MPCBatch(c.ocp, 3)
    r = mpc.solve(c.x0, sens_v=True, sens_pi=True, cold=True)
    got = outputs(mpc, r)
    same_statuses(got, c.ref_v)
    err = largest_error(got, c.ref_v)
    report(f"V mode n_mass {n_mass} N {N}", err)
    assert err < RTOL, largest_error.last
    assert float((mpc.get_lagrangian() - r.V).abs().max()) < 1e-5      # lam'h + pi'g vanish at a KKT point up to the barrier parameter


@pytest.mark.parametrize("n_mass,N", SHAPES)
def test_horizons_q_mode(oracle_port, n_mass, N):
    from mpc4rl_amd import MPCBatch
    c = case(oracle_port, n_mass, N, 3, N)
    assert abs(c.ref_q.V[0] - c.ref_v.V[0]) < 1e-12 * max(1.0, abs(c.ref_v.V[0]))     # the reference itself: Q(s, u0*(s)) = V(s)
    mpc = MPCBatch(c.ocp, 3)                                                             # a fresh handle
    r = raw_solve(mpc, c.x0, c.u0)
    got = outputs(mpc, r)
    same_statuses(got, c.ref_q)
    assert torch.equal(r.u0, torch.as_tensor(c.u0, device=r.u0.device))                  # the pinned u_0 comes back as it went in
    assert bool((r.dpi_dp == 0.0).all())                                                 # du0*/dp: exact zeros over the NaN fill
    err = largest_error(got, c.ref_q, fields=("V", "dV", "X", "U", "PI"))
    report(f"Q mode n_mass {n_mass} N {N}", err)
    assert err < RTOL, largest_error.last
    assert abs(got["V"][0] - c.ref_v.V[0]) < RTOL * max(1.0, abs(c.ref_v.V[0]))          # row 0 is pinned at its own u0*
    assert float((mpc.get_lagrangian() - r.V).abs().max()) < 1e-5
    # negative control: the same comparison against the port with the pinned u_0 moved by 1e-3
    wrong = oracle_port.solve(c.P, c.x0, u0fix=c.u0 - 1e-3 * np.sign(c.u0))
    assert largest_error(got, wrong, fields=("V", "dV", "X", "U", "PI")) > RTOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. full-SQP warm starts
# ---------------------------------------------------------------------------------------------------------------------------------
WARM_SHAPES = [(3, 10), (5, 40)]
SEED = 1      # groups 2 - 5: one batch of inputs per shape


def next_state(c, seed=1):
    """x1 = the reference's second stage + N(0, 1e-3): where a closed loop would solve next."""
    return c.ref_v.X[:, 1] + np.random.default_rng(seed).normal(0.0, 1e-3, c.x0.shape)


@pytest.mark.parametrize("n_mass,N", WARM_SHAPES)
def test_warm_full_sqp_vs_port(oracle_port, n_mass, N):
    """(a) cold at x0, then a full SQP from the stored iterate at x1, against the port warm-started from its own first result;
    (b) the same call again needs no iteration."""
    from mpc4rl_amd import MPCBatch
    B = 8
    c = case(oracle_port, n_mass, N, B, SEED)
    x1 = next_state(c)
    mpc = MPCBatch(c.ocp, B)
    r0 = mpc.solve(c.x0, cold=True)
    same_statuses(outputs(mpc, r0), c.ref_v)
    r1 = mpc.solve(x1, sens_v=True, sens_pi=True)
    got = outputs(mpc, r1)
    ref1 = oracle_port.solve(c.P, x1, warm=c.ref_v)
    same_statuses(got, ref1)
    err = largest_error(got, ref1)
    report(f"warm V n_mass {n_mass} N {N}", err)
    assert err < RTOL, largest_error.last
    # against a cold solve at x1: V only (a warm and a cold run end at points ~tol apart; V is second order in that distance)
    cold = MPCBatch(c.ocp, B).solve(x1, cold=True)
    assert bool((cold.status == 0).all())
    e = largest_error({"V": r1.V.cpu().numpy()}, {"V": cold.V.cpu().numpy()}, fields=("V",))
    report(f"warm vs cold V n_mass {n_mass} N {N}", e)
    assert e < RTOL
    # (b)
    r2 = mpc.solve(x1, sens_v=True, sens_pi=True)
    assert bool((r2.status == 0).all()) and int(r2.iters[:, 0].max()) == 0
    assert torch.allclose(r2.V, r1.V, rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("n_mass,N", WARM_SHAPES)
def test_warm_between_v_and_q_mode(oracle_port, n_mass, N):
    """(c) what the Q-learning loops do with one handle: Q cold then V warm, and V cold then Q warm."""
    from mpc4rl_amd import MPCBatch
    B = 8
    c = case(oracle_port, n_mass, N, B, SEED)
    # Q -> V
    mpc = MPCBatch(c.ocp, B)
    rq = mpc.solve(c.x0, c.u0, sens_v=True, cold=True)
    same_statuses(outputs(mpc, rq), c.ref_q)
    rv = mpc.solve(c.x0, sens_v=True, sens_pi=True)
    got = outputs(mpc, rv)
    ref = oracle_port.solve(c.P, c.x0, warm=c.ref_q)
    same_statuses(got, ref)
    err = largest_error(got, ref)
    report(f"Q -> V n_mass {n_mass} N {N}", err)
    assert err < RTOL, largest_error.last
    # V -> Q
    mpc = MPCBatch(c.ocp, B)
    rv = mpc.solve(c.x0, sens_v=True, sens_pi=True, cold=True)
    same_statuses(outputs(mpc, rv), c.ref_v)
    rq = mpc.solve(c.x0, c.u0, sens_v=True, sens_pi=True)
    got = outputs(mpc, rq)
    ref = oracle_port.solve(c.P, c.x0, u0fix=c.u0, warm=c.ref_v)
    same_statuses(got, ref)
    assert ref.sqp_iter[0] == 0 and int(rq.iters[0, 0]) == 0          # row 0 is pinned where it already is
    assert bool((rq.dpi_dp == 0.0).all())
    fields = ("u0", "V", "dV", "X", "U", "PI")
    err = largest_error(got, ref, fields=fields)
    report(f"V -> Q n_mass {n_mass} N {N}", err)
    assert err < RTOL, largest_error.last
    wrong = oracle_port.solve(c.P, c.x0, u0fix=c.u0 - 1e-3 * np.sign(c.u0), warm=c.ref_v)
    assert largest_error(got, wrong, fields=fields) > RTOL


@pytest.mark.parametrize("n_mass,N", WARM_SHAPES)
def test_warm_cold_mask(oracle_port, n_mass, N):
    """(d) mpcrl_set_cold_mask on a chain handle (mirrors test_per_instance_cold_mask): masked instances are bit for bit those of a
    cold call, the others bit for bit those of a plain warm call, and the mask is consumed by one solve."""
    from mpc4rl_amd import MPCBatch
    B = 8
    c = case(oracle_port, n_mass, N, B, SEED)
    x1 = next_state(c)
    mask = torch.as_tensor([True, False, False, True, False, True, False, False], device="cuda")      # 3 of 8
    kw = dict(sens_v=True, sens_pi=True, reorder=False)
    a = MPCBatch(c.ocp, B)
    a.solve(c.x0, cold=True, reorder=False)
    ra = a.solve(x1, cold_mask=mask, **kw)
    cold = MPCBatch(c.ocp, B).solve(x1, cold=True, **kw)
    w = MPCBatch(c.ocp, B)
    w.solve(c.x0, cold=True, reorder=False)
    rw = w.solve(x1, **kw)
    assert bool((ra.status == 0).all())
    bit_equal(ra, cold, mask)
    bit_equal(ra, rw, ~mask)
    rb = a.solve(x1, reorder=False)                                    # the mask was one-shot
    assert int(rb.iters[:, 0].max()) == 0


@pytest.mark.parametrize("n_mass,N", WARM_SHAPES)
def test_warm_iterate_rows(oracle_port, n_mass, N):
    """(e) mpcrl_get / set_iterate_rows with the chain's row lengths, (f) a stored iterate without bound multipliers."""
    from mpc4rl_amd import MPCBatch
    B, R = 8, 20
    c = case(oracle_port, n_mass, N, B, SEED)
    nx, nu = c.ocp.nx, c.ocp.nu
    rng = np.random.default_rng(7)
    a = MPCBatch(c.ocp, B)
    ra = a.solve(c.x0, cold=True)
    assert bool((ra.status == 0).all())
    x, u, pi, bnd, _ = a.get_iterate()
    lens = ((N + 1) * nx, N * nu, N * nx, 10 * (N + 1) * (nu + nx))
    tabs = [torch.full((R, n), -7.0, dtype=torch.float64, device="cuda") for n in lens]
    rows = torch.as_tensor(rng.permutation(R)[:B], device="cuda")
    a.get_iterate_rows(*tabs, index=rows)
    untouched = torch.ones(R, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    for t, src in zip(tabs, (x, u, pi, bnd)):
        assert torch.equal(t[rows], src.reshape(B, -1)) and bool((t[untouched] == -7.0).all())
    order = torch.as_tensor(rng.permutation(B), device="cuda")
    b = MPCBatch(c.ocp, B)
    b.set_iterate_rows(*tabs, index=rows[order].contiguous())
    rb = b.solve(torch.as_tensor(c.x0, device="cuda")[order])
    assert bool((rb.status == 0).all()) and int(rb.iters[:, 0].max()) == 0 and torch.equal(rb.u0, ra.u0[order])
    assert torch.equal(b.get_iterate()[0], x[order])
    # a negative index skips the instance
    keep = torch.arange(B, device="cuda") % 2 == 0
    e = MPCBatch(c.ocp, B)
    e.solve(c.x0 * 0.99, cold=True)
    xe = e.get_iterate()[0].clone()
    e.set_iterate_rows(*tabs, index=torch.where(keep, -1, rows))
    xe2 = e.get_iterate()[0]
    assert torch.equal(xe2[keep], xe[keep]) and torch.equal(xe2[~keep], x[~keep])
    tabs2 = [torch.full((R, n), -7.0, dtype=torch.float64, device="cuda") for n in lens]
    a.get_iterate_rows(*tabs2, index=torch.where(keep, -1, rows))
    for t2, src in zip(tabs2, (x, u, pi, bnd)):
        assert bool((t2[rows[keep]] == -7.0).all()) and torch.equal(t2[rows[~keep]], src.reshape(B, -1)[~keep])
    # (f) x, u, pi without the bound planes (MPCRL_COLD_DUAL at the next solve), through both entry points
    p, q = MPCBatch(c.ocp, B), MPCBatch(c.ocp, B)
    p.set_iterate(x, u, pi, None)
    q.set_iterate_rows(x.reshape(B, -1), u.reshape(B, -1), pi.reshape(B, -1), None)
    assert not p.duals_valid and not q.duals_valid
    rp, rq = p.solve(c.x0, sens_v=True, sens_pi=True), q.solve(c.x0, sens_v=True, sens_pi=True)
    bit_equal(rp, rq)
    assert bool((rp.status == 0).all())
    e = largest_error({"V": rp.V.cpu().numpy()}, {"V": ra.V.cpu().numpy()}, fields=("V",))
    report(f"cold-dual V vs cold V n_mass {n_mass} N {N}", e)
    assert e < RTOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. bounds after creation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mass,N", WARM_SHAPES)
def test_bounds_after_creation(oracle_port, n_mass, N):
    """mpcrl_set_bounds on a chain handle.  (a) tighter control bounds; (b) a lower bound on the end point's x position at stages
    1 .. N: the first state row the compact list of bounded coordinates has held (4 rows per interior stage, one terminal row; at
    (5, 40) that is 160 rows — more than two per lane, the interior point's row phases as passes over the workspace); (c) the
    original bounds again; (d) lb > ub."""
    from mpc4rl_amd import MPCBatch, _lib
    B = 8
    c = case(oracle_port, n_mass, N, B, SEED)
    nx, nu = c.ocp.nx, c.ocp.nu
    ix = 3 * (n_mass - 2)
    kw = dict(sens_v=True, sens_pi=True, cold=True)
    mpc = MPCBatch(c.ocp, B)
    first = mpc.solve(c.x0, **kw)
    same_statuses(outputs(mpc, first), c.ref_v)
    free = np.full(nx, 1e30)

    def set_all(bu, lbx, lbx_e):
        mpc.set_bounds(_lib.BOUNDS_U0, -bu * np.ones(nu), bu * np.ones(nu))
        mpc.set_bounds(_lib.BOUNDS_STAGE, np.concatenate([-bu * np.ones(nu), lbx]), np.concatenate([bu * np.ones(nu), free]))
        mpc.set_bounds(_lib.BOUNDS_TERMINAL, lbx_e, free)

    # (a) controls at +-0.5, states absent
    set_all(0.5, -free, -free)
    r = mpc.solve(c.x0, **kw)
    got = outputs(mpc, r)
    on_bound = (np.abs(got["U"]) > 0.5 - 1e-6).reshape(B, -1).sum(1)
    assert on_bound.min() >= 4, on_bound
    ref = oracle_port.solve(with_control_bounds(c.P, 0.5), c.x0)
    same_statuses(got, ref)
    err = largest_error(got, ref)
    report(f"control bounds n_mass {n_mass} N {N}", err)
    assert err < RTOL, largest_error.last
    assert largest_error(got, oracle_port.solve(with_control_bounds(c.P, 0.5 - 1e-3), c.x0)) > RTOL
    # (b) the state bound, through BOUNDS_STAGE and BOUNDS_TERMINAL
    lo = state_bound_level(c.ocp, c.ref_v, ix)
    lbx = -free.copy()
    lbx[ix] = lo
    set_all(1.0, lbx, lbx)
    r = mpc.solve(c.x0, **kw)
    got = outputs(mpc, r)
    ref = oracle_port.solve(with_state_bound(c.P, ix, lo), c.x0)
    lam, lam_ref = got["BND"][:, 0, :, nu + ix], ref.BND[:, 0, :, nu + ix]
    assert (lam.max(1) > 1e-3).sum() >= B // 2 and (lam_ref.max(1) > 1e-3).sum() >= B // 2, (lam.max(1), lam_ref.max(1))
    same_statuses(got, ref)
    assert got["X"][:, 1:, ix].min() > lo - 1e-7
    finite = np.isfinite(ref.dpi).reshape(B, -1).all(1)
    assert finite.sum() >= B // 2
    got["lam"], want = lam, {"u0": ref.u0, "V": ref.V, "dV": ref.dV, "X": ref.X, "U": ref.U, "PI": ref.PI, "lam": lam_ref}
    err = largest_error(got, want, fields=tuple(want))
    e_dpi = largest_error({"dpi": got["dpi"]}, {"dpi": np.nan_to_num(ref.dpi)}, fields=("dpi",), rows=finite)
    report(f"state bound n_mass {n_mass} N {N} (du0*/dp {e_dpi:.3e} on {int(finite.sum())} of {B})", err)
    assert err < RTOL and e_dpi < RTOL, (largest_error.last, e_dpi)
    wrong = oracle_port.solve(with_state_bound(c.P, ix, lo + 1e-3), c.x0)
    wrong = {"u0": wrong.u0, "V": wrong.V, "dV": wrong.dV, "X": wrong.X, "U": wrong.U, "PI": wrong.PI, "lam": wrong.BND[:, 0, :, nu + ix]}
    assert largest_error(got, wrong, fields=tuple(want)) > RTOL
    # (c) the original bounds again: the same request as the first one
    set_all(1.0, -free, -free)
    bit_equal(mpc.solve(c.x0, **kw), first)
    # (d) lb > ub is refused and changes nothing
    with pytest.raises(RuntimeError, match="mpcrl_set_bounds failed"):
        mpc.set_bounds(_lib.BOUNDS_STAGE, np.concatenate([np.ones(nu), -free]), np.concatenate([-np.ones(nu), free]))
    bit_equal(mpc.solve(c.x0, **kw), first)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. statuses
# ---------------------------------------------------------------------------------------------------------------------------------
def test_status_nan_x0(oracle_port):
    """Status 1: a NaN in x0.  One instance per wavefront, so the neighbours are bit for bit what they are without it, and the rows of
    the unsolved instance come back as zeros (two memsets and an early return in four kernels: not the small models' mechanism)."""
    from mpc4rl_amd import MPCBatch
    B = 5
    c = case(oracle_port, 3, 10, B, SEED)
    x0 = c.x0.copy()
    x0[2, 1] = np.nan
    ref = oracle_port.solve(c.P, x0)
    assert list(ref.status) == [0, 0, 1, 0, 0]
    mpc = MPCBatch(c.ocp, B)
    r = raw_solve(mpc, x0)
    assert r.status.tolist() == [0, 0, 1, 0, 0]
    clean_mpc = MPCBatch(c.ocp, B)
    clean = raw_solve(clean_mpc, c.x0)
    others = torch.as_tensor([True, True, False, True, True], device="cuda")
    bit_equal(r, clean, others)
    for t1, t2 in zip(mpc.get_iterate()[:4], clean_mpc.get_iterate()[:4]):
        assert torch.equal(t1[others], t2[others])
    assert bool((r.dV_dp[2] == 0.0).all()) and bool((r.dpi_dp[2] == 0.0).all())
    assert bool(torch.isfinite(r.dV_dp[others]).all()) and bool(torch.isfinite(r.dpi_dp[others]).all())
    got = outputs(mpc, r)
    ok = np.array([0, 1, 3, 4])
    err = largest_error(got, oracle_port.solve(c.P, c.x0), rows=ok)
    report("NaN x0, the four other rows", err)
    assert err < RTOL, largest_error.last


def test_status_max_iter(oracle_port):
    """Status 2 at max_iter = 2 (mpcrl_set_options): the iterate two full steps from the cold start, as the port's."""
    from mpc4rl_amd import MPCBatch
    B = 5
    c = case(oracle_port, 3, 10, B, SEED)
    mpc = MPCBatch(c.ocp, B)
    mpc.set_options(max_iter=2)
    r = mpc.solve(c.x0, sens_v=True, sens_pi=True, cold=True)
    ref = oracle_port.solve(c.P, c.x0, max_iter=2)
    assert np.all(ref.status == 2) and np.all(ref.sqp_iter == 2)
    assert bool((r.status == 2).all()) and bool((r.iters[:, 0] == 2).all())
    got = outputs(mpc, r)
    err = largest_error(got, ref, fields=("u0", "V", "X", "U"))
    report("max_iter 2", err)
    assert err < RTOL, largest_error.last
    # negative control: two iterations with the control bounds moved by 1e-3 (the first interior-point solves feel them)
    wrong = oracle_port.solve(with_control_bounds(c.P, 1.0 - 1e-3), c.x0, max_iter=2)
    assert largest_error(got, wrong, fields=("u0", "V", "X", "U")) > RTOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the mirror leg
# ---------------------------------------------------------------------------------------------------------------------------------
MIRROR = dict(n_mass=3, N=10, B=8, seed=SEED, tol=1e-8)      # the mirror's du0*/dp at 1e-6 needs the KKT point (as the other mirror tests)


def mirror_q_mode(P, it, x0, u0, V, rows=(2, 3)):
    """certify() at the Q-mode iterate `it` = (X, U, PI, BND) of the given rows -> (dL/dp [n, n_p], L [n])."""
    from oracle.from_iterate import certify
    dL, L = [], []
    for i in rows:
        mr, _, _ = certify(P, it[0][i], it[1][i], it[2][i], it[3][i], x0[i], u0fix=u0[i], cost=float(V[i]))
        dL.append(mr.dL_dp[0]), L.append(mr.L)
    return np.array(dL), np.array(L)


def mirror_state_bound(P_sb, it, x0, V, rows):
    """certify() at a V-mode iterate with the state bound active -> (dL/dp, dz/dp[:nu], L, strict-complementarity margins)."""
    from oracle.from_iterate import certify
    dL, dpi, L, sc = [], [], [], []
    for i in rows:
        mr, s, _ = certify(P_sb, it[0][i], it[1][i], it[2][i], it[3][i], x0[i], cost=float(V[i]))
        dL.append(mr.dL_dp[0]), dpi.append(mr.dpi_dp), L.append(mr.L), sc.append(s)
    return np.array(dL), np.array(dpi), np.array(L), np.array(sc)


def mirror_state_bound_problem(port, c):
    """The state-bound problem of the mirror case and the first two instances on which the port finds the bound active."""
    ix = 3 * (MIRROR["n_mass"] - 2)
    lo = state_bound_level(c.ocp, c.ref_v, ix)
    P_sb = with_state_bound(c.P, ix, lo)
    ref = port.solve(P_sb, c.x0, tol=c.tol)
    active = np.flatnonzero(ref.BND[:, 0, :, c.ocp.nu + ix].max(1) > 1e-3)
    assert np.all(ref.status == 0) and len(active) >= 2
    return ix, lo, P_sb, ref, active[:2]


def test_mirror_q_mode(oracle_port):
    """The autograd mirror of the reference's NLP at the DEVICE iterate of two Q-mode instances: its thresholds hold there, and
    dQ/dp is the mirror's dL/dp."""
    from mpc4rl_amd import MPCBatch
    c = case(oracle_port, *[MIRROR[k] for k in ("n_mass", "N", "B", "seed", "tol")])
    mpc = MPCBatch(c.ocp, MIRROR["B"])
    r = mpc.solve(c.x0, c.u0, sens_v=True, sens_pi=True, cold=True)
    got = outputs(mpc, r)
    same_statuses(got, c.ref_q)
    rows = (2, 3)
    dL, L = mirror_q_mode(c.P, (got["X"], got["U"], got["PI"], got["BND"]), c.x0, c.u0, got["V"], rows)
    sel = list(rows)
    have = {"dV": got["dV"][sel], "L": mpc.get_lagrangian().cpu().numpy()[sel]}
    err = largest_error(have, {"dV": dL, "L": L}, fields=("dV", "L"))
    report("mirror, Q mode", err)
    assert err < RTOL, largest_error.last
    wrong = oracle_port.solve(c.P, c.x0, u0fix=c.u0 - 1e-3 * np.sign(c.u0), tol=c.tol)
    assert largest_error(have, {"dV": wrong.dV[sel], "L": wrong.V[sel]}, fields=("dV", "L")) > RTOL


def test_mirror_active_state_bound(oracle_port):
    """... and at two instances whose state bound is active: dV/dp and du0*/dp (the mirror's dense solve with the iterate's own
    lam / t on the active rows) at 1e-6, with the strict-complementarity margin of the cartpole active-bound test."""
    from mpc4rl_amd import MPCBatch, _lib
    c = case(oracle_port, *[MIRROR[k] for k in ("n_mass", "N", "B", "seed", "tol")])
    ix, lo, P_sb, ref, rows = mirror_state_bound_problem(oracle_port, c)
    nx, nu = c.ocp.nx, c.ocp.nu
    mpc = MPCBatch(c.ocp, MIRROR["B"])
    lb, ub = np.concatenate([-np.ones(nu), np.full(nx, -1e30)]), np.concatenate([np.ones(nu), np.full(nx, 1e30)])
    lb[nu + ix] = lo
    mpc.set_bounds(_lib.BOUNDS_STAGE, lb, ub)
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, lb[nu:], ub[nu:])
    r = mpc.solve(c.x0, sens_v=True, sens_pi=True, cold=True)
    got = outputs(mpc, r)
    same_statuses(got, ref)
    assert np.all(got["BND"][rows, 0, :, nu + ix].max(1) > 1e-3)
    dL, dpi, L, sc = mirror_state_bound(P_sb, (got["X"], got["U"], got["PI"], got["BND"]), c.x0, got["V"], rows)
    print("[chain modes] strict-complementarity margins", sc)
    assert sc.min() >= 1e-4
    have = {"dV": got["dV"][rows], "dpi": got["dpi"][rows], "L": mpc.get_lagrangian().cpu().numpy()[rows]}
    err = largest_error(have, {"dV": dL, "dpi": dpi, "L": L}, fields=("dV", "dpi", "L"))
    report("mirror, active state bound", err)
    assert err < RTOL, largest_error.last
    wrong = oracle_port.solve(with_state_bound(c.P, ix, lo + 1e-3), c.x0, tol=c.tol)
    assert largest_error(have, {"dV": wrong.dV[rows], "dpi": wrong.dpi[rows], "L": wrong.V[rows]}, fields=("dV", "dpi", "L")) > RTOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the two row stores of the interior point at their switch
# ---------------------------------------------------------------------------------------------------------------------------------
# Up to 128 bound rows (two per lane) stay in registers, more go through the workspace.  n_mass 3, N = 11 with bounds on the three
# controls and all nine states at the interior stages has n0 + 10 * 12 + ne rows: n0 = 3 (V mode) or 0 (Q mode: u_0 is pinned) at
# stage 0, ne bounded states at the terminal stage.  128 rows: the register store with the second row of lane 63 in use; 129: the
# workspace store.  The state bounds are loose (+-LOOSE: rows of the interior point that never bind) but for one lower bound on the
# end point's x position, which is active on part of the batch.
EDGE = dict(n_mass=3, N=11, B=4, seed=SEED)
LOOSE = 1e3
EDGE_CASES = [(False, 5, 128), (False, 6, 129), (True, 8, 128), (True, 9, 129)]


def with_loose_state_bounds(P_sb, ne):
    """P_sb = with_state_bound(...): every other state bounded by +-LOOSE at stages 1 .. N - 1, the first ne states at stage N."""
    nx = P_sb.nx
    lbx = np.full(nx, -LOOSE)
    lbx[int(P_sb.idxbx[0])] = float(P_sb.lbx[0])
    ubx = np.full(nx, LOOSE)
    return dataclasses.replace(P_sb, idxbx=np.arange(nx), lbx=lbx, ubx=ubx, idxbx_e=np.arange(ne), lbx_e=lbx[:ne], ubx_e=ubx[:ne])


@functools.lru_cache(maxsize=None)
def edge_case(port, qmode, ne):
    """(the bounded problem, the pinned u_0 or None, the port's solution, the port's solution with the active bound moved by 1e-3)"""
    c = case(port, *[EDGE[k] for k in ("n_mass", "N", "B", "seed")])
    ix = 3 * (EDGE["n_mass"] - 2)
    u0, free = None, c.ref_v
    if qmode:      # x_1[ix] = x_0[ix] + dT u_0[0] is pinned with u_0: on the feasible side of a bound below x_0[ix]
        u0 = c.u0.copy()
        u0[:, 0] = np.abs(u0[:, 0])
        free = port.solve(c.P, c.x0, u0fix=u0)
        assert np.all(free.status == 0)
    lo = state_bound_level(c.ocp, free, ix)
    P = with_loose_state_bounds(with_state_bound(c.P, ix, lo), ne)
    wrong = with_loose_state_bounds(with_state_bound(c.P, ix, lo + 1e-3), ne)
    return c, ix, P, u0, port.solve(P, c.x0, u0fix=u0), port.solve(wrong, c.x0, u0fix=u0)


@pytest.mark.parametrize("qmode,ne,rows", EDGE_CASES)
def test_row_store_switch(oracle_port, qmode, ne, rows):
    from mpc4rl_amd import MPCBatch, _lib
    c, ix, P, u0, ref, wrong = edge_case(oracle_port, qmode, ne)
    nx, nu, N, B = c.ocp.nx, c.ocp.nu, EDGE["N"], EDGE["B"]
    assert (0 if qmode else nu) + (N - 1) * (nu + nx) + ne == rows
    assert np.abs(ref.X).max() < 1e-2 * LOOSE < 1e-4 * _lib.NO_BOUND
    mpc = MPCBatch(c.ocp, B)
    lbe, ube = np.full(nx, -1e30), np.full(nx, 1e30)
    lbe[:ne], ube[:ne] = P.lbx_e, P.ubx_e
    mpc.set_bounds(_lib.BOUNDS_STAGE, np.concatenate([-np.ones(nu), P.lbx]), np.concatenate([np.ones(nu), P.ubx]))
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, lbe, ube)
    r = mpc.solve(c.x0, u0, sens_v=True, sens_pi=True, cold=True)
    got = outputs(mpc, r)
    same_statuses(got, ref)
    lam, lam_ref = got["BND"][:, 0, :, nu + ix], ref.BND[:, 0, :, nu + ix]
    assert (lam.max(1) > 1e-3).sum() >= 2 and (lam_ref.max(1) > 1e-3).sum() >= 2, (lam.max(1), lam_ref.max(1))      # the active row
    others = nu + np.flatnonzero(np.arange(nx) != ix)      # the loose rows: slack ~LOOSE, multiplier = (barrier parameter) / slack
    assert max(np.abs(got["BND"][:, :2][..., others]).max(), np.abs(ref.BND[:, :2][..., others]).max()) < 1e-6
    assert got["X"][:, 1:, ix].min() > float(P.lbx[ix]) - 1e-7
    err = largest_error(got, ref)
    report(f"{rows} bound rows, {'Q' if qmode else 'V'} mode", err)
    assert err < RTOL, largest_error.last
    assert largest_error(got, wrong) > RTOL      # negative control: the active bound moved by 1e-3
