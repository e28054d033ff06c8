"""GPU parity at the sizes bench.py times (BASELINE.json configs 2-4) and a certification of the HIP iterate by the mirror of the
reference's NLP.

  * cartpole 4096 (the bench inputs) and a hard distribution of 2048 states, linear system 4096, chain n_mass 5 at B = 1024:
    the HIP path through the C ABI against the oracle's C++ port on the same inputs — status, SQP / interior-point iteration
    counts, u0*, V, dV/dp, du0*/dp within 1e-6 relative (north_star).
  * mirror certification: x, u, pi, lam, t pulled out of the handle with mpcrl_get_iterate are fed to oracle/nlp_mirror.py (the
    restatement of rlmpc/mpc/nlp.py's L, R, z) exactly as update_nlp copies them out of acados (nlp.py:1354-1398); the reference's
    own consistency thresholds (nlp.py:1445-1537) must hold AT THE PRODUCT'S ITERATE, and the mirror's dL/dp and
    dz/dp[:nu] = -(dR/dz)^-1 dR/dp (nlp.py:1401,1410-1424; torch autograd + a dense solve) must equal the kernel's dV/dp and
    du0*/dp.  This ties the product to the reference-held checks without going through the SQP oracle.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def rel_rows(a, b, floor=1.0):
    """per-instance max relative error, scaled by the largest entry of the instance's reference row"""
    B = len(b)
    a, b = np.asarray(a, float).reshape(B, -1).copy(), np.asarray(b, float).reshape(B, -1).copy()
    both_nan = np.isnan(a) & np.isnan(b)     # du0*/dp is NaN on both sides where the exact-Hessian KKT matrix is not positive definite
    a[both_nan], b[both_nan] = 0.0, 0.0
    return (np.abs(a - b) / np.maximum(np.abs(b).max(1, keepdims=True), floor)).max(1) if B else np.zeros(0)


def compare(r, ref, min_conv, strict=None, name="", dpi_tol=RTOL):
    st, it = r.status.cpu().numpy(), r.iters.cpu().numpy()
    same = st == ref.status
    ok = (st == 0) & (ref.status == 0)
    conv = (st == 0).mean()
    e = {"u0": rel_rows(r.u0.cpu().numpy()[ok], ref.u0[ok]), "V": rel_rows(r.V.cpu().numpy()[ok], ref.V[ok]),
         "dV": rel_rows(r.dV_dp.cpu().numpy()[ok], ref.dV[ok])}
    sel = ok if strict is None else ok & strict
    # du0*/dp is NaN where the exact-Hessian KKT matrix of the adjoint solve is not positive definite (both sides test their own
    # pivots: a pivot within rounding of zero can fall either way, and what the other side then returns is ill-conditioned garbage)
    dpi_k = r.dpi_dp.cpu().numpy()
    nan_k, nan_r = np.isnan(dpi_k).reshape(len(st), -1).any(1), np.isnan(ref.dpi).reshape(len(st), -1).any(1)
    assert (nan_k != nan_r)[ok].mean() < 0.01
    sel = sel & ~nan_k & ~nan_r
    e["dpi"] = rel_rows(dpi_k[sel], ref.dpi[sel])
    sqp_eq, ipm_eq = (it[ok, 0] == ref.sqp_iter[ok]).mean(), (it[ok, 1] == ref.ipm_iter[ok]).mean()
    print(f"{name}: B {len(st)} status equal {same.mean():.4f} converged gpu {conv:.4f} port {(ref.status == 0).mean():.4f} "
          f"sqp iters equal {sqp_eq:.4f} ipm iters equal {ipm_eq:.4f} " + " ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
    assert conv >= min_conv
    # the same iteration in two arithmetic orders: iteration counts differ only where a stopping test is met to within rounding
    assert np.abs(it[ok, 0] - ref.sqp_iter[ok]).max() <= 1 and sqp_eq > 0.97 and ipm_eq > 0.95
    for k, v in e.items():
        assert v.max() < (dpi_tol if k == "dpi" else RTOL), (k, float(v.max()))
    return same, ok


def test_cartpole_bench_inputs_vs_port(oracle_port):
    """BASELINE config 2/3 at full size: the 4096 instances bench.py times (make_inputs(4096, rank 0)), every one against the port."""
    import bench
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    from oracle.problems import make_cartpole
    x0 = bench.make_inputs(4096, 0)
    mpc = MPCBatch(cartpole_ocp(), 4096)
    r = mpc.solve(torch.as_tensor(x0, device="cuda"), sens_v=True, sens_pi=True, cold=True)
    ref = oracle_port.solve(make_cartpole(), x0)
    same, ok = compare(r, ref, 1.0, name="cartpole bench inputs")
    assert same.all() and ok.all()
    res = mpc.get_iterate()[4].cpu().numpy()
    assert res.max() < 1e-6 and np.abs(res - ref.res).max() < 1e-6


def test_cartpole_hard_distribution_vs_port(oracle_port):
    """2048 states from the box +-[2, 3, pi, 3] at max_iter = 60: full-step SQP without globalisation (what the reference runs,
    config/cartpole.yaml:8-14) fails on part of them, on both sides alike; everything both sides solve must agree."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    from oracle.problems import make_cartpole
    rng = np.random.default_rng(5)
    lohi = np.array([2.0, 3.0, np.pi, 3.0])
    x0 = rng.uniform(-lohi, lohi, (2048, 4))
    mpc = MPCBatch(cartpole_ocp(max_iter=60), 2048)
    r = mpc.solve(torch.as_tensor(x0, device="cuda"), sens_v=True, sens_pi=True, cold=True)
    ref = oracle_port.solve(make_cartpole(), x0, max_iter=60)
    st = r.status.cpu().numpy()
    # du0*/dp is compared where strict complementarity holds at the port's solution (a weakly active bound makes it ill-defined)
    lam, t = ref.BND[:, 0:2].reshape(2048, -1), ref.BND[:, 2:4].reshape(2048, -1)
    strict = np.maximum(lam, t).min(1) >= 1e-3
    same, ok = compare(r, ref, 0.8, strict=strict, name="cartpole hard distribution")
    assert same.mean() > 0.995           # the rest: chaotic non-converging iterations that end differently in two arithmetic orders


def test_linear_bench_inputs_vs_port(oracle_port):
    """`bench.py --workload linear` at its size: 4096 states of the environment's box interior, gamma = 0.99."""
    from mpc4rl_amd import MPCBatch, linear_system_ocp
    from oracle.problems import make_linear_system
    rng = np.random.default_rng(0)
    B = 4096
    x0 = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.5, 0.5, B)])
    mpc = MPCBatch(linear_system_ocp(discount_factor=0.99), B)
    r = mpc.solve(torch.as_tensor(x0, device="cuda"), sens_v=True, sens_pi=True, cold=True)
    ref = oracle_port.solve(make_linear_system(gamma=0.99), x0)
    s = np.abs(ref.BND[:, 4:6]).reshape(B, -1).max(axis=1)      # quirk q1: du0/dp is ill-defined where a soft bound is active
    # The regulated state x[0] approaches the origin, which IS its (soft) lower bound (linear_system/acados.py:73-131: x in [0, 1]):
    # every instance ends with a weakly active row (lam ~ 8e-6, t ~ 3e-6 at a late stage), i.e. NO instance passes the
    # strict-complementarity filter of SURVEY.md §8c (margin >= 1e-3), and lam / t of that row carries a 1e-12 absolute rounding
    # difference of t as a 1e-6 relative one into du0*/dp.  u0*, V, dV/dp hold the 1e-6 bar (measured 7e-12, 8e-13, 1e-9);
    # du0*/dp is held to 2e-5 (measured 7e-6 on the worst of 4096, identical iteration counts on all of them).
    same, ok = compare(r, ref, 1.0, strict=s < 1e-9, name="linear bench inputs", dpi_tol=2e-5)
    assert same.all()


def chain_all_vs_port(r, ref, B, name):
    """Every instance of a chain batch against the port: statuses and SQP iteration counts, interior-point counts (equal except where a
    stopping test is met to within rounding), the four outputs at 1e-6 (rows scaled by the instance's largest reference entry)."""
    st, it = r.status.cpu().numpy(), r.iters.cpu().numpy()
    assert np.array_equal(st, ref.status) and np.all(ref.status == 0)
    sqp_eq, ipm_eq = (it[:, 0] == ref.sqp_iter).mean(), (it[:, 1] == ref.ipm_iter).mean()
    e = {"u0": rel_rows(r.u0.cpu().numpy(), ref.u0), "V": rel_rows(r.V.cpu().numpy(), ref.V), "dV": rel_rows(r.dV_dp.cpu().numpy(), ref.dV),
         "dpi": rel_rows(r.dpi_dp.cpu().numpy(), ref.dpi, floor=1e-300)}
    print(f"{name}: B {B} sqp iters equal {sqp_eq:.4f} ipm iters equal {ipm_eq:.4f} " + " ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
    assert np.abs(it[:, 0] - ref.sqp_iter).max() <= 1 and sqp_eq > 0.97 and ipm_eq > 0.95
    for k, v in e.items():
        assert v.max() < RTOL, (k, float(v.max()), int(v.argmax()))


def test_chain5_bench_size_vs_port(oracle_port):
    """BASELINE config 4 (n_mass = 5, N = 40, B = 1024, the inputs of `bench.py --workload chain5`): ALL 1024 instances against the
    port (statuses, iteration counts, u0*, V, dV/dp, du0*/dp at 1e-6), then size-independent properties of the batch."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp, P = chain_mass_ocp(n_mass=5), make_chain_mass(n_mass=5)
    B = 1024
    rng = np.random.default_rng(0)
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 12:] += rng.normal(0.0, 1e-2, (B, 9))
    mpc = MPCBatch(ocp, B)
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    assert float(mpc.get_iterate()[4].max()) < 1e-5 and float(r.u0.abs().max()) <= 1.0 + 1e-9
    assert bool(torch.isfinite(r.dV_dp).all()) and bool(torch.isfinite(r.dpi_dp).all())
    chain_all_vs_port(r, oracle_port.solve(P, x0), B, "chain n_mass 5 bench inputs")
    # a second call from the stored iterate needs no iteration and reproduces the outputs; the batch order changes nothing
    r2 = mpc.solve(x0, sens_v=True)
    assert int(r2.iters[:, 0].max()) == 0 and torch.allclose(r2.V, r.V, rtol=1e-13)
    perm = rng.permutation(B)
    rp = MPCBatch(ocp, B).solve(x0[perm], sens_v=True, sens_pi=True, cold=True)      # (the same request: bit for bit)
    idx = torch.as_tensor(perm, device=r.V.device)
    assert torch.equal(rp.V, r.V[idx]) and torch.equal(rp.dV_dp, r.dV_dp[idx]) and torch.equal(rp.dpi_dp, r.dpi_dp[idx])
    # dV/dp has ONE evaluation order whatever the flags (grad_theta (nu' F) always comes off the tables of the second-order point pass,
    # chain_sens_th2_kernel): the same bits with and without du0*/dp
    rv = MPCBatch(ocp, B).solve(x0[perm], sens_v=True, cold=True)
    assert torch.equal(rv.V, rp.V) and torch.equal(rv.dV_dp, rp.dV_dp)


# ---------------------------------------------------------------------------------------------------------------------------------
# mirror certification of the HIP iterate
# ---------------------------------------------------------------------------------------------------------------------------------
def _certify_batch(name, kw, mpc, r, x0, theta=None, u0=None, gamma=None, idx=None, procs=8):
    from oracle.from_iterate import certify_job      # the worker lives in an importable module (fresh interpreters unpickle it)
    x, u, pi, bnd, _ = [t.cpu().numpy() for t in mpc.get_iterate()]
    V = r.V.cpu().numpy()
    idx = range(len(x0)) if idx is None else idx
    jobs = [(name, kw, x[i], u[i], pi[i], bnd[i], x0[i], None if theta is None else theta[i], None if u0 is None else u0[i], gamma,
             float(V[i])) for i in idx]
    # one thread per worker: the GPU boxes show 256 logical CPUs behind a quota of 16, and a BLAS pool of 256 threads in each of 8
    # workers makes the dense solves take minutes (the children inherit these variables at spawn)
    saved = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}
    os.environ.update({k: "1" for k in saved})
    try:
        with mp.get_context("spawn").Pool(min(procs, len(jobs))) as pool:
            rows = pool.map(certify_job, jobs, chunksize=1)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return [np.array([row[c] for row in rows]) for c in range(6)]


def _check_certified(r, L_dev, out, idx, q_mode=False, strict_margin=1e-3, soft=False, dpi_tol=RTOL):
    dL, dpi, L, sc, smax, stat = out
    sel = np.asarray(list(idx))
    dV_k, dpi_k = r.dV_dp.cpu().numpy()[sel], r.dpi_dp.cpu().numpy()[sel]
    e_dV = rel_rows(dV_k, dL)
    assert e_dV.max() < RTOL, ("dV/dp vs mirror dL/dp", float(e_dV.max()))
    assert rel_rows(L_dev.cpu().numpy()[sel], L).max() < RTOL                  # mpcrl_get_lagrangian == nlp.L at the iterate
    if q_mode:
        assert np.all(dpi_k == 0.0)                                             # u_0 pinned: the product reports exact zeros
        return
    # dz/dp of the mirror is only defined where strict complementarity holds (interior-point iterate: lam t ~ 1e-11 on every row)
    # and, with L1-soft bounds, where no slack is active (quirk q1: the reference's own system is rank-deficient there)
    good = (sc >= strict_margin) if not soft else (smax < 1e-9)
    assert good.mean() >= 0.5
    e = (np.abs(dpi_k - dpi).reshape(len(sel), -1).max(1) / np.maximum(np.abs(dpi).reshape(len(sel), -1).max(1), 1.0))
    print("mirror certification: dV/dp", float(e_dV.max()), "du0/dp", float(e[good].max()), "on", int(good.sum()), "of", len(sel),
          "stationarity at the HIP iterate", float(stat.max()))
    assert e[good].max() < dpi_tol, float(e[good].max())


def test_mirror_certifies_the_hip_iterate_cartpole():
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    ocp = cartpole_ocp()
    rng = np.random.default_rng(11)
    B = 32
    x0 = np.zeros((B, 4))
    x0[:16, 2] = rng.uniform(0.9 * np.pi, 1.1 * np.pi, 16)                         # the reference's reset distribution
    x0[16:] = rng.uniform(-1, 1, (16, 4)) * np.array([0.5, 1.0, 0.3, 1.0])         # near upright: u0 not saturated
    theta = np.tile(ocp.p0, (B, 1))
    theta[:, :3] *= rng.uniform(0.9, 1.1, (B, 3))
    mpc = MPCBatch(ocp, B)
    mpc.set_theta(torch.as_tensor(theta))
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    out = _certify_batch("cartpole", {}, mpc, r, x0, theta=theta)
    _check_certified(r, mpc.get_lagrangian(), out, range(B))
    # Q(s, a): u_0 pinned (mpc.py:52-96)
    u0 = rng.uniform(-25, 25, (8, 1))
    mq = MPCBatch(ocp, 8)
    rq = mq.solve(x0[16:24], u0, sens_v=True, sens_pi=True, cold=True)
    assert bool((rq.status == 0).all())
    outq = _certify_batch("cartpole", {}, mq, rq, x0[16:24], u0=u0)
    _check_certified(rq, mq.get_lagrangian(), outq, range(8), q_mode=True)


def test_mirror_certifies_the_hip_iterate_cartpole_active_state_bound():
    """The mirror of the reference's NLP (dense pivoted solve with the iterate's own lam / t ~ 1e20 on the active rows) at the four G7b states
    whose cart reaches the end of the track: the position bound |s| <= 2.4 (config/cartpole.yaml:82-91) is active on the horizon, u0* is not
    saturated.  Until round 6 the adjoint solve's stiffness cap left du0/dp 1.5e-6 ... 3.6e-6 off there; with the Richardson extrapolation
    in the cap (SmallSolver::sensitivities) the 1e-6 bar holds against the reference-anchored leg as well."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7b_cartpole_grad.npz"))
    x0 = g["x0"][:4]
    mpc = MPCBatch(cartpole_ocp(tol=1e-9), 4)
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    bnd = mpc.get_iterate()[3].cpu().numpy()
    assert np.all(bnd[:, 0:2, 1:, 1:].reshape(4, -1).max(1) > 1e-3)            # a state row's multiplier is active on every one of them
    out = _certify_batch("cartpole", {}, mpc, r, x0)
    _check_certified(r, mpc.get_lagrangian(), out, range(4), strict_margin=1e-4)


def test_mirror_certifies_the_hip_iterate_linear():
    from mpc4rl_amd import MPCBatch, linear_system_ocp
    rng = np.random.default_rng(12)
    B = 32
    x0 = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.5, 0.5, B)])
    x0[0] = [0.5, 0.5]                                                              # linear_system/environment.py:46
    for gamma in (0.99, 0.9):
        mpc = MPCBatch(linear_system_ocp(discount_factor=gamma), B)
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
        assert bool((r.status == 0).all())
        out = _certify_batch("linear", {"gamma": gamma}, mpc, r, x0, gamma=gamma)
        # (every instance carries a weakly active row at the origin = the soft bound of x[0], see test_linear_bench_inputs_vs_port:
        # the mirror's dz/dp, which differentiates lam t = tau with the iterate's own lam / t, is held to 1e-5 there; measured 1.5e-6)
        _check_certified(r, mpc.get_lagrangian(), out, range(B), soft=True, dpi_tol=1e-5)


def test_mirror_certifies_the_hip_iterate_chain():
    """n_mass 3 (4 instances), the even size 4 (2 instances: the ragged row groups of the round-4 sweeps against the mirror of the
    reference's own nlp.py) and n_mass 5 (2 instances; 2 385 KKT unknowns x 499 parameters, ~15 s of autograd + dense LU each)."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    rng = np.random.default_rng(13)
    for n_mass, B in ((3, 4), (4, 2), (5, 2)):
        ocp = chain_mass_ocp(n_mass=n_mass, tol=1e-8)   # the mirror's thresholds are looser, du0/dp at 1e-6 needs the KKT point
        M = n_mass - 2
        x0 = np.tile(ocp.x0, (B, 1))
        x0[1:, 3 * (M + 1):] += rng.normal(0.0, 1e-2, (B - 1, 3 * M))
        mpc = MPCBatch(ocp, B)
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
        assert bool((r.status == 0).all())
        out = _certify_batch("chain", {"n_mass": n_mass}, mpc, r, x0)
        dL, dpi, L, sc, smax, stat = out
        assert rel_rows(r.dV_dp.cpu().numpy(), dL).max() < RTOL
        dk = r.dpi_dp.cpu().numpy()
        assert (np.abs(dk - dpi).reshape(B, -1).max(1) / np.abs(dpi).reshape(B, -1).max(1)).max() < RTOL
        assert rel_rows(mpc.get_lagrangian().cpu().numpy(), L).max() < RTOL


def test_mirror_certifies_the_hip_iterate_chain_n6_n7():
    """The perf dimension of BASELINE config 4 against the reference-anchored leg: one perturbed instance each of n_mass 6 (nx 27: 2 787
    KKT unknowns x 823 parameters) and n_mass 7 (nx 33: 3 357 x 1 173) at tol 1e-8 — the reference's update_nlp thresholds at the HIP
    iterate, dL/dp and dz/dp[:nu] of the mirror against the kernels' dV/dp, du0*/dp at 1e-6.  Both run at once (~45 s / ~70 s of autograd
    + dense LU on one core each)."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.from_iterate import certify_job
    rng = np.random.default_rng(17)
    jobs, held = [], []
    for n_mass in (6, 7):
        ocp = chain_mass_ocp(n_mass=n_mass, tol=1e-8)
        M = n_mass - 2
        x0 = np.tile(ocp.x0, (1, 1))
        x0[:, 3 * (M + 1):] += rng.normal(0.0, 1e-2, (1, 3 * M))
        mpc = MPCBatch(ocp, 1)
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
        assert bool((r.status == 0).all())
        x, u, pi, bnd, _ = [t.cpu().numpy() for t in mpc.get_iterate()]
        jobs.append(("chain", {"n_mass": n_mass}, x[0], u[0], pi[0], bnd[0], x0[0], None, None, None, float(r.V[0])))
        held.append((n_mass, r, mpc.get_lagrangian().cpu().numpy()))
    saved = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}
    os.environ.update({k: "1" for k in saved})
    try:
        with mp.get_context("spawn").Pool(2) as pool:
            rows = pool.map(certify_job, jobs, chunksize=1)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    for (n_mass, r, L_dev), (dL, dpi, L, sc, smax, stat) in zip(held, rows):
        e_dV = rel_rows(r.dV_dp.cpu().numpy(), dL[None])
        e_dpi = np.abs(r.dpi_dp.cpu().numpy()[0] - dpi).max() / np.abs(dpi).max()
        print(f"mirror certification chain n_mass {n_mass}: dV/dp {float(e_dV.max()):.2e} du0/dp {float(e_dpi):.2e} stationarity {stat:.2e}")
        assert e_dV.max() < RTOL and e_dpi < RTOL and abs(L_dev[0] - L) <= RTOL * max(1.0, abs(L))


def _cores():
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return n


def test_mirror_certifies_the_bench_inputs():
    """The only reference-anchored check of the repo on the inputs the benchmark itself times.
      * cartpole: 256 of the 4096 instances of `bench.py` (bench.make_inputs(4096, rank 0), every 16th): the reference's update_nlp
        thresholds (nlp.py:1445-1537) hold at the HIP iterate and dL/dp, dz/dp[:nu] of the mirror (nlp.py:1401,1410-1424) equal the
        kernel's dV/dp, du0*/dp at 1e-6;
      * chain n_mass 5: 16 instances of `bench.py --workload chain5` at the REFERENCE'S OWN tolerance 1e-5 (ocp_utils.py:311-312) —
        what tests/test_chain_mass.py really asserts through update_nlp: its thresholds at the iterate acados would hand over;
      * linear system: initial states that move AWAY from the soft bound x[0] >= 0 (x[1] >= 0), where no row ends weakly active and
        the slacks are zero: du0*/dp at 1e-6 (the bench box [0.15, 0.85] x [-0.5, 0.5] is held to 1e-5 above for that reason)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from mpc4rl_amd import MPCBatch, cartpole_ocp, chain_mass_ocp, linear_system_ocp
    # every worker imports torch and counts as a process that holds the GPU, beside this one: at most 16 of them may at once
    procs = max(2, min(8, _cores()))
    x0 = bench.make_inputs(4096, 0)
    mpc = MPCBatch(cartpole_ocp(), 4096)
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    idx = np.arange(0, 4096, 16)
    out = _certify_batch("cartpole", {}, mpc, r, x0, idx=idx, procs=procs)
    _check_certified(r, mpc.get_lagrangian(), out, idx)
    # chain, at the reference's tolerance
    ocp = chain_mass_ocp(n_mass=5)
    B = 16
    rng = np.random.default_rng(0)
    xc = np.tile(ocp.x0, (B, 1))
    xc[:, 12:] += rng.normal(0.0, 1e-2, (B, 9))
    mc = MPCBatch(ocp, B)
    rc = mc.solve(xc, sens_v=True, sens_pi=True, cold=True)
    assert bool((rc.status == 0).all())
    dL, dpi, L, sc, smax, stat = _certify_batch("chain", {"n_mass": 5}, mc, rc, xc, procs=min(procs, 8))
    e_dpi = (np.abs(rc.dpi_dp.cpu().numpy() - dpi).reshape(B, -1).max(1) / np.abs(dpi).reshape(B, -1).max(1)).max()
    print("chain5 at tol 1e-5: dV/dp", float(rel_rows(rc.dV_dp.cpu().numpy(), dL).max()), "du0/dp", float(e_dpi), "stationarity", float(stat.max()))
    assert rel_rows(rc.dV_dp.cpu().numpy(), dL).max() < RTOL and rel_rows(mc.get_lagrangian().cpu().numpy(), L).max() < RTOL
    assert e_dpi < 1e-5          # both linearise at the same iterate, which is itself 1e-5 from the KKT point
    # linear system away from the soft bound
    B = 32
    rng = np.random.default_rng(21)
    xl = np.column_stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.0, 0.6, B)])
    for gamma in (0.99, 0.9):
        ml = MPCBatch(linear_system_ocp(discount_factor=gamma), B)
        rl = ml.solve(xl, sens_v=True, sens_pi=True, cold=True)
        assert bool((rl.status == 0).all())
        out = _certify_batch("linear", {"gamma": gamma}, ml, rl, xl, gamma=gamma, procs=procs)
        _check_certified(rl, ml.get_lagrangian(), out, range(B), soft=True, dpi_tol=RTOL)


def test_rccl_world1_allreduce_and_td3_step():
    """The `nccl` (= RCCL) path that multi-GPU runs take, exercised on one GPU: init_process_group("nccl") with world size 1,
    allreduce_weighted_grad through the K5 reduction kernel + the collective, and one BatchedTD3.train step whose single
    all-reduce carries the critic gradients and the theta-gradient."""
    import socket
    import torch.distributed as dist
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedTD3, cartpole_ocp
    from mpc4rl_amd.distributed import allreduce_weighted_grad, mean_update
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        one = torch.ones(1, dtype=torch.float64, device=dev)
        dist.all_reduce(one)
        assert float(one.item()) == 1.0
        rng = np.random.default_rng(0)
        g, w = torch.as_tensor(rng.normal(size=(4096, 12)), device=dev), torch.as_tensor(rng.normal(size=4096), device=dev)
        s_, ws, n = allreduce_weighted_grad(g, w)
        assert torch.allclose(s_, (w[:, None] * g).sum(0), rtol=1e-11, atol=1e-11) and int(round(float(n))) == 4096
        v = (torch.arange(4096, device=dev) % 3 != 0).to(torch.float64)
        assert torch.allclose(mean_update(g, w, valid=v), ((w * v)[:, None] * g).sum(0) / v.sum(), rtol=1e-11, atol=1e-13)
        E = 256
        env = BatchedCartPoleSwingUpEnv(E, device=dev, seed=0)
        agent = BatchedTD3(cartpole_ocp(), env, batch_size=E, buffer_steps=8, policy_delay=1, lr_actor=1e-6, seed=0, device=dev)
        w0 = [p.detach().clone() for p in agent.critic.parameters()]
        agent.collect(2)
        tr = agent.train(1)
        torch.cuda.synchronize()
        # (the swing-up start states saturate u0, where du0*/dtheta = 0: the theta step itself may be exactly zero here)
        assert np.isfinite(tr["critic_loss"]) and bool(torch.isfinite(agent.theta).all()) and np.isfinite(tr["theta_step_norm"])
        assert any(float((p.detach() - q).abs().max()) > 0.0 for p, q in zip(agent.critic.parameters(), w0))     # the all-reduced gradient arrived
    finally:
        dist.destroy_process_group()


def test_divergence_exit_rule(oracle_port, monkeypatch):
    """mpcrl_set_exit_rule (opt-in; the reference has no such exit: full-step SQP to nlp_solver_max_iter, config/cartpole.yaml:12-14):
    on 2048 states from the whole state box at max_iter = 500 the rule (window 10, factor 0.1) ends the non-converging instances
    early with status 2, the same instances the oracle port ends under the same rule; every instance that still converges returns
    bit for bit what it returns with the rule off; the plain and the time-sliced launch agree bit for bit under the rule."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    from oracle.problems import make_cartpole
    rng = np.random.default_rng(7)
    B = 2048
    x0 = rng.uniform(-1, 1, (B, 4)) * np.array([2.0, 3.0, np.pi, 5.0])
    xt = torch.as_tensor(x0, device="cuda")
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCRL_TIME_SLICE", mode)
        off = MPCBatch(cartpole_ocp(max_iter=500), B)
        r0 = off.solve(xt, sens_v=True, sens_pi=True, cold=True)
        on = MPCBatch(cartpole_ocp(max_iter=500), B)
        on.set_exit_rule(10, 0.1)
        r1 = on.solve(xt, sens_v=True, sens_pi=True, cold=True)
        out[mode] = (r0, r1)
    (r0, r1), (s0, s1) = out["0"], out["1"]
    for a, b in ((r0, s0), (r1, s1)):
        for t1, t2 in ((a.u0, b.u0), (a.V, b.V), (a.status, b.status), (a.iters, b.iters), (a.dV_dp, b.dV_dp)):
            assert torch.equal(t1, t2)
    st0, st1 = r0.status.cpu().numpy(), r1.status.cpu().numpy()
    it0, it1 = r0.iters.cpu().numpy(), r1.iters.cpu().numpy()
    assert it0[:, 0].max() == 500 and it1[:, 0].max() <= 120, (it0[:, 0].max(), it1[:, 0].max())
    conv1 = st1 == 0
    assert np.all(st0[conv1] == 0) and conv1.sum() >= 0.9 * (st0 == 0).sum()      # nothing converges only BECAUSE of the rule; few are lost
    for a, b in ((r0.u0, r1.u0), (r0.V, r1.V), (r0.dV_dp, r1.dV_dp), (r0.dpi_dp, r1.dpi_dp), (r0.iters, r1.iters)):
        a, b = a.cpu().numpy()[conv1], b.cpu().numpy()[conv1]
        assert np.array_equal(a, b, equal_nan=True)
    ref = oracle_port.solve(make_cartpole(), x0, max_iter=500, exit_window=10, exit_factor=0.1)
    same = st1 == ref.status
    ok = conv1 & (ref.status == 0)
    print(f"exit rule: converged off {(st0 == 0).mean():.4f} on {conv1.mean():.4f} (port {(ref.status == 0).mean():.4f}), status equal to port "
          f"{same.mean():.4f}, SQP iterations max off {it0[:, 0].max()} on {it1[:, 0].max()} (port {ref.sqp_iter.max()}), "
          f"sum off {it0[:, 0].sum()} on {it1[:, 0].sum()}")
    assert same.mean() > 0.99 and (it1[ok, 0] == ref.sqp_iter[ok]).mean() > 0.97
    assert rel_rows(r1.u0.cpu().numpy()[ok], ref.u0[ok]).max() < RTOL and rel_rows(r1.V.cpu().numpy()[ok], ref.V[ok]).max() < RTOL
    # misuse
    assert on.lib.mpcrl_set_exit_rule(on._h, 300, 0.1) < 0 and on.lib.mpcrl_set_exit_rule(on._h, 10, 0.0) < 0


def test_divergence_exit_rule_chain(oracle_port):
    """mpcrl_set_exit_rule on the chain of masses (ABI 110; each instance has a wavefront — a SIMD — to itself, so a diverging one holds
    it for max_iter rounds): 64 instances of n_mass 5 whose velocities / positions are perturbed by N(0, 2) / N(0, 0.05), a few of which
    full-step SQP does not solve.  Under (window 5, factor 0.5): the same statuses as the port under the same rule, nobody iterates to
    max_iter any more, and every instance that still converges returns bit for bit what it returns with the rule off."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp, P = chain_mass_ocp(n_mass=5), make_chain_mass(n_mass=5)
    rng = np.random.default_rng(2)
    B = 64
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 12:] += rng.normal(0.0, 2.0, (B, 9))
    x0[:, :12] += rng.normal(0.0, 0.05, (B, 12))
    off = MPCBatch(ocp, B)
    r0 = off.solve(x0, sens_v=True, sens_pi=True, cold=True)
    on = MPCBatch(ocp, B)
    on.set_exit_rule(5, 0.5)
    r1 = on.solve(x0, sens_v=True, sens_pi=True, cold=True)
    st0, st1 = r0.status.cpu().numpy(), r1.status.cpu().numpy()
    it0, it1 = r0.iters.cpu().numpy(), r1.iters.cpu().numpy()
    ref0 = oracle_port.solve(P, x0)
    ref1 = oracle_port.solve(P, x0, exit_window=5, exit_factor=0.5)
    print(f"chain exit rule: statuses off {np.bincount(st0, minlength=5)} on {np.bincount(st1, minlength=5)} (port {np.bincount(ref1.status, minlength=5)}), "
          f"SQP iterations max off {it0[:, 0].max()} on {it1[:, 0].max()} (port {ref1.sqp_iter.max()})")
    assert (st0 == 2).sum() >= 1 and it0[:, 0].max() == 50                       # the inputs do contain instances that run to max_iter
    assert np.array_equal(st0, ref0.status) and np.array_equal(st1, ref1.status)
    assert it1[:, 0].max() < 50 and np.abs(it1[:, 0] - ref1.sqp_iter).max() <= 1
    conv1 = st1 == 0
    assert np.all(st0[conv1] == 0) and conv1.sum() >= (st0 == 0).sum() - 2
    for a, b in ((r0.u0, r1.u0), (r0.V, r1.V), (r0.dV_dp, r1.dV_dp), (r0.dpi_dp, r1.dpi_dp), (r0.iters, r1.iters)):
        assert np.array_equal(a.cpu().numpy()[conv1], b.cpu().numpy()[conv1], equal_nan=True)
    assert rel_rows(r1.u0.cpu().numpy()[conv1], ref1.u0[conv1]).max() < RTOL and rel_rows(r1.V.cpu().numpy()[conv1], ref1.V[conv1]).max() < RTOL


@pytest.mark.gpu
def test_launch_shape_tuner(monkeypatch):
    """mpcrl_set_launch_mode(0) (the default): a handle whose batch size makes the time-sliced launch a candidate (4096 cartpole
    instances: one round of 4-instance wavefronts instead of two of 3-instance ones) probes both shapes on its own cold solves —
    calls 1 and 2 of every 64 — and reads the times back without waiting.  The shapes return the same bits, so every call of the
    sequence must return what the first one did, whatever shape it ran in; after the probes both times are known and the handle's
    promise (mpcrl_query_time_sliced) is the shape the times prefer.  Forced modes override the tuner."""
    monkeypatch.delenv("MPCRL_TIME_SLICE", raising=False)
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    from mpc4rl_amd import _lib
    B = 4096
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(B, 4, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    x[:, 1] += 3.14159
    x = x.cuda()
    mpc = MPCBatch(cartpole_ocp(), B)
    assert mpc.launch_times()[:2] == (-1.0, -1.0)
    first = mpc.solve(x, cold=True, sens_pi=True)
    shapes = []
    for _ in range(5):
        shapes.append(mpc.lib.mpcrl_query_time_sliced(mpc._h, _lib.COLD | _lib.SENS_PI, None))
        r = mpc.solve(x, cold=True, sens_pi=True)
        torch.cuda.synchronize()
        assert torch.equal(r.u0, first.u0) and torch.equal(r.V, first.V) and torch.equal(r.iters, first.iters)
        assert torch.equal(torch.nan_to_num(r.dpi_dp), torch.nan_to_num(first.dpi_dp))
    assert shapes[0] == 1 and shapes[1] == 0                       # the probes: call 1 time-sliced, call 2 plain
    ts, tp, pref = mpc.launch_times()
    assert ts > 0.0 and tp > 0.0 and pref == ("plain" if tp < 0.80 * ts else "time-sliced")
    assert all(s == (0 if pref == "plain" else 1) for s in shapes[3:])
    # warm calls are probed on their own (different work per instance): their first probe is still ahead
    assert mpc.launch_times(warm=True)[:2] == (-1.0, -1.0) and mpc.lib.mpcrl_query_time_sliced(mpc._h, _lib.SENS_PI, None) == 1
    w0 = mpc.solve(x, sens_pi=True)
    for _ in range(4):
        w = mpc.solve(x, sens_pi=True)
        torch.cuda.synchronize()
        assert torch.equal(w.u0, w0.u0) and torch.equal(w.V, w0.V)
    tws, twp, _ = mpc.launch_times(warm=True)
    assert tws > 0.0 and twp > 0.0 and (tws, twp) != (ts, tp)
    mpc.set_launch_mode(-1)
    assert mpc.lib.mpcrl_query_time_sliced(mpc._h, _lib.COLD, None) == 0
    mpc.set_launch_mode(1)
    assert mpc.lib.mpcrl_query_time_sliced(mpc._h, _lib.COLD, None) == 1
    r = mpc.solve(x, cold=True, sens_pi=True)
    assert torch.equal(r.u0, first.u0) and torch.equal(r.iters, first.iters)
    assert mpc.lib.mpcrl_set_launch_mode(mpc._h, 2) < 0
    # a batch the static rule already gives to the plain launch is never probed
    small = MPCBatch(cartpole_ocp(), 96)
    for _ in range(4):
        small.solve(x[:96], cold=True)
    torch.cuda.synchronize()
    assert small.launch_times()[:2] == (-1.0, -1.0)


def test_exact_qp_mode_on_the_device_bench_inputs(oracle_port):
    """SURVEY §7 hard-part 4 on the PRODUCT (round 6; until now shown on the CPU port only, tests/test_exact_vs_inexact.py): the
    reference solves every QP to HPIPM's tolerance (config/cartpole.yaml:8-14, mpc.py:42); the shipped kernels run an inexact-SQP /
    warm-started interior-point iteration.  MPCRL_EXACT_QP (test-only flag, a separate instantiation of the plain solve kernel:
    forcing term off, cold interior-point starts, fixed fraction to the boundary, no predictor-only steps) runs the 4096 benchmark
    inputs the exact way ON THE DEVICE: (a) the shipped iteration returns the same u0*, V, dV/dp, du0*/dp at 1e-6, every instance;
    (b) the exact device mode is the port's frozen ORACLE_EXACT mode: statuses, iteration counts, outputs."""
    import bench
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    from oracle.problems import make_cartpole
    x0 = bench.make_inputs(4096, 0)
    xt = torch.as_tensor(x0, device="cuda")
    mpc = MPCBatch(cartpole_ocp(), 4096)
    a = mpc.solve(xt, sens_v=True, sens_pi=True, cold=True)
    e = mpc.solve(xt, sens_v=True, sens_pi=True, cold=True, exact_qp=True)
    torch.cuda.synchronize()
    assert bool((a.status == 0).all()) and bool((e.status == 0).all())
    for name in ("u0", "V", "dV_dp", "dpi_dp"):
        err = rel_rows(getattr(a, name).cpu().numpy(), getattr(e, name).cpu().numpy())
        print("shipped vs exact-QP on the device:", name, float(err.max()))
        assert err.max() < RTOL, (name, float(err.max()))
    ia, ie = a.iters.cpu().numpy(), e.iters.cpu().numpy()
    print("iterations shipped / exact: sqp %.2f / %.2f, interior point %.2f / %.2f" % (ia[:, 0].mean(), ie[:, 0].mean(), ia[:, 1].mean(), ie[:, 1].mean()))
    assert abs(ia[:, 0].mean() - ie[:, 0].mean()) < 0.5 and ia[:, 1].mean() < 0.5 * ie[:, 1].mean()
    ref = oracle_port.solve(make_cartpole(), x0, exact=True)
    compare(e, ref, 1.0, name="exact-QP mode, device vs port")
    with pytest.raises(RuntimeError):       # the flag is refused where it has no meaning: a real-time iteration
        mpc.solve(xt, rti=True, exact_qp=True)


@pytest.mark.parametrize("n_mass", [5, 7])
def test_exact_qp_mode_on_the_device_chain_bench_inputs(oracle_port, n_mass):
    """The same for BASELINE config 4 (chain of masses, the 1024 bench inputs of each size): the reference solves every QP to HPIPM's
    tolerance (chain_mass/ocp_utils.py:308-312: SQP, tol 1e-5), the shipped kernel runs an inexact-SQP iteration with an interior point
    warm-started across QPs.  MPCRL_EXACT_QP (a wave-uniform switch at the SQP level: forcing term off, cold interior-point starts,
    fixed fraction to the boundary) on the device: the shipped iteration returns the exact mode's u0*, V, dV/dp, du0*/dp at 1e-6 on
    every instance, and the exact device mode is the port's frozen ORACLE_EXACT mode (64 instances: statuses, iteration counts)."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.problems import make_chain_mass
    # (at the reference's tol = 1e-5 two iterations that both stop within tol of the KKT point are ~1e-6 apart — measured 7.5e-7 on u0*,
    # 1.8e-6 on dV/dp, and still 2.2e-6 on dV/dp at tol 1e-8: dV/dp is as good as the multipliers —: the two ITERATIONS are compared
    # at the KKT point, tol 1e-9.  There the exact mode's complementarity residual stalls at 1.4e-9 ... 1.9e-9 on ~8 % of the batch
    # (status 2 at max_iter, on the device and in the port alike): the comparison is on the instances both modes solve, >= 90 %)
    ocp = chain_mass_ocp(n_mass=n_mass, tol=1e-9)
    B, M = 1024, n_mass - 2
    rng = np.random.default_rng(0)
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 3 * (M + 1):] += rng.normal(0.0, 1e-2, (B, 3 * M))
    xt = torch.as_tensor(x0, device="cuda")
    mpc = MPCBatch(ocp, B)
    def margin():      # strict-complementarity margin of the stored iterate: min over the control-bound rows of max(lam, t)
        b = mpc.get_iterate()[3].cpu().numpy()
        return np.maximum(b[:, 0:2, :-1, :3], b[:, 2:4, :-1, :3]).reshape(B, -1).min(1)
    a = mpc.solve(xt, sens_v=True, sens_pi=True, cold=True)
    m_a = margin()
    e = mpc.solve(xt, sens_v=True, sens_pi=True, cold=True, exact_qp=True)
    m_e = margin()
    torch.cuda.synchronize()
    both = ((a.status == 0) & (e.status == 0)).cpu().numpy()
    assert bool((a.status == 0).all()) and both.mean() > 0.9 and set(np.unique(e.status.cpu().numpy())) <= {0, 2}
    # du0*/dp is a property of the KKT POINT only where strict complementarity holds; where a control bound is weakly active (lam and t
    # both small) the barrier diagonal lam / t of the final interior-point iterate is whatever the path left, and the two modes differ
    # (1.4e-3 at a margin of 1.7e-4, 1.4e-5 at 1e-3; 6e-7 from 1e-2 on): the 1e-6 bar is on the strictly complementary instances
    strict = both & (np.minimum(m_a, m_e) > 1e-2)
    assert strict.mean() > 0.6
    for name in ("u0", "V", "dV_dp", "dpi_dp"):
        sel = strict if name == "dpi_dp" else both
        err = rel_rows(getattr(a, name).cpu().numpy()[sel], getattr(e, name).cpu().numpy()[sel])
        print("chain n_mass %d, shipped vs exact-QP on the device (%d instances):" % (n_mass, sel.sum()), name, float(err.max()))
        # u0*, V, du0*/dp at 1e-6.  dV/dp at 1e-5: both iterates satisfy the KKT residuals to 1e-9 and still differ by 4e-8 in x, u and 5e-7
        # in the multipliers (the conditioning of this KKT system), which dV/dp = dL/dp carries with |dF/dp| ~ 1e2: measured 2.2e-6
        assert err.max() < (1e-5 if name == "dV_dp" else RTOL), (name, float(err.max()))
    ia, ie = a.iters.cpu().numpy()[both], e.iters.cpu().numpy()[both]
    print("iterations shipped / exact: sqp %.2f / %.2f, interior point %.2f / %.2f" % (ia[:, 0].mean(), ie[:, 0].mean(), ia[:, 1].mean(), ie[:, 1].mean()))
    assert abs(ia[:, 0].mean() - ie[:, 0].mean()) < 1.0 and ia[:, 1].mean() < ie[:, 1].mean()
    n = 64
    ref = oracle_port.solve(make_chain_mass(n_mass=n_mass), x0[:n], exact=True, tol=1e-9)
    st, it = e.status.cpu().numpy()[:n], e.iters.cpu().numpy()[:n]
    assert (st == ref.status).mean() > 0.95                                    # (an instance whose residual sits at the stall can end either way)
    okb = (st == 0) & (ref.status == 0)
    assert np.abs(it[okb, 0] - ref.sqp_iter[okb]).max() <= 1 and (it[okb, 1] == ref.ipm_iter[okb]).mean() > 0.9
    for name, mine, theirs in (("u0", e.u0, ref.u0), ("V", e.V, ref.V), ("dV", e.dV_dp, ref.dV), ("dpi", e.dpi_dp, ref.dpi)):
        assert rel_rows(mine.cpu().numpy()[:n][okb], theirs[okb]).max() < RTOL, name      # (the same iteration on both sides: 1e-6 throughout)


def test_exact_qp_flag_linear_system():
    """The linear-system kernel accepts the flag (its QP is tight and its fraction to the boundary fixed anyway: the flag only takes the
    interior-point warm start of a warm call away): cold calls are bit-identical with and without it; the one-stage kernels refuse it."""
    from mpc4rl_amd import MPCBatch, linear_system_ocp
    rng = np.random.default_rng(3)
    x0 = np.column_stack([rng.uniform(0.15, 0.85, 256), rng.uniform(-0.5, 0.5, 256)])
    lin = MPCBatch(linear_system_ocp(), 256)
    a = lin.solve(x0, sens_v=True, sens_pi=True, cold=True)
    e = lin.solve(x0, sens_v=True, sens_pi=True, cold=True, exact_qp=True)
    for n in ("u0", "V", "dV_dp", "dpi_dp", "status", "iters"):
        assert torch.equal(getattr(a, n), getattr(e, n)), n
    w = lin.solve(x0 + 0.01, exact_qp=True)                # a warm call in exact mode: the same answers as a cold one
    c = MPCBatch(linear_system_ocp(), 256).solve(x0 + 0.01, cold=True)
    assert bool((w.status == 0).all()) and float((w.u0 - c.u0).abs().max()) < 1e-6 and float((w.V - c.V).abs().max()) < 1e-6


def test_no_bnd_store_linear():
    """MPCRL_NO_BND_STORE (round 6): same outputs bit for bit, the bound planes of the stored iterate untouched, x / u / pi stored,
    and the next solve starts its interior point from the default point — exactly what a set_iterate(x, u, pi, bnd=None) does."""
    from mpc4rl_amd import MPCBatch, linear_system_ocp
    rng = np.random.default_rng(5)
    B = 512
    x0 = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.5, 0.5, B)])
    x1 = x0 + rng.uniform(-0.02, 0.02, x0.shape)
    A, Bm = MPCBatch(linear_system_ocp(discount_factor=0.99), B), MPCBatch(linear_system_ocp(discount_factor=0.99), B)
    bnd_before = A.get_iterate()[3].clone()
    ra = A.solve(x0, sens_v=True, sens_pi=True, cold=True, store_bounds=False)
    rb = Bm.solve(x0, sens_v=True, sens_pi=True, cold=True)
    for n in ("u0", "V", "dV_dp", "dpi_dp", "status", "iters"):
        assert torch.equal(getattr(ra, n), getattr(rb, n)), n
    xa, ua, pa, bnda, _ = A.get_iterate()
    xb, ub, pb, bndb, _ = Bm.get_iterate()
    assert torch.equal(xa, xb) and torch.equal(ua, ub) and torch.equal(pa, pb)
    assert torch.equal(bnda, bnd_before) and not torch.equal(bndb, bnd_before)
    assert not A.duals_valid and Bm.duals_valid
    Bm.set_iterate(xb, ub, pb, None)                   # primal / costate guess only: MPCRL_COLD_DUAL on the next solve
    ra2, rb2 = A.solve(x1, sens_v=True, sens_pi=True), Bm.solve(x1, sens_v=True, sens_pi=True)
    for n in ("u0", "V", "dV_dp", "dpi_dp", "status", "iters"):
        assert torch.equal(getattr(ra2, n), getattr(rb2, n)), n
    assert A.duals_valid


def test_two_rccl_ranks_on_the_one_gpu():
    """the only piece of the N > 1 path that never ran with RCCL and more than one rank (no multi-GPU node so
    far).  bench.py --gpus 2 with both ranks on cuda:0 (MPCRL_BENCH_SHARE_GPU), 512 chain instances each: the line must report
    rccl_ranks == 2.  RCCL may refuse two ranks on one device ("Duplicate GPU detected"); then the refusal is what gets recorded
    (gpurun_out/r06_rccl_two_ranks_one_gpu.txt, copied to profiles/) and the test asserts that it is THAT error and nothing else."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"MPCRL_BENCH_SHARE_GPU": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "NCCL_DEBUG": "WARN"})
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "chain5", "--batch", "512", "--steps", "3",
                          "--warmup", "1", "--no-cpu"], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    rec = os.path.join(root, "gpurun_out", "r06_rccl_two_ranks_one_gpu.txt")
    if out.returncode == 0 and lines:
        line = json.loads(lines[0])
        with open(rec, "w") as fh:
            fh.write("bench.py --gpus 2 --workload chain5 --batch 512, both ranks on cuda:0 (MPCRL_BENCH_SHARE_GPU=1):\n" + lines[0] + "\n")
        assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2, line
        assert "one all-reduce" in line["config"]["parallelism"]
    else:
        text = out.stderr + out.stdout
        keep = [ln for ln in text.splitlines() if "alt_rsmi" not in ln and
                any(w in ln for w in ("Duplicate GPU", "NCCL", "RCCL", "invalid usage", "ncclInvalidUsage", "Error", "error"))]
        with open(rec, "w") as fh:
            fh.write("bench.py --gpus 2 with both ranks on cuda:0 (MPCRL_BENCH_SHARE_GPU=1): RCCL refused, rc %d\n" % out.returncode + "\n".join(keep[-40:]) + "\n")
        print("\n".join(keep[-12:]))
        assert any(("Duplicate GPU" in ln) or ("invalid usage" in ln) or ("ncclInvalidUsage" in ln) for ln in keep), text[-3000:]


def test_plain_bench_run_dumps_reproducible_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: exactly K timed steps, the headline line without the --full
    extras, and the last step's outputs on disk — bit for bit the same in a second run on the same seeded inputs."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--dump-outputs", str(tmp_path / d)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, out.stdout
        lines.append(json.loads(js[0]))
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0.0 and line["dtype"] == "f64"
    assert not {"secondary", "steady_state", "cpu_baseline"} & set(line) and "peak_measured" not in line["roofline"]
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["V.npy", "dV_dp.npy", "dpi_dp.npy", "iters.npy", "status.npy", "u0.npy"]
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and a.shape[0] == 4096 and np.array_equal(a, b, equal_nan=True), n
    assert np.all(np.load(tmp_path / "a" / "status.npy") == 0)
