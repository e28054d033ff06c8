"""GPU parity: the HIP path (through the C ABI) against the CPU oracle port on the same seeded inputs.

Tolerances: the engine and the oracle run the same iteration in fp64, so iterates agree to ~1e-10; the bar
from BASELINE.json's north_star is 1e-6 relative on u0*, V, dV/dp, du0*/dp and that is what is asserted
(tighter values are printed)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def rel_err(a, b, floor=1.0):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def cartpole_x0(B, seed=0):
    """BASELINE config 2/3 inputs: theta ~ U(0.9 pi, 1.1 pi), rest 0 (continuous_cartpole/environment.py:178-180)
    for the first half, near-upright states (non-saturated u0, non-trivial du0/dp) for the second half."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 4))
    h = B // 2
    x0[:h, 2] = rng.uniform(0.9 * np.pi, 1.1 * np.pi, h)
    x0[h:] = rng.uniform(-1, 1, (B - h, 4)) * np.array([0.5, 1.0, 0.3, 1.0])
    return x0


def run_both(ocp, P, oracle_port, x0, u0=None, theta=None, **kw):
    from mpc4rl_amd import MPCBatch
    B = x0.shape[0]
    mpc = MPCBatch(ocp, B)
    if theta is not None:
        mpc.set_theta(torch.as_tensor(theta))
    r = mpc.solve(x0, u0, sens_v=True, sens_pi=True, cold=True)
    torch.cuda.synchronize()
    ref = oracle_port.solve(P, x0, p=theta, u0fix=u0, **kw)
    return mpc, r, ref


def check(r, ref, need_strict=None):
    st = r.status.cpu().numpy()
    assert np.array_equal(st, ref.status), (st, ref.status)
    ok = st == 0
    assert ok.mean() > 0.9
    it = r.iters.cpu().numpy()
    # the same iteration in two arithmetic orders: counts agree except where a stopping test is met to within rounding
    assert np.abs(it[ok, 0] - ref.sqp_iter[ok]).max() <= 1 and (it[ok, 0] == ref.sqp_iter[ok]).mean() > 0.97
    errs = {
        "u0": rel_err(r.u0.cpu().numpy()[ok], ref.u0[ok]),
        "V": rel_err(r.V.cpu().numpy()[ok], ref.V[ok]),
        "dV": rel_err(r.dV_dp.cpu().numpy()[ok], ref.dV[ok]),
    }
    sel = ok if need_strict is None else ok & need_strict
    errs["dpi"] = rel_err(r.dpi_dp.cpu().numpy()[sel], ref.dpi[sel])
    print(errs, "ipm iters equal:", np.array_equal(it[ok, 1], ref.ipm_iter[ok]))
    for k, v in errs.items():
        assert v < RTOL, (k, v)
    return errs


def test_cartpole_solve_and_sens_vs_oracle(oracle_port):
    from mpc4rl_amd import cartpole_ocp
    from oracle.problems import make_cartpole
    x0 = cartpole_x0(256)
    mpc, r, ref = run_both(cartpole_ocp(), make_cartpole(), oracle_port, x0)
    check(r, ref)
    x, u, pi, bnd, res = [t.cpu().numpy() for t in mpc.get_iterate()]
    ok = ref.status == 0
    assert rel_err(x[ok], ref.X[ok]) < RTOL and rel_err(u[ok], ref.U[ok]) < RTOL and rel_err(pi[ok], ref.PI[ok]) < RTOL
    assert np.all(res[ok] < 1e-6)          # assert_kkt_residual, nlp.py:1295-1299


def test_cartpole_q_mode_vs_oracle(oracle_port):
    from mpc4rl_amd import cartpole_ocp
    from oracle.problems import make_cartpole
    B = 64
    rng = np.random.default_rng(1)
    x0 = cartpole_x0(B, 1)
    u0 = rng.uniform(-30, 30, (B, 1))
    u0[0] = -30.0                          # scripts/cartpole_mpc_sensitivities.py:80-81
    x0[0] = [0.0, 0.0, np.pi / 2, 0.0]
    _, r, ref = run_both(cartpole_ocp(), make_cartpole(), oracle_port, x0, u0)
    check(r, ref)
    assert np.allclose(r.u0.cpu().numpy(), u0)
    assert np.all(r.dpi_dp.cpu().numpy() == 0.0)


def test_cartpole_per_instance_theta(oracle_port):
    from mpc4rl_amd import cartpole_ocp
    from oracle.problems import make_cartpole
    B = 96
    P = make_cartpole()
    rng = np.random.default_rng(2)
    theta = np.tile(P.p0, (B, 1))
    theta[:, :3] *= rng.uniform(0.9, 1.1, (B, 3))
    _, r, ref = run_both(cartpole_ocp(), P, oracle_port, cartpole_x0(B, 2), theta=theta)
    check(r, ref)


def test_linear_system_vs_oracle(oracle_port):
    from mpc4rl_amd import linear_system_ocp
    from oracle.problems import make_linear_system
    B = 64
    rng = np.random.default_rng(3)
    x0 = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.5, 0.5, B)])
    x0[0] = [0.5, 0.5]                     # linear_system/environment.py:46
    x0[1] = [0.2, 0.2]                     # scripts/linear_system_mpc_nlp.py:18
    for gamma in (0.99, 0.9):
        _, r, ref = run_both(linear_system_ocp(discount_factor=gamma), make_linear_system(gamma=gamma), oracle_port, x0)
        # du0/dp is ill-defined where a soft bound is active (quirk q1, LICQ fails): compare where slacks are 0
        s = np.abs(ref.BND[:, 4:6]).reshape(B, -1).max(axis=1)
        check(r, ref, need_strict=s < 1e-9)


def test_linear_system_q_mode(oracle_port):
    from mpc4rl_amd import linear_system_ocp
    from oracle.problems import make_linear_system
    x0 = np.tile([0.2, 0.2], (8, 1))
    u0 = np.linspace(-0.9, 0.9, 8).reshape(8, 1)
    u0[0] = -0.5                           # scripts/linear_system_mpc_nlp.py:18
    _, r, ref = run_both(linear_system_ocp(), make_linear_system(), oracle_port, x0, u0)
    check(r, ref)


def test_chain_mass_sweep_vs_oracle(oracle_port):
    """The harness of the reference's tests/test_chain_mass.py (rlmpc/examples/chain_mass.py:133-174): C_3_0 swept over
    [0.5, 1.5] x nominal in 10 points, x0 = masses equally spaced on the x axis; u0* and du0*/dp per point — here the
    ten points are ONE batched call with per-instance parameters."""
    from mpc4rl_amd import chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp, P = chain_mass_ocp(), make_chain_mass()
    p_idx = ocp.p_labels.index("C_3_0")
    vals = np.linspace(0.5 * ocp.p0[p_idx], 1.5 * ocp.p0[p_idx], 10)
    theta = np.tile(ocp.p0, (10, 1))
    theta[:, p_idx] = vals
    x0 = np.tile(ocp.x0, (10, 1))
    _, r, ref = run_both(ocp, P, oracle_port, x0, theta=theta)
    st = r.status.cpu().numpy()
    assert np.all(st == 0) and np.array_equal(st, ref.status)
    assert np.abs(r.iters.cpu().numpy()[:, 0] - ref.sqp_iter).max() <= 1
    assert rel_err(r.u0.cpu().numpy(), ref.u0) < RTOL and rel_err(r.V.cpu().numpy(), ref.V) < RTOL
    assert rel_err(r.dV_dp.cpu().numpy(), ref.dV) < RTOL
    dpi, dref = r.dpi_dp.cpu().numpy(), ref.dpi
    assert rel_err(dpi, dref, floor=np.abs(dref).max()) < RTOL
    assert rel_err(dpi[:, :, p_idx], dref[:, :, p_idx], floor=np.abs(dref[:, :, p_idx]).max()) < RTOL   # the swept column
    # first-order consistency of the sweep (what the reference's plot_results shows): FD of u0* along the sweep vs du0*/dp
    fd = np.gradient(r.u0.cpu().numpy(), vals, axis=0)
    assert np.abs(fd[1:-1] - dpi[1:-1, :, p_idx]).max() < 5e-3 * max(1.0, np.abs(dpi[:, :, p_idx]).max())


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_chain_mass_vs_golden():
    """G4 (all ten sweep points, n_mass = 5) and G5 (n_mass = 7, nx = 33): the tuned HIP path against vectors the dense oracle
    produced in its frozen exact-QP mode (tests/golden/make_golden.py)."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    g = np.load(os.path.join(GOLD, "g4_chain5.npz"))
    ocp = chain_mass_ocp()
    assert len(g["p_vals"]) == 10
    theta = np.tile(ocp.p0, (len(g["p_vals"]), 1))
    theta[:, int(g["p_idx"])] = g["p_vals"]
    # at the golden's NLP tolerance (1e-8) the north_star bar 1e-6; at the chain's default tolerance 1e-5 (ocp_utils.py:311-312) a run
    # is itself only within ~1e-5 x conditioning of the KKT point (tests/test_oracle.py::test_port_vs_golden_chain)
    for tol, bar in ((1e-8, RTOL), (None, 2e-5)):
        mpc = MPCBatch(chain_mass_ocp() if tol is None else chain_mass_ocp(tol=tol), len(theta))
        mpc.set_theta(torch.as_tensor(theta))
        r = mpc.solve(g["x0"], sens_v=True, sens_pi=True, cold=True)
        assert np.all(r.status.cpu().numpy() == 0)
        assert rel_err(r.u0.cpu().numpy(), g["u0"]) < bar and rel_err(r.V.cpu().numpy(), g["V"]) < RTOL
        assert rel_err(r.dV_dp.cpu().numpy(), g["dV"]) < bar
        assert rel_err(r.dpi_dp.cpu().numpy(), g["dpi"], floor=np.abs(g["dpi"]).max()) < bar
        assert float((mpc.get_lagrangian() - r.V).abs().max()) < 1e-5   # lam'h + pi'g vanish at a KKT point up to the barrier parameter
    g = np.load(os.path.join(GOLD, "g5_chain7.npz"))
    for tol, bar in ((1e-8, RTOL), (None, 2e-5)):
        mpc = MPCBatch(chain_mass_ocp(n_mass=7) if tol is None else chain_mass_ocp(n_mass=7, tol=tol), len(g["x0"]))
        r = mpc.solve(g["x0"], sens_v=True, sens_pi=True, cold=True)
        assert np.all(r.status.cpu().numpy() == 0)
        assert rel_err(r.u0.cpu().numpy(), g["u0"]) < bar and rel_err(r.V.cpu().numpy(), g["V"]) < RTOL
        assert rel_err(r.dV_dp.cpu().numpy(), g["dV"]) < bar
        assert rel_err(r.dpi_dp.cpu().numpy(), g["dpi"], floor=np.abs(g["dpi"]).max()) < bar


def test_golden_cartpole_and_linear_on_gpu():
    """HIP path (tuned inexact SQP) against the committed golden vectors (dense Python oracle in its frozen exact-QP mode +
    autograd mirror): G3 = 64 reset-distribution states + 64 near-upright states, each at theta x {1, 0.9, 1.1}."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp, linear_system_ocp
    g = np.load(os.path.join(GOLD, "g3_cartpole.npz"))
    ocp = cartpole_ocp()
    B = len(g["x0"])
    assert B == 384
    theta = np.tile(ocp.p0, (B, 1))
    theta[:, :3] = g["theta_model"]
    strict = g["sc"] >= 1e-3          # strict-complementarity filter of SURVEY.md §8c (see tests/test_oracle.py::check_against_kkt_golden)

    def per_instance(a, b):
        a, b = np.asarray(a, float).reshape(B, -1), np.asarray(b, float).reshape(B, -1)
        return (np.abs(a - b) / np.maximum(np.abs(b).max(1, keepdims=True), 1.0)).max(1)

    for tol in (1e-8, None):          # the golden's own NLP tolerance, then the solver default 1e-6 (the reference's setting)
        mpc = MPCBatch(cartpole_ocp() if tol is None else cartpole_ocp(tol=tol), B)
        mpc.set_theta(torch.as_tensor(theta))
        r = mpc.solve(g["x0"], sens_v=True, sens_pi=True, cold=True)
        assert np.all(r.status.cpu().numpy() == 0)
        e = {k: per_instance(a.cpu().numpy(), g[k]) for k, a in (("u0", r.u0), ("V", r.V), ("dV", r.dV_dp), ("dpi", r.dpi_dp))}
        print("tol", tol, {k: (float(v.max()), float((v < RTOL).mean())) for k, v in e.items()})
        assert e["V"].max() < RTOL and e["dV"].max() < RTOL and e["dpi"].max() < 2e-5
        if tol is not None:           # both at the KKT point: the north_star bar on every instance
            assert e["u0"].max() < RTOL and e["dpi"][strict].max() < RTOL
        else:                         # a run stopped at 1e-6 is itself only within ~1e-6 x conditioning of the KKT point
            assert e["u0"].max() < 1e-5 and (e["u0"] < RTOL).mean() >= 0.99 and (e["dpi"][strict] < RTOL).mean() >= 0.99
        assert rel_err(mpc.get_lagrangian().cpu().numpy(), g["L"]) < RTOL
        x, u, pi, _, _ = mpc.get_iterate()
        assert rel_err(x[:12].cpu().numpy(), g["X"]) < 1e-5 and rel_err(u[:12].cpu().numpy(), g["U"]) < 1e-5
        assert rel_err(pi[:12].cpu().numpy(), g["PI"]) < 1e-5
    mq = MPCBatch(ocp, 1)
    rq = mq.solve(g["q_x0"], g["q_u0fix"], sens_v=True, sens_pi=True, cold=True)   # scripts/cartpole_mpc_sensitivities.py:80-81
    assert int(rq.status[0]) == 0 and rel_err(rq.V.cpu().numpy(), g["q_V"]) < RTOL and rel_err(rq.dV_dp.cpu().numpy(), g["q_dV"]) < RTOL
    for tag in ("g099", "g09"):
        g = np.load(os.path.join(GOLD, f"g2_linear_{tag}.npz"))
        mpc = MPCBatch(linear_system_ocp(discount_factor=float(g["gamma"])), len(g["x0"]))
        r = mpc.solve(g["x0"], sens_v=True, sens_pi=True, cold=True)
        assert np.all(r.status.cpu().numpy() == 0)
        strict = g["smax"] < 1e-9
        for k, a in (("u0", r.u0), ("V", r.V), ("dV", r.dV_dp)):
            assert rel_err(a.cpu().numpy(), g[k]) < RTOL, k
        assert rel_err(r.dpi_dp.cpu().numpy()[strict], g["dpi"][strict]) < RTOL


def test_hip_vs_third_party_solver():
    """G6 (tests/golden/make_thirdparty.py): u0* and V of KKT points found and certified by scipy.optimize (SLSQP on the cartpole
    NLP from the cold iterate, trust-constr on the linear-system QP) — a solver the build did not write.  The HIP path, through
    the C ABI, at the solver default tolerance and at 1e-8, against it at the north_star bar."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp, linear_system_ocp
    g6 = np.load(os.path.join(GOLD, "g6_thirdparty.npz"))
    B = len(g6["cp_x0"])
    ocp = cartpole_ocp()
    theta = np.tile(ocp.p0, (B, 1))
    theta[:, :3] = g6["cp_theta_model"]
    for tol, bar in ((1e-8, RTOL), (None, 1e-5)):     # a run stopped at 1e-6 is within ~1e-6 x conditioning of the KKT point
        mpc = MPCBatch(cartpole_ocp() if tol is None else cartpole_ocp(tol=tol), B)
        mpc.set_theta(torch.as_tensor(theta))
        r = mpc.solve(g6["cp_x0"], cold=True)
        assert np.all(r.status.cpu().numpy() == 0)
        assert rel_err(r.u0.cpu().numpy(), g6["cp_u0"]) < bar and rel_err(r.V.cpu().numpy(), g6["cp_V"]) < RTOL
    for tag, gamma in (("g099", 0.99), ("g09", 0.9)):
        mpc = MPCBatch(linear_system_ocp(discount_factor=gamma), len(g6[f"lin_{tag}_x0"]))
        r = mpc.solve(g6[f"lin_{tag}_x0"], cold=True)
        assert np.all(r.status.cpu().numpy() == 0)
        assert rel_err(r.u0.cpu().numpy(), g6[f"lin_{tag}_u0"]) < RTOL and rel_err(r.V.cpu().numpy(), g6[f"lin_{tag}_V"]) < RTOL


def test_chain_mass_n7_vs_oracle_and_full_size_properties(oracle_port):
    """BASELINE config 4 at its perf dimension (n_mass = 7, nx = 33, N = 40): parity with the oracle port on 8 instances, then the
    full batch of 1024 — EVERY instance against the port (statuses, iteration counts, the four outputs at 1e-6) and through
    size-independent properties (all converge, KKT residuals below tol, bounds respected, a second call from the stored iterate needs
    no iteration and reproduces the outputs, results independent of the batch order)."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp, P = chain_mass_ocp(n_mass=7), make_chain_mass(n_mass=7)
    assert ocp.nx == 33 and ocp.n_p == P.n_p
    rng = np.random.default_rng(0)

    def inputs(B):
        x0 = np.tile(ocp.x0, (B, 1))
        x0[:, 3 * 6:] += rng.normal(0.0, 1e-2, (B, 15))      # N(0, 1e-2) velocity perturbation
        return x0

    x0 = inputs(8)
    _, r, ref = run_both(ocp, P, oracle_port, x0)
    st = r.status.cpu().numpy()
    assert np.all(st == 0) and np.array_equal(st, ref.status)
    assert np.abs(r.iters.cpu().numpy()[:, 0] - ref.sqp_iter).max() <= 1
    assert rel_err(r.u0.cpu().numpy(), ref.u0) < RTOL and rel_err(r.V.cpu().numpy(), ref.V) < RTOL
    assert rel_err(r.dV_dp.cpu().numpy(), ref.dV) < RTOL
    assert rel_err(r.dpi_dp.cpu().numpy(), ref.dpi, floor=np.abs(ref.dpi).max()) < RTOL
    B = 1024
    x0 = inputs(B)
    mpc = MPCBatch(ocp, B)
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    assert float(mpc.get_iterate()[4].max()) < 1e-5 and float(r.u0.abs().max()) <= 1.0 + 1e-9
    assert bool(torch.isfinite(r.dV_dp).all()) and bool(torch.isfinite(r.dpi_dp).all())
    r2 = mpc.solve(x0, sens_v=True, sens_pi=True)
    assert int(r2.iters[:, 0].max()) == 0 and torch.allclose(r2.V, r.V, rtol=1e-13) and torch.allclose(r2.dV_dp, r.dV_dp, rtol=1e-10, atol=1e-12)
    perm = rng.permutation(B)
    rp = MPCBatch(ocp, B).solve(x0[perm], sens_v=True, sens_pi=True, cold=True)      # (the same request: bit for bit)
    idx = torch.as_tensor(perm, device=r.V.device)
    assert torch.equal(rp.V, r.V[idx]) and torch.equal(rp.dV_dp, r.dV_dp[idx]) and torch.equal(rp.dpi_dp, r.dpi_dp[idx])
    # dV/dp has ONE evaluation order whatever the flags (grad_theta (nu' F) always comes off the tables of the second-order point pass,
    # chain_sens_th2_kernel): the same bits with and without du0*/dp
    rv = MPCBatch(ocp, B).solve(x0[perm], sens_v=True, cold=True)
    assert torch.equal(rv.V, rp.V) and torch.equal(rv.dV_dp, rp.dV_dp)
    from test_gpu_fullsize import chain_all_vs_port
    chain_all_vs_port(r, oracle_port.solve(P, x0), B, "chain n_mass 7 bench size")


def test_chain_mass_n3_vs_oracle(oracle_port):
    """The smallest chain (n_mass = 3, nx = 9): its own instantiation of the chain kernels — the in-wavefront direction pass takes
    whole stages per step there (the tables of seven stages do not fit the LDS region) — against the oracle port, and the RTI step."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp, P = chain_mass_ocp(n_mass=3), make_chain_mass(n_mass=3)
    assert ocp.nx == 9 and ocp.n_p == P.n_p
    rng = np.random.default_rng(3)
    B = 12
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 3 * 2:] += rng.normal(0.0, 1e-2, (B, 3))
    _, r, ref = run_both(ocp, P, oracle_port, x0)
    st = r.status.cpu().numpy()
    assert np.all(st == 0) and np.array_equal(st, ref.status)
    assert np.abs(r.iters.cpu().numpy()[:, 0] - ref.sqp_iter).max() <= 1
    assert rel_err(r.u0.cpu().numpy(), ref.u0) < RTOL and rel_err(r.V.cpu().numpy(), ref.V) < RTOL
    assert rel_err(r.dV_dp.cpu().numpy(), ref.dV) < RTOL
    assert rel_err(r.dpi_dp.cpu().numpy(), ref.dpi, floor=np.abs(ref.dpi).max()) < RTOL


@pytest.mark.parametrize("n_mass", [4, 6])
def test_chain_mass_even_sizes_vs_oracle(oracle_port, n_mass):
    """n_mass is a free integer in the reference (rlmpc/mpc/chain_mass/ocp_utils.py:344-350).  The even sizes (nx = 15 / 27) are the
    ones whose state count is not a multiple of the 4-row MFMA groups less one: the ragged row groups of the round-4 sweeps
    (chain_kernel.hpp OmCfg::RAGGED) run only here.  Solve, value / policy gradients and the RTI step against the oracle port."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from oracle.problems import make_chain_mass
    ocp, P = chain_mass_ocp(n_mass=n_mass), make_chain_mass(n_mass=n_mass)
    assert ocp.nx == (2 * (n_mass - 2) + 1) * 3 and ocp.n_p == P.n_p
    rng = np.random.default_rng(n_mass)
    B = 12
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 3 * (n_mass - 3):3 * (n_mass - 2)] += rng.normal(0.0, 1e-2, (B, 3))     # the last free mass, displaced
    x0[:, 3 * (n_mass - 1):] += rng.normal(0.0, 1e-2, (B, ocp.nx - 3 * (n_mass - 1)))   # and some velocity
    theta = np.tile(P.p0, (B, 1)) * rng.uniform(0.97, 1.03, (B, P.n_p))
    _, r, ref = run_both(ocp, P, oracle_port, x0, theta=theta)
    st = r.status.cpu().numpy()
    assert np.all(st == 0) and np.array_equal(st, ref.status)
    assert np.abs(r.iters.cpu().numpy()[:, 0] - ref.sqp_iter).max() <= 1
    assert rel_err(r.u0.cpu().numpy(), ref.u0) < RTOL and rel_err(r.V.cpu().numpy(), ref.V) < RTOL
    assert rel_err(r.dV_dp.cpu().numpy(), ref.dV) < RTOL
    assert rel_err(r.dpi_dp.cpu().numpy(), ref.dpi, floor=np.abs(ref.dpi).max()) < RTOL


def test_cartpole_cost_parameters_reach_the_kernel(oracle_port):
    """W_0, W, W_e, yref_0, yref, yref_e are part of p and the solve uses them (set_parameter / cost_set, mpc.py:233-257), per
    instance; their gradient entries stay zero (non-parameterised NLS mirror, nlp.py:1039-1055)."""
    from mpc4rl_amd import cartpole_ocp
    from oracle.problems import make_cartpole
    B = 48
    P = make_cartpole()
    rng = np.random.default_rng(4)
    theta = np.tile(P.p0, (B, 1))
    theta[:, :3] *= rng.uniform(0.95, 1.05, (B, 3))
    for b in range(B):
        d0, d, de = rng.uniform(0.5, 2.0, 5), rng.uniform(0.5, 2.0, 5), rng.uniform(0.5, 2.0, 4)
        W0, W, We = np.diag(P.p0[3:28].reshape(5, 5).diagonal() * d0), np.diag(P.p0[28:53].reshape(5, 5).diagonal() * d), \
            np.diag(P.p0[53:69].reshape(4, 4).diagonal() * de)
        W[0, 2] = W[2, 0] = 0.3 * rng.uniform(-1, 1)              # off-diagonal weight, symmetric
        W[1, 4] = 0.004                                           # and an unsymmetric entry: only (W + W')/2 matters
        theta[b, 3:28], theta[b, 28:53], theta[b, 53:69] = W0.flatten("F"), W.flatten("F"), We.flatten("F")
        theta[b, 69:74] = rng.uniform(-0.1, 0.1, 5)
        theta[b, 74:79] = rng.uniform(-0.1, 0.1, 5)
        theta[b, 79:83] = rng.uniform(-0.05, 0.05, 4)
    x0 = cartpole_x0(B, 4)
    _, r, ref = run_both(cartpole_ocp(), P, oracle_port, x0, theta=theta)
    check(r, ref)
    nominal = oracle_port.solve(P, x0)
    assert np.abs(ref.u0 - nominal.u0).max() > 0.5                # the cost block matters
    assert bool((r.dV_dp[:, 3:] == 0).all()) and bool((r.dpi_dp[:, :, 3:] == 0).all())


@pytest.mark.parametrize("B", [1, 2, 4, 100, 4097])
def test_ragged_batch_sizes(oracle_port, B):
    """Batch sizes that do not fill the last wavefront (3 instances per wave), a single instance, and > 4096."""
    from mpc4rl_amd import cartpole_ocp
    from oracle.problems import make_cartpole
    x0 = cartpole_x0(B, seed=7)
    mpc, r, ref = run_both(cartpole_ocp(), make_cartpole(), oracle_port, x0, nthreads=8)
    st = r.status.cpu().numpy()
    assert np.array_equal(st, ref.status)
    assert rel_err(r.u0.cpu().numpy(), ref.u0) < RTOL and rel_err(r.V.cpu().numpy(), ref.V) < RTOL
    assert rel_err(r.dV_dp.cpu().numpy(), ref.dV) < RTOL and rel_err(r.dpi_dp.cpu().numpy(), ref.dpi) < RTOL
    assert np.abs(r.iters.cpu().numpy()[:, 0] - ref.sqp_iter).max() <= 1


def test_status_codes_and_reorder_invariance(oracle_port):
    """max-iter status for every instance; the packing-order hint must not change any result bit."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    x0 = cartpole_x0(300, seed=9)
    mpc = MPCBatch(cartpole_ocp(max_iter=3), 300)
    r = mpc.solve(x0, cold=True)
    assert set(np.unique(r.status.cpu().numpy())) <= {0, 2} and int((r.status == 2).sum()) > 0
    assert int(r.iters[:, 0].max()) == 3
    a = MPCBatch(cartpole_ocp(), 300)
    ra = a.solve(x0, sens_v=True, sens_pi=True, cold=True, reorder=True)
    b = MPCBatch(cartpole_ocp(), 300)
    rb = b.solve(x0, sens_v=True, sens_pi=True, cold=True, reorder=False)
    for t1, t2 in ((ra.u0, rb.u0), (ra.V, rb.V), (ra.dV_dp, rb.dV_dp), (ra.dpi_dp, rb.dpi_dp), (ra.status, rb.status), (ra.iters, rb.iters)):
        assert torch.equal(t1, t2)


def test_full_size_properties_cartpole():
    """BASELINE full size (4096): size-independent properties instead of an oracle run — every instance converges, the KKT
    residuals are below tol, a second call from the stored iterate needs zero iterations and reproduces the outputs,
    V is invariant to a permutation of the batch, and u0 respects its bounds."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    B = 4096
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 4))
    x0[:, 2] = rng.uniform(0.9 * np.pi, 1.1 * np.pi, B)
    mpc = MPCBatch(cartpole_ocp(), B)
    r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    res = mpc.get_iterate()[4]
    assert float(res.max()) < 1e-6
    assert float(r.u0.abs().max()) <= 30.0 + 1e-9
    r2 = mpc.solve(x0, sens_v=True, sens_pi=True)
    assert int(r2.iters[:, 0].max()) == 0 and torch.allclose(r2.V, r.V, rtol=1e-14) and torch.allclose(r2.dV_dp, r.dV_dp, rtol=1e-12)
    perm = rng.permutation(B)
    rp = MPCBatch(cartpole_ocp(), B).solve(x0[perm], cold=True)
    assert torch.equal(rp.V, r.V[torch.as_tensor(perm, device=r.V.device)])


def test_auto_order_does_not_change_results():
    """mpcrl_auto_order (the packing-order kernel) does not change any result: bitwise the same outputs as with the identity order.
    A wrong permutation (a repeated or missing index) would leave some instance unsolved or solved twice and fail this."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    ocp = cartpole_ocp()
    B = 1000
    rng = np.random.default_rng(5)
    x0 = np.zeros((B, 4))
    x0[:, 2] = rng.uniform(0.9 * np.pi, 1.1 * np.pi, B)
    x0[:, 0] = rng.uniform(-0.01, 0.01, B)
    mpc = MPCBatch(ocp, B)
    mpc.set_launch_mode(-1)      # the plain launch: the one that reads the order (the time-sliced one clears it)
    xt = torch.as_tensor(x0, device="cuda")
    r1 = mpc.solve(xt, sens_v=True, cold=True, reorder=True)
    perm, _ = mpc.get_order()      # what that solve read: a permutation, and not the identity
    assert perm is not None
    perm = perm.cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(B)) and not np.array_equal(perm, np.arange(B))
    mpc.lib.mpcrl_set_order(mpc._h, None, None)
    r2 = mpc.solve(xt, sens_v=True, cold=True, reorder=False)
    assert torch.equal(r1.u0, r2.u0) and torch.equal(r1.V, r2.V) and torch.equal(r1.dV_dp, r2.dV_dp)


@pytest.mark.parametrize("B", [4, 7, 100, 4096, 5000])
def test_time_sliced_launch_is_bitwise_the_plain_one(B, monkeypatch):
    """small_solve_sliced_kernel (ipw + 1 instances per wavefront, one parked — in LDS at this horizon — between SQP iterations) runs
    the same iteration per instance as small_solve_kernel: every output bit-identical, for ragged batches too.  MPCRL_TIME_SLICE
    forces / forbids it."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    x0 = cartpole_x0(B, seed=13)
    theta = np.tile(cartpole_ocp().p0, (B, 1))
    theta[:, :3] *= np.random.default_rng(1).uniform(0.95, 1.05, (B, 3))
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCRL_TIME_SLICE", mode)
        mpc = MPCBatch(cartpole_ocp(), B)
        mpc.set_theta(torch.as_tensor(theta))
        r = mpc.solve(x0, sens_v=True, sens_pi=True, cold=True)
        out[mode] = (r, mpc.get_iterate(), mpc.get_lagrangian())
    (ra, ia, la), (rb, ib, lb) = out["0"], out["1"]
    assert int((ra.status == 0).sum()) > 0.9 * B
    for t1, t2 in ((ra.u0, rb.u0), (ra.V, rb.V), (ra.status, rb.status), (ra.iters, rb.iters), (ra.dV_dp, rb.dV_dp), (ra.dpi_dp, rb.dpi_dp), (la, lb)):
        assert torch.equal(t1, t2)
    for t1, t2 in zip(ia, ib):
        assert torch.equal(t1, t2)
    # a warm call after the sliced cold one starts at the solution (the parked / finished iterates were all written back)
    r2 = mpc.solve(x0)
    ok = rb.status == 0
    assert int(r2.iters[ok][:, 0].max()) == 0 and torch.equal(r2.V[ok], rb.V[ok])


@pytest.mark.parametrize("N,tf", [(20, 2.0), (30, 3.0)])
def test_time_sliced_launch_q_mode(N, tf, monkeypatch):
    """Q-mode (u0 pinned, mpc.py:71-76) through the sliced launch: the pinned u0 follows its instance through the rotation, with the
    parked instance in LDS (N = 20) and in HBM (N = 30).  Bit-identical to the plain launch."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    B = 101
    x0 = cartpole_x0(B, seed=21)
    u0 = torch.as_tensor(np.random.default_rng(2).uniform(-20.0, 20.0, (B, 1)), device="cuda")
    out = []
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCRL_TIME_SLICE", mode)
        mpc = MPCBatch(cartpole_ocp(N=N, tf=tf), B)
        out.append(mpc.solve(x0, u0, sens_v=True, cold=True))
    ra, rb = out
    assert int((ra.status == 0).sum()) > 0.8 * B
    for f in ("u0", "V", "status", "iters", "dV_dp"):
        assert torch.equal(getattr(ra, f), getattr(rb, f)), f
    assert torch.equal(ra.u0[ra.status == 0], u0[ra.status == 0])


def test_time_sliced_launch_status_codes(monkeypatch):
    """max-iter status inside the sliced launch: iteration counts and statuses equal the plain launch's."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    x0 = cartpole_x0(301, seed=9)
    res = []
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCRL_TIME_SLICE", mode)
        r = MPCBatch(cartpole_ocp(max_iter=3), 301).solve(x0, cold=True)
        res.append(r)
    assert torch.equal(res[0].status, res[1].status) and torch.equal(res[0].iters, res[1].iters) and torch.equal(res[0].V, res[1].V)
    assert int((res[1].status == 2).sum()) > 0 and int(res[1].iters[:, 0].max()) == 3


@pytest.mark.parametrize("N,tf", [(15, 1.5), (30, 3.0), (10, 1.0)])
def test_time_sliced_launch_other_horizons(N, tf, monkeypatch, oracle_port):
    """Horizons with a different number of instance slots per wavefront (N = 30: 2 slots + 1 parked, N = 15: 3 + 1 with 16-lane
    slots, N = 10: the matrix-core sweep caps the slots at 4, sliced 3 + 1): sliced == plain bitwise, and both match the oracle."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    from oracle.problems import make_cartpole
    B = 97
    x0 = cartpole_x0(B, seed=21)
    out = []
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCRL_TIME_SLICE", mode)
        mpc = MPCBatch(cartpole_ocp(N=N, tf=tf), B)
        out.append(mpc.solve(x0, sens_v=True, sens_pi=True, cold=True))
    ra, rb = out
    for t1, t2 in ((ra.u0, rb.u0), (ra.V, rb.V), (ra.status, rb.status), (ra.iters, rb.iters), (ra.dV_dp, rb.dV_dp), (ra.dpi_dp, rb.dpi_dp)):
        assert torch.equal(t1, t2)
    ref = oracle_port.solve(make_cartpole(N=N, tf=tf), x0)
    st = rb.status.cpu().numpy()
    assert np.array_equal(st, ref.status)
    ok = st == 0
    assert ok.mean() > 0.8
    assert rel_err(rb.u0.cpu().numpy()[ok], ref.u0[ok]) < RTOL and rel_err(rb.V.cpu().numpy()[ok], ref.V[ok]) < RTOL
    assert rel_err(rb.dV_dp.cpu().numpy()[ok], ref.dV[ok]) < RTOL and rel_err(rb.dpi_dp.cpu().numpy()[ok], ref.dpi[ok]) < RTOL


def test_sensitivity_rows_are_written_in_full():
    """The small models' sensitivity kernel owns its output rows (no memset in front of it): with the output buffers poisoned
    before mpcrl_solve, the cost block of p comes back exactly zero, du0*/dp is zero in Q-mode, an instance that was not solved
    (NaN x0: status neither 0 nor 2) has zero rows, and the entries with a gradient equal those of an ordinary solve."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp, linear_system_ocp
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import _ptr
    for ocp, nx in ((cartpole_ocp(), 4), (linear_system_ocp(), 2)):
        B = 131
        x0 = cartpole_x0(B, seed=4) if nx == 4 else np.random.default_rng(4).uniform(-0.5, 0.5, (B, 2))
        x0[7] = np.nan
        ref = MPCBatch(ocp, B).solve(x0, sens_v=True, sens_pi=True, cold=True)
        for qmode in (False, True):
            mpc = MPCBatch(ocp, B)
            kw = dict(dtype=torch.float64, device=mpc.device)
            xd = torch.as_tensor(x0, **kw).contiguous()
            ud = torch.zeros((B, mpc.nu), **kw) if qmode else None
            u0o, V = torch.empty((B, mpc.nu), **kw), torch.empty((B,), **kw)
            dV, dpi = torch.full((B, mpc.n_p), np.nan, **kw), torch.full((B, mpc.nu, mpc.n_p), np.nan, **kw)
            st, it = torch.empty((B,), dtype=torch.int32, device=mpc.device), torch.empty((B, 2), dtype=torch.int32, device=mpc.device)
            flags = _lib.SENS_V | _lib.SENS_PI | _lib.COLD
            rc = mpc.lib.mpcrl_solve(mpc._h, _ptr(xd), _ptr(ud), flags, _ptr(u0o), _ptr(V), _ptr(dV), _ptr(dpi), _ptr(st), _ptr(it),
                                     mpc._stream())
            torch.cuda.synchronize()
            assert rc == 0
            solved = (st == 0) | (st == 2)
            assert int(st[7]) == 1 and int(solved.sum()) >= B - 12   # NaN x0: status 1 (as in the oracle), not a silent "converged"
            assert torch.all(dV[~solved] == 0.0) and torch.all(dpi[~solved] == 0.0)
            assert torch.isfinite(dV[solved]).all()
            if nx == 4:
                assert torch.all(dV[:, 3:] == 0.0) and torch.all(dpi[:, :, 3:] == 0.0)
            if qmode:
                assert torch.all(dpi == 0.0)
            else:
                assert torch.equal(st, ref.status)
                assert torch.equal(dV, ref.dV_dp)
                assert torch.equal(torch.nan_to_num(dpi, nan=7.0), torch.nan_to_num(ref.dpi_dp, nan=7.0))


@pytest.mark.parametrize("N,tf,B", [(20, 2.0, 4096), (20, 2.0, 101), (30, 3.0, 203)])
def test_time_sliced_launch_warm_calls(N, tf, B, monkeypatch):
    """Warm calls through the time-sliced launch (small_solve_sliced_kernel<.., WARM>): the resident instances and, on its first take,
    the parked one start from their stored iterates; the per-instance cold mask, the change of x0 that sizes the first QP's warm
    start, the Q-mode's pinned u0 and a stored iterate without multipliers (MPCRL_COLD_DUAL) are handled as in small_solve_kernel.
    A closed-loop sequence — cold solve, three warm solves at moved states (one with a cold mask, one in Q-mode), set_iterate without
    multipliers, warm solve — must be bit-identical between the two launch shapes, parked state in LDS (N = 20) and in HBM (N = 30)."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    rng = np.random.default_rng(5)
    x0 = cartpole_x0(B, seed=17)
    steps = [torch.as_tensor(rng.normal(0.0, s, (B, 4)), device="cuda") for s in (0.02, 0.05, 0.01)]
    mask = torch.as_tensor(rng.uniform(size=B) < 0.2, device="cuda")
    u0 = torch.as_tensor(rng.uniform(-10.0, 10.0, (B, 1)), device="cuda")
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MPCRL_TIME_SLICE", mode)
        mpc = MPCBatch(cartpole_ocp(N=N, tf=tf), B)
        xs = torch.as_tensor(x0, device="cuda").clone()
        seq = [mpc.solve(xs, cold=True)]
        xs = xs + steps[0]
        seq.append(mpc.solve(xs, sens_pi=True))                                   # warm
        xs = xs + steps[1]
        seq.append(mpc.solve(xs, sens_v=True, cold_mask=mask))                    # warm, a fifth of the instances reset
        xs = xs + steps[2]
        seq.append(mpc.solve(xs, u0, sens_v=True))                                # warm, Q-mode
        x, u, pi, bnd, res = mpc.get_iterate()
        mpc.set_iterate(x, u, pi)                                                 # primal iterate only: next solve = MPCRL_COLD_DUAL
        seq.append(mpc.solve(xs))
        out[mode] = (seq, mpc.get_iterate())
    (sa, ia), (sb, ib) = out["0"], out["1"]
    for n, (ra, rb) in enumerate(zip(sa, sb)):
        assert int((ra.status == 0).sum()) > 0.8 * B, n
        for f in ("u0", "V", "status", "iters", "dV_dp", "dpi_dp"):
            t1, t2 = getattr(ra, f), getattr(rb, f)
            assert (t1 is None and t2 is None) or torch.equal(torch.nan_to_num(t1), torch.nan_to_num(t2)), (n, f)
    for t1, t2 in zip(ia, ib):
        assert torch.equal(t1, t2)
    ok = (sa[0].status == 0) & (sa[1].status == 0) & (sa[2].status == 0)
    it = lambda r, m: float(r.iters[m][:, 0].double().mean())
    assert it(sa[1], ok) < 0.9 * it(sa[0], ok)                      # a warm call is warm ...
    assert it(sa[2], ok & mask) > 1.1 * it(sa[2], ok & ~mask)       # ... and an instance of the cold mask is not


@pytest.mark.parametrize("N,B", [(40, 4096), (40, 101), (20, 37), (39, 64), (47, 50), (48, 50), (61, 21), (63, 23)])
def test_linear_kernel_three_stages_per_lane_vs_one(N, B, monkeypatch):
    """lq_solve_kernel (linear_kernel.hpp: three stages per lane; four instances per wavefront in DPP rows at 9..16 lanes per instance,
    eight in half rows up to 8 lanes; FOUR stages per lane in rows at N = 48..63, round 6) against small_solve_kernel<LinearDev> (MPCRL_LINEAR_SPL=1: one stage per lane) on a closed-loop
    sequence — cold solve with both gradients, warm solves at moved states, a per-instance cold mask, Q-mode, a stored iterate without
    multipliers, a real-time iteration, per-instance parameters — over horizons that exercise every lane layout (N + 1 = 3 x lanes
    exactly, one and two dead stages in the last lane, lanes behind the live ones, more than 16 lanes).  Same iteration, other
    summation order: statuses and SQP iteration counts are equal, interior-point counts equal on > 99 % of the instances and never
    more than one apart, numbers agree within the 1e-6 bar of the port comparison where the counts are equal (an iterate that stops one
    interior-point iteration earlier differs by what the QP tolerance allows: 1e-4)."""
    from mpc4rl_amd import MPCBatch, linear_system_ocp
    rng = np.random.default_rng(N * 1000 + B)
    x0 = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.5, 0.5, B)])
    steps = [torch.as_tensor(rng.normal(0.0, s, (B, 2)), device="cuda") for s in (0.02, 0.05, 0.01, 0.01)]
    mask = torch.as_tensor(rng.uniform(size=B) < 0.25, device="cuda")
    u0 = torch.as_tensor(rng.uniform(-0.9, 0.9, (B, 1)), device="cuda")
    ocp = linear_system_ocp(N=N)
    theta = np.tile(ocp.p0, (B, 1))
    theta[:, :6] *= rng.uniform(0.97, 1.03, (B, 6))
    theta[:, 9:] = rng.normal(0.0, 0.05, (B, 3))
    out = {}
    for spl in ("1", "3"):
        monkeypatch.setenv("MPCRL_LINEAR_SPL", spl)
        mpc = MPCBatch(ocp, B)
        xs = torch.as_tensor(x0, device="cuda").clone()
        seq = [mpc.solve(xs, sens_v=True, sens_pi=True, cold=True)]
        xs = (xs + steps[0]).clamp_(torch.tensor([0.05, -0.9], device="cuda"), torch.tensor([0.95, 0.9], device="cuda"))
        seq.append(mpc.solve(xs, sens_pi=True))                                   # warm
        xs = xs + steps[1] * 0.2
        seq.append(mpc.solve(xs, sens_v=True, cold_mask=mask))                    # warm, a quarter of the instances reset
        xs = xs + steps[2] * 0.2
        seq.append(mpc.solve(xs, u0, sens_v=True))                                # warm, Q-mode
        x, u, pi, bnd, res = mpc.get_iterate()
        mpc.set_iterate(x, u, pi)                                                 # primal iterate only: next solve = MPCRL_COLD_DUAL
        seq.append(mpc.solve(xs))
        seq.append(mpc.solve(xs + steps[3] * 0.2, rti=True, sens_pi=True))       # one real-time iteration
        mpc.set_theta(torch.as_tensor(theta))
        seq.append(mpc.solve(xs, sens_v=True, sens_pi=True, cold=True))           # per-instance parameters
        out[spl] = (seq, mpc.get_iterate(), mpc.get_lagrangian() if hasattr(mpc, "get_lagrangian") else None)
    (sa, ia, la), (sb, ib, lb) = out["1"], out["3"]
    close = lambda t1, t2, tol: float((torch.nan_to_num(t1) - torch.nan_to_num(t2)).abs().max() / max(1.0, float(torch.nan_to_num(t1).abs().max()))) < tol
    for n, (ra, rb) in enumerate(zip(sa, sb)):
        assert int((ra.status == 0).sum()) > 0.9 * B, n
        nst = int((ra.status != rb.status).sum())
        dit = (ra.iters[:, 1] - rb.iters[:, 1]).abs()
        print(f"call {n}: statuses differ on {nst} of {B} instances, interior-point counts on {int((dit != 0).sum())} (by at most {int(dit.max())})")
        # a stopping test met to within rounding moves an interior-point count by one, and after a real-time iteration (call 5) the
        # status of an instance whose residual sits at tol
        assert nst <= (B // 1000 if n == 5 else 0) and torch.equal(ra.iters[:, 0], rb.iters[:, 0]), n
        assert int(dit.max()) <= 1 and float((dit == 0).double().mean()) > 0.99, n
        ok = (ra.status == 0) & (rb.status == 0)
        for f in ("u0", "V", "dV_dp", "dpi_dp"):
            t1, t2 = getattr(ra, f), getattr(rb, f)
            assert (t1 is None) == (t2 is None), (n, f)
            if t1 is not None:
                # du0*/dp is ill-defined where a soft bound is active (quirk q1): the two kernels share the adjoint pass on slightly
                # different iterates, so the comparison is loose there and tight everywhere else
                assert close(t1[ok & (dit == 0)], t2[ok & (dit == 0)], 2e-5 if f == "dpi_dp" else 1e-6), (n, f)
                if bool((ok & (dit != 0)).any()):      # stopped one iteration apart: the QP tolerance is what they share
                    assert close(t1[ok & (dit != 0)], t2[ok & (dit != 0)], 1e-3 if f == "dpi_dp" else 1e-4), (n, f)
    for t1, t2 in zip(ia[:3], ib[:3]):      # x, u, pi (the rows' multipliers near zero move with a stopping test met one iteration apart)
        assert close(t1, t2, 1e-4)
    if la is not None:
        assert close(la, lb, 1e-4)


def test_hip_vs_third_party_gradients_and_chain_solutions():
    """G7 (tests/golden/make_thirdparty_grad.py): dV/dp and du0*/dp of the HIP path against central differences of a THIRD-PARTY solver's
    V and u0* (scipy SLSQP on cartpole, a certified active-set polish of trust-constr on the linear system) at 1e-5, and u0*, V of the
    chain of masses against SLSQP's KKT points at 1e-6 — gradients and a chain solution that no code of this repository produced."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp, chain_mass_ocp, linear_system_ocp
    if not os.path.exists(os.path.join(GOLD, "g7_thirdparty_grad.npz")):
        pytest.skip("tests/golden/g7_thirdparty_grad.npz has not been generated (make_thirdparty_grad.py, ~1.5 h on 8 cores)")
    g7 = np.load(os.path.join(GOLD, "g7_thirdparty_grad.npz"))

    def held(fd0, fd1, mine):
        # Central differences at two steps, d and 10 d: fd(d) = g + c d^2, so g = fd0 - (fd1 - fd0) / 99 and |fd1 - fd0| / 99 estimates
        # what is left of the truncation error in fd0; entries whose estimate exceeds 2e-6 are left out (and NaN entries of jobs the
        # generator did not finish).  Returns the largest |mine - g|, rows scaled by their largest entry (>= 1).
        fd0, fd1, mine = (np.asarray(a, float).reshape(len(fd0), -1) for a in (fd0, fd1, mine))
        fin = np.isfinite(fd0) & np.isfinite(fd1)
        if not fin.any():
            return 0.0
        f0, f1 = np.where(fin, fd0, 0.0), np.where(fin, fd1, 0.0)
        scale = np.maximum(np.abs(f0).max(axis=1, keepdims=True), 1.0)
        g = f0 - (f1 - f0) / 99.0
        ok = fin & (np.abs(f1 - f0) / 99.0 <= 2e-6 * scale)
        assert ok[fin].mean() >= 0.9, ok[fin].mean()
        return float(np.where(ok, np.abs(mine - g) / scale, 0.0).max())

    B = len(g7["cp_x0"])
    ocp = cartpole_ocp(tol=1e-9)
    theta = np.tile(ocp.p0, (B, 1))
    theta[:, :3] = g7["cp_theta_model"]
    mpc = MPCBatch(ocp, B)
    mpc.set_theta(torch.as_tensor(theta))
    r = mpc.solve(g7["cp_x0"], sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    assert rel_err(r.u0.cpu().numpy(), g7["cp_u0"]) < RTOL and rel_err(r.V.cpu().numpy(), g7["cp_V"]) < RTOL
    e_v = held(g7["cp_dV_d0"], g7["cp_dV_d1"], r.dV_dp.cpu().numpy()[:, :3])
    e_pi = held(g7["cp_du0_d0"][:, :, 0], g7["cp_du0_d1"][:, :, 0], r.dpi_dp.cpu().numpy()[:, 0, :3])
    print("cartpole vs third-party finite differences: dV/dp", e_v, "du0*/dp", e_pi)
    assert e_v < 1e-5 and e_pi < 1e-5
    for tag, gamma in (("g099", 0.99), ("g09", 0.9)):
        ml = MPCBatch(linear_system_ocp(discount_factor=gamma), len(g7[f"lin_{tag}_x0"]))
        ml.set_options(tol=1e-9)
        rl = ml.solve(g7[f"lin_{tag}_x0"], sens_v=True, sens_pi=True, cold=True)
        assert bool((rl.status == 0).all())
        have = np.isfinite(g7[f"lin_{tag}_V"])
        if have.any():
            assert rel_err(rl.u0.cpu().numpy()[have], g7[f"lin_{tag}_u0"][have]) < RTOL and rel_err(rl.V.cpu().numpy()[have], g7[f"lin_{tag}_V"][have]) < RTOL
        e_v = held(g7[f"lin_{tag}_dV_d0"], g7[f"lin_{tag}_dV_d1"], rl.dV_dp.cpu().numpy())
        e_pi = held(g7[f"lin_{tag}_du0_d0"][:, :, 0], g7[f"lin_{tag}_du0_d1"][:, :, 0], rl.dpi_dp.cpu().numpy()[:, 0, :])
        print("linear", tag, "vs third-party finite differences: dV/dp", e_v, "du0*/dp", e_pi)
        assert e_v < 1e-5 and e_pi < 3e-5      # (du0*/dp: the weakly active soft row, see tests/test_oracle.py)
        if not len(g7[f"lin_{tag}_polished_x0"]):
            continue
        mp_ = MPCBatch(linear_system_ocp(discount_factor=gamma), len(g7[f"lin_{tag}_polished_x0"]))
        mp_.set_options(tol=1e-9)
        rp = mp_.solve(g7[f"lin_{tag}_polished_x0"], cold=True)
        assert rel_err(rp.u0.cpu().numpy(), g7[f"lin_{tag}_polished_u0"]) < RTOL and rel_err(rp.V.cpu().numpy(), g7[f"lin_{tag}_polished_V"]) < RTOL
    for n_mass in (3, 5):
        if f"chain{n_mass}_x0" not in g7.files:
            continue
        mc = MPCBatch(chain_mass_ocp(n_mass=n_mass, tol=1e-9), 1)
        rc = mc.solve(g7[f"chain{n_mass}_x0"][None], cold=True)
        assert int(rc.status[0]) == 0
        assert rel_err(rc.u0.cpu().numpy(), g7[f"chain{n_mass}_u0"][None]) < RTOL and abs(float(rc.V[0]) - float(g7[f"chain{n_mass}_V"])) < RTOL * max(1.0, abs(float(rc.V[0])))


@pytest.mark.parametrize("fixture", ["g8_chain_grad.npz", "g8_chain4_grad.npz", "g8_chain5_grad.npz", "g8_chain7_grad.npz"])
def test_hip_vs_third_party_chain_gradients(fixture):
    """G8 (tests/golden/make_thirdparty_chain_grad.py): dV/dp and du0*/dp of the HIP chain path (n_mass 3) against central differences of
    scipy-SLSQP's V and u0* over four parameters of different kinds (mass, spring constant, rest length, damping) at 1e-5."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    f = os.path.join(GOLD, fixture)
    if not os.path.exists(f):
        pytest.skip(f"tests/golden/{fixture} has not been generated (make_thirdparty_chain_grad.py, hours)")
    g8 = np.load(f)
    mc = MPCBatch(chain_mass_ocp(n_mass=int(g8["n_mass"]), tol=1e-9), 1)
    r = mc.solve(g8["x0"][None], sens_v=True, sens_pi=True, cold=True)
    assert int(r.status[0]) == 0
    assert rel_err(r.u0.cpu().numpy(), g8["u0"][None]) < RTOL and abs(float(r.V[0]) - float(g8["V"])) < RTOL * max(1.0, abs(float(g8["V"])))
    idx = g8["p_index"]
    dV, dpi = r.dV_dp.cpu().numpy()[0], r.dpi_dp.cpu().numpy()[0]
    for name, mine, fd0, fd1 in (("dV/dp", dV[idx], g8["dV_d0"], g8["dV_d1"]), ("du0*/dp", dpi[:, idx].T, g8["du0_d0"], g8["du0_d1"])):
        fd0, fd1, mine = (np.asarray(a, float).reshape(len(idx), -1) for a in (fd0, fd1, mine))
        scale = np.maximum(np.abs(fd0).max(1, keepdims=True), 1.0)
        ok = np.abs(fd0 - fd1) <= 2e-6 * scale
        assert ok.all()                                    # every entry is used (round 5 accepted a quarter of dropped ones)
        err = float((np.abs(mine - fd0) / scale).max())
        print("chain n_mass", int(g8["n_mass"]), name, "HIP vs third-party finite differences:", err)
        assert err < 1e-5, name


def test_hip_vs_third_party_reference_sweep():
    """The reference's own chain test (tests/test_chain_mass.py -> rlmpc/examples/chain_mass.py:133-174: C_3_0 over linspace(0.05, 0.15, 10) at
    n_mass 5, x0 of examples/chain_mass.py:17-25) on the HIP path, held to certified third-party KKT points and their finite differences
    (G8 sweep): ONE batched solve of the ten parameter points, u0*, V at 1e-6, dV/dC_3_0 and du0*/dC_3_0 at 1e-5."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    f = os.path.join(GOLD, "g8_chain5_sweep.npz")
    if not os.path.exists(f):
        pytest.skip("tests/golden/g8_chain5_sweep.npz has not been generated")
    g = np.load(f)
    ocp = chain_mass_ocp(n_mass=5, tol=1e-9)
    n, j = len(g["C_3_0"]), int(g["p_index"][0])
    assert ocp.p_labels[j] == "C_3_0" and np.allclose(g["x0"], ocp.x0)
    th = np.tile(ocp.p0, (n, 1))
    th[:, j] = g["C_3_0"]
    mc = MPCBatch(ocp, n)
    mc.set_theta(torch.as_tensor(th))
    r = mc.solve(np.tile(g["x0"], (n, 1)), sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    assert rel_err(r.u0.cpu().numpy(), g["u0"]) < RTOL and rel_err(r.V.cpu().numpy(), g["V"]) < RTOL
    dV, dpi = r.dV_dp.cpu().numpy()[:, j], r.dpi_dp.cpu().numpy()[:, :, j]
    for name, mine, fd0, fd1 in (("dV/dC_3_0", dV, g["dV_d0"], g["dV_d1"]), ("du0*/dC_3_0", dpi, g["du0_d0"], g["du0_d1"])):
        fd0, fd1, mine = (np.asarray(a, float).reshape(n, -1) for a in (fd0, fd1, mine))
        scale = np.maximum(np.abs(fd0).max(1, keepdims=True), 1.0)
        assert (np.abs(fd0 - fd1) <= 2e-6 * scale).all()
        err = float((np.abs(mine - fd0) / scale).max())
        print("reference sweep,", name, "HIP vs third-party finite differences:", err)
        assert err < 1e-5, name


def test_hip_vs_third_party_cartpole_gradients_active_state_bound():
    """G7b (tests/golden/make_thirdparty_grad2.py): the HIP path's dV/dp and du0*/dp against central differences of scipy-SLSQP's V and u0*
    at ten cartpole states with an unsaturated u0*, four of them with the position bound |s| <= 2.4 active on the horizon."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    g = np.load(os.path.join(GOLD, "g7b_cartpole_grad.npz"))
    assert np.all(np.abs(g["u0"]) < 29.0) and np.all(np.abs(g["s_max"][:4] - 2.4) < 1e-7)
    mpc = MPCBatch(cartpole_ocp(tol=1e-9), len(g["x0"]))
    r = mpc.solve(g["x0"], sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    bnd = mpc.get_iterate()[3].cpu().numpy()                      # lam_l, lam_u of the state rows on stages 1..N
    lam_x = bnd[:, 0:2, 1:, 1:]
    assert np.all(lam_x[:4].reshape(4, -1).max(1) > 1e-3)
    assert rel_err(r.u0.cpu().numpy(), g["u0"]) < RTOL and rel_err(r.V.cpu().numpy(), g["V"]) < RTOL

    def held(fd0, fd1, mine):
        fd0, fd1, mine = (np.asarray(a, float).reshape(len(fd0), -1) for a in (fd0, fd1, mine))
        scale = np.maximum(np.abs(fd0).max(axis=1, keepdims=True), 1.0)
        gg = fd0 - (fd1 - fd0) / 99.0
        ok = np.abs(fd1 - fd0) / 99.0 <= 2e-6 * scale
        assert ok.mean() >= 0.9, ok
        return float(np.where(ok, np.abs(mine - gg) / scale, 0.0).max())

    e_v = held(g["dV_d0"], g["dV_d1"], r.dV_dp.cpu().numpy()[:, :3])
    e_pi = held(g["du0_d0"][:, :, 0], g["du0_d1"][:, :, 0], r.dpi_dp.cpu().numpy()[:, 0, :3])
    print("cartpole (active state bound / near upright) HIP vs third-party finite differences: dV/dp", e_v, "du0*/dp", e_pi)
    assert e_v < 1e-6 and e_pi < 1e-6       # (the stiffness cap alone: 3.6e-6; with the Richardson extrapolation in the cap: 3e-9)


def test_hip_vs_third_party_cartpole_gradients_96_states():
    """G7c (tests/golden/make_thirdparty_grad3.py): the HIP path against certified third-party KKT points (MINPACK on the KKT equations) and
    their finite differences at 94 cartpole states — u0*, V at 1e-6, dV/dp, du0*/dp at 1e-5."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    g = np.load(os.path.join(GOLD, "g7c_cartpole_grad.npz"))
    n = len(g["x0"])
    mpc = MPCBatch(cartpole_ocp(tol=1e-9), n)
    r = mpc.solve(g["x0"], sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all())
    assert rel_err(r.u0.cpu().numpy(), g["u0"]) < RTOL and rel_err(r.V.cpu().numpy(), g["V"]) < RTOL

    def held(fd0, fd1, mine):
        fd0, fd1, mine = (np.asarray(a, float).reshape(len(fd0), -1) for a in (fd0, fd1, mine))
        scale = np.maximum(np.abs(fd0).max(axis=1, keepdims=True), 1.0)
        gg = fd0 - (fd1 - fd0) / 99.0
        ok = np.abs(fd1 - fd0) / 99.0 <= 2e-6 * scale
        assert ok.mean() >= 0.98, ok.mean()
        return float(np.where(ok, np.abs(mine - gg) / scale, 0.0).max())

    e_v = held(g["dV_d0"], g["dV_d1"], r.dV_dp.cpu().numpy()[:, :3])
    e_pi = held(g["du0_d0"][:, :, 0], g["du0_d1"][:, :, 0], r.dpi_dp.cpu().numpy()[:, 0, :3])
    print("cartpole, %d states, HIP vs third-party finite differences: dV/dp" % n, e_v, "du0*/dp", e_pi)
    assert e_v < 1e-5 and e_pi < 1e-5


def test_hip_vs_third_party_q_mode_gradients():
    """G7d: Q(s, a) and dQ/dp of the HIP path (u0_fixed of mpcrl_solve; MPC.q_update, mpc.py:52-96) at 31 cartpole (state, pinned u0) pairs
    against certified third-party KKT points (MINPACK on the KKT equations with u_0 as an equality) and their central differences."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    g = np.load(os.path.join(GOLD, "g7d_cartpole_qmode.npz"))
    n = len(g["x0"])
    mpc = MPCBatch(cartpole_ocp(tol=1e-9), n)
    r = mpc.solve(g["x0"], g["u0"], sens_v=True, sens_pi=True, cold=True)
    assert bool((r.status == 0).all()) and np.array_equal(r.u0.cpu().numpy(), g["u0"])
    assert rel_err(r.V.cpu().numpy(), g["Q"]) < RTOL
    fd0, fd1, mine = g["dQ_d0"], g["dQ_d1"], r.dV_dp.cpu().numpy()[:, :3]
    scale = np.maximum(np.abs(fd0).max(axis=1, keepdims=True), 1.0)
    gg = fd0 - (fd1 - fd0) / 99.0
    ok = np.abs(fd1 - fd0) / 99.0 <= 2e-6 * scale
    assert ok.mean() >= 0.98
    e = float(np.where(ok, np.abs(mine - gg) / scale, 0.0).max())
    print("cartpole Q-mode, %d pairs, HIP dQ/dp vs third-party finite differences:" % n, e)
    assert e < 1e-6 and bool((r.dpi_dp == 0.0).all())


@pytest.mark.parametrize("spl", ["3", "1"])
def test_linear_warm_qp_failure_restarts_cold(spl, monkeypatch, oracle_port):
    """LQ model, both kernel families: a WARM interior point that runs out of iterations (it jams against the rows the moved x0
    activates, then cycles: tests/test_oracle.py WARM_QP_FAILS, found by profiles/microbench/fuzz_parity.py seed 7 as a status 4 of
    the product AND the port) is run once more from the cold interior point.  Which side of 60 iterations a jammed interior point
    ends on is decided by rounding, so the assertion is the result: status 0 and the ONE solution of the convex QP."""
    from mpc4rl_amd import MPCBatch, linear_system_ocp
    from oracle.problems import make_linear_system
    WARM_QP_FAILS = np.array([[[0.8726968153298129, 0.5483649132524803], [0.8572483237722713, 0.5365310381189186]],
                              [[0.11781405145159196, -0.5019479937647703], [0.12047207467889322, -0.4954152158824344]],
                              [[0.8580657761160446, 0.5993274993476269], [0.8486730546864062, 0.6143373226840217]]])
    monkeypatch.setenv("MPCRL_LINEAR_SPL", spl)
    P = make_linear_system(gamma=0.9, N=23)
    mpc = MPCBatch(linear_system_ocp(discount_factor=0.9, N=23), 3)
    r0 = mpc.solve(WARM_QP_FAILS[:, 0], sens_v=True, cold=True)
    r1 = mpc.solve(WARM_QP_FAILS[:, 1], sens_v=True)
    first = oracle_port.solve(P, WARM_QP_FAILS[:, 0])
    warm = oracle_port.solve(P, WARM_QP_FAILS[:, 1], warm=first)
    cold = oracle_port.solve(P, WARM_QP_FAILS[:, 1])
    print("interior-point iterations of the warm call:", r1.iters[:, 1].tolist(), "port", warm.ipm_iter.tolist())
    assert torch.all(r0.status == 0) and torch.all(r1.status == 0)
    assert rel_err(r1.u0.cpu().numpy(), cold.u0) < 1e-6 and rel_err(r1.V.cpu().numpy(), cold.V) < 1e-6
    assert rel_err(r1.dV_dp.cpu().numpy(), cold.dV) < 1e-4
    same = r1.iters[:, 1].cpu().numpy() == warm.ipm_iter
    assert same.sum() >= 1 and rel_err(r1.dV_dp.cpu().numpy()[same], warm.dV[same]) < 1e-6
