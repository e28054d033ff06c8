"""CPU checks of the Q-learners' Gauss-Newton step inside a box and a trust region: the C ABI's new symbol, the torch statement
``qlearning_gn_box_step`` against a brute-force enumeration of all active sets, the KKT certificate of tests/gn_box_cases.py on boxes of
every kind, the info codes, the step's covariance under a rescaling of the parameters, and the constructors' argument checks.

Bounds (derived, not measured; eps = 2^-53): the certificate's tol_a (gn_box_cases.py), and for two solves of one block
  ||d - d_ref||_2 <= 8 K (K + 1) eps cond_2(H_FF) ||d_ref||_2 (backward stability of Cholesky, on both sides)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from gn_box_cases import EPS, box_of, brute_force, certificate, correlated_problem, h_of, make_cases, message

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mpcrl_qlearning_gn_apply_box"


def test_new_symbol_in_header_and_binding_abi132():
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    api = open(os.path.join(ROOT, "mpc4rl_amd", "csrc", "mpcrl_loops.hip")).read()
    assert re.search(r"\b" + NEW + r"\(", hdr) and re.search(r"\b" + NEW + r"\(", api) and NEW in _lib.EXPORTS
    assert int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 132
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.mpcrl_version() == 132
        getattr(lib, NEW)


def _box_step(c, K, lr, damping, **kw):
    from mpc4rl_amd import qlearning_gn_box_step
    return qlearning_gn_box_step(c["msg"], K, lr, damping, c["lo"], c["hi"], c["scale"], c["radius"], c["theta"], **kw)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_box_step_matches_enumeration_of_active_sets(K):
    """All 3^K active sets in numpy on correlated problems.  `released` counts the seeds whose optimal active set is not the set of entries
    the unconstrained step violates: clipping the Newton step (or fixing what it violates) gives another point there."""
    from mpc4rl_amd import qlearning_gn_box_step
    seeds = 40 if K < 5 else 16
    released = 0
    for seed in range(seeds):
        H, bb, l, u = correlated_problem(K, seed)
        msg = message(H, bb, 1)
        delta, active, info, it = qlearning_gn_box_step(msg, K, 1.0, 0.0, l, u, np.ones(K), np.inf, np.zeros(K), with_iterations=True)
        assert info == 0 and 1 <= it <= 3 * K + 1
        Hh, g = h_of(msg, K, 0.0)
        ref, ref_active = brute_force(Hh, g, l, u)
        certificate(msg, K, 1.0, 0.0, l, u, delta.numpy(), active.numpy(), f"K {K} seed {seed}")
        assert np.array_equal(active.numpy(), ref_active), (K, seed)
        on = ref_active != 0
        assert np.array_equal(delta.numpy()[on], ref[on])
        if (~on).any():
            F = np.nonzero(~on)[0]
            assert np.linalg.norm(delta.numpy()[F] - ref[F]) <= 8 * K * (K + 1) * EPS * np.linalg.cond(Hh[np.ix_(F, F)]) * np.linalg.norm(ref[F])
        z = np.linalg.solve(Hh, g)
        violated = np.where(z < l, 1, np.where(z > u, 2, 0))
        released += int(not np.array_equal(violated, ref_active))
    print(f"K {K}: the optimal active set is not the violated set in {released} of {seeds} seeds")
    if K >= 3:
        assert 4 * released >= seeds


def _problem(K, seed):
    rng = np.random.default_rng(seed)
    M = 4 * K + 3
    g = rng.normal(size=(M, K)) * 10.0 ** rng.uniform(-2, 2, K)
    A = rng.normal(size=(K, K)) / math.sqrt(K) + np.eye(K)          # correlated sensitivities
    g = g @ A
    td = rng.normal(size=M)
    return g.T @ g, g.T @ td, M


@pytest.mark.parametrize("K", [1, 2, 17, 64])
def test_box_step_kkt_certificate(K):
    from mpc4rl_amd import qlearning_gn_step
    from mpc4rl_amd.qlearning import gn_box_iteration_cap
    lr, damping = 0.8, 1e-3
    G, b, M = _problem(K, K)
    cases = make_cases(G, b, M, K, lr, damping, seed=K)
    assert [c["name"] for c in cases] == ["unbounded", "loose", "tiny radius", "mix", "l = u", "theta outside", "on a bound"]
    for c in cases:
        what = f"K {K} {c['name']}"
        delta, active, info, it = _box_step(c, K, lr, damping, with_iterations=True)
        l, u = box_of(c["lo"], c["hi"], c["scale"], c["radius"], c["theta"])
        assert info == 0 and 1 <= it < gn_box_iteration_cap(K), what
        print(f"{what}: {it} iterations")
        certificate(c["msg"], K, lr, damping, l, u, delta.numpy(), active.numpy(), what)
        new = c["theta"] + delta.numpy()
        new = np.minimum(np.maximum(new, c["lo"]), c["hi"])
        assert (c["lo"] <= new).all() and (new <= c["hi"]).all()
        if c["expect"] == "free":
            ref, info0 = qlearning_gn_step(c["msg"], K, lr, damping)
            H, _ = h_of(c["msg"], K, damping)
            assert info0 == 0 and int(active.sum()) == 0
            assert float((delta - ref).norm()) <= 8 * K * (K + 1) * EPS * np.linalg.cond(H) * float(ref.norm()), what
        if c["expect"] == "all":
            assert int((active != 0).sum()) == K, what
        if c["name"] == "mix" and K > 2:
            assert 0 < int((active != 0).sum()) < K, what
        if c["name"] == "theta outside":
            assert (l > 0).any() and (K < 2 or (u < 0).any())
        if c["name"] == "l = u":
            assert (l == u).sum() == 1 and int(active[l == u]) != 0
    # an unconstrained solution that lies on a bound of a dense problem, exactly in this arithmetic: the step's own figure as the bound
    c = dict(cases[0])
    d0 = _box_step(c, K, lr, damping)[0].numpy()
    t = int(np.argmax(np.abs(d0)))
    c["scale"], c["radius"] = np.where(np.arange(K) == t, np.abs(d0[t]), 10 * np.abs(d0).max()), 1.0
    delta, active, info = _box_step(c, K, lr, damping)
    l, u = box_of(c["lo"], c["hi"], c["scale"], c["radius"], c["theta"])
    assert info == 0 and (d0[t] == l[t] or d0[t] == u[t])
    certificate(c["msg"], K, lr, damping, l, u, delta.numpy(), active.numpy(), f"K {K} on a bound (dense)")
    assert np.array_equal(delta.numpy(), d0)


def test_box_step_info_codes():
    from mpc4rl_amd import qlearning_gn_box_step
    rng = np.random.default_rng(0)
    K, M = 5, 40
    g = rng.normal(size=(M, K))
    td = rng.normal(size=M)
    G, b = g.T @ g, g.T @ td
    one, inf, th = np.ones(K), np.full(K, np.inf), rng.normal(size=K)

    def refused(out, code):
        delta, active, info = out
        assert info == code and float(delta.abs().sum()) == 0.0 and int(active.sum()) == 0

    refused(qlearning_gn_box_step(message(G, b, 0), K, 1.0, 1e-3, -inf, inf, one, 0.1, th), -1)
    lo, hi = th - 1.0, th + 1.0
    lo[3] = th[3] + 0.5                                             # l_3 = 0.5 > u_3 = 0.1
    refused(qlearning_gn_box_step(message(G, b, M), K, 1.0, 1e-3, lo, hi, one, 0.1, th), -2)
    lo[3] = np.nan
    refused(qlearning_gn_box_step(message(G, b, M), K, 1.0, 1e-3, lo, hi, one, 0.1, th), -2)
    g[:, 3] = 0.0                                                   # singular G, damping 0: pivot 3
    refused(qlearning_gn_box_step(message(g.T @ g, g.T @ td, M), K, 1.0, 0.0, -inf, inf, one, 0.1, th), 4)
    delta, active, info = qlearning_gn_box_step(message(g.T @ g, g.T @ td, M), K, 1.0, 1e-3, -inf, inf, one, 0.1, th)
    assert info == 0 and float(delta[3]) == 0.0
    with pytest.raises(ValueError):
        qlearning_gn_box_step(message(G, b, M), K, 1.0, 1e-3, -inf, inf, one, 0.0, th)
    with pytest.raises(ValueError):
        qlearning_gn_box_step(message(G, b, M), K, 1.0, 1e-3, -inf, inf, one, float("nan"), th)
    with pytest.raises(ValueError):
        qlearning_gn_box_step(message(G, b, M), K, 1.0, 1e-3, -inf[:3], inf, one, 0.1, th)


def test_box_step_is_covariant_under_parameter_rescaling():
    """Parameters measured in other units, p_a -> D_a p_a with D_a = 2^k (exact): the sensitivities scale by 1 / D_a, and lo, hi, scale and
    theta by D_a.  The step scales by D_a within the solve bound (on both sides) and the active set is the same."""
    lr, damping, K = 0.8, 1e-3, 17
    G, b, M = _problem(K, 3)
    rng = np.random.default_rng(1)
    D = 2.0 ** rng.integers(-20, 21, K)
    D[0], D[1] = 2.0 ** -20, 2.0 ** 20
    for c in make_cases(G, b, M, K, lr, damping, seed=5)[1:6]:
        base, act0, info0 = _box_step(c, K, lr, damping)
        H, _ = h_of(c["msg"], K, damping)
        Gs, bs = G / np.outer(D, D), b / D
        s = dict(c, msg=message(Gs, bs, M), lo=c["lo"] * D, hi=c["hi"] * D, scale=c["scale"] * D, theta=c["theta"] * D)
        scaled, act1, info1 = _box_step(s, K, lr, damping)
        assert info0 == 0 == info1
        assert torch.equal(act0, act1), c["name"]
        F = np.nonzero(act0.numpy() == 0)[0]
        on = act0.numpy() != 0
        back = scaled.numpy() / D
        assert np.array_equal(back[on], base.numpy()[on]), c["name"]       # a bound scales exactly
        if F.size:
            err = np.linalg.norm((back - base.numpy())[F])
            bound = 2 * 8 * K * (K + 1) * EPS * np.linalg.cond(H[np.ix_(F, F)]) * np.linalg.norm(base.numpy()[F])
            print(f"{c['name']}: active {int(on.sum())}, deviation {err:.3e}, bound {bound:.3e}")
            assert err <= bound, c["name"]


def test_constructor_checks_of_bounds_and_trust_region_come_before_the_device_check():
    from mpc4rl_amd import (BatchedCartPoleSwingUpEnv, BatchedChainMassEnv, BatchedLinearSystemEnv, CartpoleQLearning, ChainQLearning,
                            LinearQLearning, cartpole_ocp, chain_mass_ocp, chain_theta_bounds, linear_system_ocp)
    from mpc4rl_amd.problems import chain_param_layout
    cases = [(CartpoleQLearning, cartpole_ocp(), BatchedCartPoleSwingUpEnv(4, device="cpu")),
             (LinearQLearning, linear_system_ocp(), BatchedLinearSystemEnv(4, device="cpu"))]
    chain = chain_mass_ocp(n_mass=3, N=10)
    cases.append((ChainQLearning, chain, BatchedChainMassEnv(4, chain, device="cpu")))
    for cls, ocp, env in cases:
        n_p = ocp.n_p
        lo, hi, one = torch.full((n_p,), -1.0, dtype=torch.float64), torch.full((n_p,), 1.0, dtype=torch.float64), torch.ones(n_p, dtype=torch.float64)
        gn = dict(method="gauss_newton")
        bad_scale = one.clone()
        bad_scale[n_p - 1] = 0.0
        for kw in (dict(gn, trust_radius=0.0), dict(gn, trust_radius=-1.0), dict(gn, trust_radius=float("nan")), dict(gn, trust_radius="0.1"),
                   dict(gn, theta_bounds=(lo[:-1], hi)), dict(gn, theta_bounds=(hi, lo)), dict(gn, theta_bounds=lo),
                   dict(gn, theta_bounds=(lo * float("nan"), hi)), dict(gn, theta_scale=one[:-1]), dict(gn, theta_scale=bad_scale),
                   dict(gn, theta_scale=one * float("inf")), dict(gn, theta_scale=-one),
                   dict(trust_radius=0.1), dict(method="gradient", theta_bounds=(lo, hi)), dict(method="gradient", theta_scale=one)):
            with pytest.raises(ValueError):
                cls(ocp, env, 6, **kw)
        for kw in (dict(gn, trust_radius=0.05), dict(gn, theta_bounds=(lo, hi)), dict(gn, theta_scale=one),
                   dict(gn, trust_radius=float("inf"), theta_bounds=(lo, lo), theta_scale=one)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):    # valid arguments, CPU environment: refused, never emulated
                cls(ocp, env, 6, **kw)
    lo, hi = chain_theta_bounds(chain)
    off = chain_param_layout(3)[4]
    p0 = torch.as_tensor(chain.p0, dtype=torch.float64)
    bounded = torch.zeros(chain.n_p, dtype=torch.bool)
    for key in ("m", "D"):
        bounded[off[key][0]: off[key][1]] = True
    assert lo.shape == hi.shape == (chain.n_p,) and lo.dtype == torch.float64
    assert torch.equal(lo[bounded], 0.5 * p0[bounded]) and torch.equal(hi[bounded], 1.5 * p0[bounded]) and bool((lo[bounded] > 0).all())
    assert bool(torch.isinf(lo[~bounded]).all()) and bool(torch.isinf(hi[~bounded]).all())
    lo, hi = chain_theta_bounds(chain, rel=0.1)
    assert torch.equal(lo[bounded], (1.0 - 0.1) * p0[bounded])
    with pytest.raises(ValueError):
        chain_theta_bounds(chain, rel=1.0)
