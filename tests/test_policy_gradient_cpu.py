"""CPU checks of the deterministic policy gradient with a compatible critic (mpc4rl_amd/policy_gradient.py): the C ABI's new symbols,
the torch statements ``cdpg_terms`` and ``cdpg_step`` of the kernels against a plain loop over the terms and against a planted
solution, the step's covariance under a rescaling of the parameters, every info code and the clip, and the constructors' checks.

Bounds (derived, not measured), eps = 2^-53:
  sums   |G_ac - G_exact,ac| <= (4 M + 2 nu + 2) eps sum_j (|J|'|d|)_ja (|J|'|d|)_jc over the M terms: 4 M eps for a sum of M products in
         any order, and each psi_ja carries nu products and nu - 1 sums of its own, (1 + eps)^(2 nu) on each factor at most, measured
         against |J|'|d| >= |psi|; likewise b with |delta_j| (|J|'|d|)_ja; M_ac within 4 (M nu) eps sum |J_jc'a J_jc'c| (M nu rows);
  solve  ||w - w_ref||_2 <= 8 K (K + 1) eps cond_2(H) ||w_ref||_2 (backward stability of Cholesky, on both sides); the plain gradient
         (M/n) w inherits it times ||M/n||_2, plus K eps ||M/n||_2 ||w|| for the product, which the same constant covers."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcrl_cdpg_record", "mpcrl_cdpg_workspace_bytes", "mpcrl_cdpg_terms", "mpcrl_cdpg_apply"]
EPS = 2.0 ** -53


def test_new_symbols_in_header_binding_and_library():
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    api = open(os.path.join(ROOT, "mpc4rl_amd", "csrc", "mpcrl_loops.hip")).read()
    declared = sorted(set(re.findall(r"\b(mpcrl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))   # as tests/test_cabi.py reads it
    assert sorted(_lib.EXPORTS) == declared
    for name in NEW:
        assert name in declared, name
        assert re.search(r"\b" + name + r"\(", api), name
        assert name in _lib.EXPORTS, name
    assert int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 132    # additions do not bump it
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = _lib.load()
    for name in NEW:
        getattr(lib, name)


def make_tables(T, E, nu, K, seed, prefixes=(0, 1, 2, 3)):
    """Episode tables with every kind of term: live prefixes of the given lengths and T, failed solves, and NaN in J, v and u0 of every row
    that is dead or failed."""
    rng = np.random.default_rng(seed)
    L = np.full(E, T)
    L[: len(prefixes)] = prefixes
    live = (np.arange(T)[:, None] < L[None, :]).astype(np.uint8)
    cost = rng.uniform(0, 5, (T, E))
    v = rng.normal(size=(T, E))
    u0 = rng.normal(size=(T, E, nu))
    act = u0 + 0.1 * rng.normal(size=(T, E, nu))
    J = rng.normal(size=(T, E, nu, K)) * 10.0 ** rng.integers(-2, 3, K)
    status = np.where(rng.uniform(size=(T, E)) < 0.15, rng.choice([1, 2, 4], size=(T, E)), 0).astype(np.int32)
    status[:, E - 1] = 0                                            # one environment whose terms are all valid
    bad = (status != 0) | (live == 0)
    v[bad], u0[bad], J[bad] = np.nan, np.nan, np.nan
    return v, u0, J, status, act, cost, live


def loop_terms(v, u0, J, status, act, cost, live, gamma):
    """A plain loop over the terms: delta and psi as the statement rounds them, exact sums (math.fsum) of the valid terms' products and
    the sums that the bounds are made of."""
    T, E = cost.shape
    nu, K = J.shape[2], J.shape[3]
    delta, valid = np.zeros((max(T - 2, 0), E)), np.zeros((max(T - 2, 0), E), dtype=bool)
    tri = [(a, c) for a in range(K) for c in range(a, K)]
    Gp, Ga, Mp, Ma = ({k: [] for k in tri} for _ in range(4))
    bp, ba = ({a: [] for a in range(K)} for _ in range(2))
    for i in range(T - 2):
        for e in range(E):
            if not (live[i, e] and live[i + 1, e] and live[i + 2, e] and status[i, e] == 0 and status[i + 1, e] == 0):
                continue
            valid[i, e] = True
            t = gamma * v[i + 1, e]
            t = cost[i, e] + t
            delta[i, e] = t - v[i, e]
            d = act[i, e] - u0[i, e]
            Jn = np.nan_to_num(J[i, e])
            psi = Jn[0] * d[0]
            for c in range(1, nu):
                psi = psi + Jn[c] * d[c]
            pa = np.abs(Jn).T @ np.abs(d)
            for a in range(K):
                bp[a].append(delta[i, e] * psi[a]), ba[a].append(abs(delta[i, e]) * pa[a])
                for c in range(a, K):
                    Gp[(a, c)].append(psi[a] * psi[c]), Ga[(a, c)].append(pa[a] * pa[c])
                    for q in range(nu):
                        Mp[(a, c)].append(Jn[q, a] * Jn[q, c]), Ma[(a, c)].append(abs(Jn[q, a] * Jn[q, c]))
    s = lambda dct, keys: np.array([math.fsum(dct[k]) for k in keys])
    return dict(delta=delta, valid=valid, G=s(Gp, tri), Gabs=s(Ga, tri), b=s(bp, range(K)), babs=s(ba, range(K)), M=s(Mp, tri), Mabs=s(Ma, tri),
                sd=math.fsum(delta[valid]), sdabs=math.fsum(np.abs(delta[valid])))


def _t(arrs):
    return [torch.as_tensor(a) for a in arrs]


@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("nu", [1, 3])
def test_cdpg_terms_match_a_plain_loop(nu, K):
    from mpc4rl_amd import cdpg_terms
    T, E, gamma = 7, 9, 0.97
    d = make_tables(T, E, nu, K, 10 * nu + K)
    msg, delta, valid = cdpg_terms(*_t(d), gamma)
    ref = loop_terms(*d, gamma)
    KK, M = K * (K + 1) // 2, (T - 2) * E
    assert msg.shape == (K * (K + 1) + K + 2,) and torch.isfinite(msg).all()
    assert np.array_equal(valid.numpy(), ref["valid"]) and np.array_equal(delta.numpy(), ref["delta"])       # exact: the same roundings
    # prefixes 0 .. 2 give no term, 3 at most the first (its solves may have failed), the all-valid column every one
    assert not ref["valid"][:, :3].any() and not ref["valid"][1:, 3].any() and ref["valid"][:, E - 1].all()
    assert 0 < ref["valid"].sum() < M and int(msg[-1]) == ref["valid"].sum()
    m = msg.numpy()
    f = (4 * M + 2 * nu + 2) * EPS
    assert (np.abs(m[:KK] - ref["G"]) <= f * ref["Gabs"]).all()
    assert (np.abs(m[KK: KK + K] - ref["b"]) <= f * ref["babs"]).all()
    assert (np.abs(m[KK + K: 2 * KK + K] - ref["M"]) <= 4 * M * nu * EPS * ref["Mabs"]).all()
    assert abs(m[2 * KK + K] - ref["sd"]) <= 4 * M * EPS * ref["sdabs"]
    # the packing of both triangles: entry (a, c), a <= c, sits at a K - a (a - 1) / 2 + (c - a); G at 0, M at KK + K
    Jn = np.nan_to_num(d[2])
    dd = d[4] - d[1]
    for a, c in {(0, 0), (0, K - 1), (K - 1, K - 1), (K // 2, K - 1)}:
        at = a * K - a * (a - 1) // 2 + (c - a)
        Mac = math.fsum(Jn[i, e, q, a] * Jn[i, e, q, c] for i, e in zip(*np.nonzero(ref["valid"])) for q in range(nu))
        assert abs(m[KK + K + at] - Mac) <= 4 * M * nu * EPS * ref["Mabs"][at]
        psi = lambda i, e, k: math.fsum(Jn[i, e, q, k] * dd[i, e, q] for q in range(nu))
        Gac = math.fsum(psi(i, e, a) * psi(i, e, c) for i, e in zip(*np.nonzero(ref["valid"])))
        assert abs(m[at] - Gac) <= f * ref["Gabs"][at]


def test_cdpg_terms_liveness_prefix_of_the_whole_episode_and_one_control_tables():
    """A live prefix of length T gives T - 2 terms, of 3 one, of 0 .. 2 none; A and u0 of a one-control plant may come as [T, E]."""
    from mpc4rl_amd import cdpg_terms
    T, E, K = 6, 5, 3
    v, u0, J, status, act, cost, live = make_tables(T, E, 1, K, 3)
    status[:] = 0
    msg, delta, valid = cdpg_terms(*_t((v, u0, J, status, act, cost, live)), 0.9)
    assert valid.sum(0).tolist() == [0, 0, 0, 1, T - 2]
    msg2 = cdpg_terms(*_t((v, u0[..., 0], J, status, act[..., 0], cost, live)), 0.9)[0]
    assert torch.equal(msg, msg2)
    empty = cdpg_terms(*_t([a[:2] for a in (v, u0, J, status, act, cost, live)]), 0.9)       # T = 2: no term
    assert float(empty[0].abs().sum()) == 0.0 and empty[1].shape == (0, E)


def test_cdpg_message_is_additive_over_environments():
    from mpc4rl_amd import cdpg_terms
    T, E, nu, K, gamma = 6, 10, 3, 4, 0.99
    d = make_tables(T, E, nu, K, 11)
    whole = cdpg_terms(*_t(d), gamma)[0].numpy()
    parts = [cdpg_terms(*_t([a[:, sl] for a in d]), gamma)[0].numpy() for sl in (slice(0, 5), slice(5, E))]
    ref = loop_terms(*d, gamma)
    M = (T - 2) * E
    bound = np.concatenate([(4 * M + 2 * nu + 2) * EPS * ref["Gabs"], (4 * M + 2 * nu + 2) * EPS * ref["babs"], 4 * M * nu * EPS * ref["Mabs"],
                            [4 * M * EPS * ref["sdabs"]], [0.0]])
    got = parts[0] + parts[1]
    assert got[-1] == whole[-1] == ref["valid"].sum()
    assert (np.abs(got - whole) <= 2 * bound).all()                 # each side is within `bound` of the exact sums


# ---------------------------------------------------------------------- the step
def _message(G, b, Mm, count, sd=0.0):
    iu = np.triu_indices(G.shape[0])
    return torch.as_tensor(np.concatenate([G[iu], b, Mm[iu], [sd], [float(count)]]))


def _planted(K, seed, kappa_spread=2.0):
    """psi, w* and delta = psi' w* with small integers, so that G, b = G w* and delta are exact; M from integer rows too."""
    rng = np.random.default_rng(seed)
    n = 4 * K + 3
    psi = rng.integers(-4, 5, (n, K)).astype(np.float64)
    psi[:K] += 6.0 * np.eye(K)                                      # well conditioned
    w = rng.integers(-5, 6, K).astype(np.float64)
    w[0] = 3.0
    Jr = rng.integers(-3, 4, (2 * n, K)).astype(np.float64)
    return psi.T @ psi, psi.T @ (psi @ w), Jr.T @ Jr, n, w


@pytest.mark.parametrize("natural", [True, False])
@pytest.mark.parametrize("K", [1, 3, 17, 64])
def test_cdpg_step_returns_the_planted_critic(K, natural):
    """delta = psi' w* planted exactly, damping 0: w = w* within the Cholesky bound, and the step is -lr w or -lr (M/n) w."""
    from mpc4rl_amd import cdpg_step
    G, b, Mm, n, w_star = _planted(K, K)
    lr = 0.25
    step, w, active, info = cdpg_step(_message(G, b, Mm, n), K, lr, 0.0, natural)
    cond = np.linalg.cond(G / n)
    bound = 8 * K * (K + 1) * EPS * cond * np.linalg.norm(w_star)
    err = np.linalg.norm(w.numpy() - w_star)
    print(f"K {K} natural {natural}: |w - w*| {err:.3e}, bound {bound:.3e}")
    assert info == 0 and int(active.sum()) == 0
    assert err <= bound
    ref = -lr * w_star if natural else -lr * (Mm / n) @ w_star
    scale = 1.0 if natural else np.linalg.norm(Mm / n, 2)
    assert np.linalg.norm(step.numpy() - ref) <= lr * scale * bound


def test_cdpg_step_is_covariant_under_parameter_rescaling():
    """Scaling column a of du0/dp by s_a = 2^k, k in -20 .. 20 (a parameter measured in other units), scales w_a and the natural step by
    1 / s_a (a vector); the plain gradient by s_a (a covector)."""
    from mpc4rl_amd import cdpg_step, cdpg_terms
    T, E, nu, K, gamma = 6, 9, 3, 6, 0.99
    d = list(make_tables(T, E, nu, K, 3))
    k = np.random.default_rng(1).integers(-20, 21, K)
    k[0], k[1] = -20, 20                                            # both ends of the range
    s = 2.0 ** k
    base = {nat: cdpg_step(cdpg_terms(*_t(d), gamma)[0], K, 0.7, 1e-3, nat) for nat in (True, False)}
    d[2] = d[2] * s
    scaled = {nat: cdpg_step(cdpg_terms(*_t(d), gamma)[0], K, 0.7, 1e-3, nat) for nat in (True, False)}
    st = torch.as_tensor(s)
    for nat in (True, False):
        assert base[nat][3] == 0 == scaled[nat][3] and float(base[nat][0].abs().min()) > 0.0
        rel_w = (scaled[nat][1] * st - base[nat][1]).abs() / base[nat][1].abs()
        rel_s = ((scaled[nat][0] * st if nat else scaled[nat][0] / st) - base[nat][0]).abs() / base[nat][0].abs()
        print(f"covariance, natural {nat}: max relative deviation w {float(rel_w.max()):.2e}, step {float(rel_s.max()):.2e}")
        assert float(rel_w.max()) <= 1e-12 and float(rel_s.max()) <= 1e-12


def test_cdpg_step_info_codes():
    from mpc4rl_amd import cdpg_step
    rng = np.random.default_rng(0)
    K, n = 5, 40
    psi = rng.normal(size=(n, K))
    psi[:, 3] = 0.0                                                 # an entry no term is sensitive to: a zero row and column of G
    dl = rng.normal(size=n)
    G, b, Mm = psi.T @ psi, psi.T @ dl, np.eye(K)
    step, w, active, info = cdpg_step(_message(G, b, Mm, n), K, 1.0, 0.0, True)
    assert info == 4 and float(step.abs().sum()) == 0.0 == float(w.abs().sum()) and int(active.sum()) == 0      # pivot 3, 1-based
    step, w, active, info = cdpg_step(_message(G, b, Mm, n), K, 1.0, 1e-3, True)
    assert info == 0 and float(step[3]) == 0.0 and float(step.abs().sum()) > 0.0
    for msg in (_message(G, b, Mm, 0), _message(np.zeros((K, K)), b, Mm, n), _message(np.where(np.eye(K) > 0, np.nan, G), b, Mm, n)):
        step, w, active, info = cdpg_step(msg, K, 1.0, 1e-3, False)
        assert info == -1 and float(step.abs().sum()) == 0.0 == float(w.abs().sum())
    th = np.zeros(K)
    for kw in (dict(lo=np.full(K, 1.0), hi=np.full(K, -1.0)), dict(lo=np.array([np.nan] + [-1.0] * (K - 1))),
               dict(hi=np.full(K, 5.0), scale=np.array([np.nan] + [1.0] * (K - 1)), radius=1.0)):
        step, w, active, info = cdpg_step(_message(G, b, Mm, n), K, 1.0, 1e-3, True, theta_idx=th, **kw)
        assert info == -2 and float(step.abs().sum()) == 0.0 and int(active.sum()) == 0
    with pytest.raises(ValueError):
        cdpg_step(_message(G, b, Mm, n), K, 1.0, 1e-3, True, radius=0.0)


def test_cdpg_step_clip_and_active():
    """The clip is entrywise: an entry outside its interval takes the interval's end bit for bit, the others are the free step's."""
    from mpc4rl_amd import cdpg_step
    K = 6
    G, b, Mm, n, w_star = _planted(K, 2)
    msg = _message(G, b, Mm, n)
    for natural in (True, False):
        free = cdpg_step(msg, K, 0.5, 1e-3, natural)[0]
        assert float(free.abs().min()) > 0.0
        th = torch.linspace(-1.0, 1.0, K, dtype=torch.float64)
        lo, hi = th - 0.5 * free.abs(), th + 2.0 * free.abs()                   # a step down is cut to half of itself, a step up is free
        lo[0], hi[0] = -math.inf, math.inf
        step, w, active, info = cdpg_step(msg, K, 0.5, 1e-3, natural, lo=lo, hi=hi, theta_idx=th)
        want = torch.where(free < lo - th, 1, torch.where(free > hi - th, 2, 0))
        want[0] = 0
        assert info == 0 and torch.equal(active.to(torch.int64), want) and bool((active == 1).any())
        assert torch.equal(step[active == 0], free[active == 0]) and torch.equal(step[active == 1], (lo - th)[active == 1])
        # the trust region alone: |step_a| <= radius scale_a, the ends bit for bit; scale defaults to 1
        sc = free.abs() * torch.tensor([0.5, 2.0] * (K // 2), dtype=torch.float64)
        step, w2, active, info = cdpg_step(msg, K, 0.5, 1e-3, natural, scale=sc, radius=1.0)
        assert info == 0 and torch.equal(w2, w)
        assert active.tolist() == [(1 if float(free[a]) < 0 else 2) if a % 2 == 0 else 0 for a in range(K)]
        assert torch.equal(step[0::2].abs(), sc[0::2]) and torch.equal(step[1::2], free[1::2])
        step, _, active, info = cdpg_step(msg, K, 0.5, 1e-3, natural, radius=float(free.abs().max()) * 2)
        assert info == 0 and int(active.sum()) == 0 and torch.equal(step, free)


# ---------------------------------------------------------------------- the learners' constructors
def test_constructor_checks_come_before_the_device_check():
    from mpc4rl_amd import (BatchedCartPoleSwingUpEnv, BatchedChainMassEnv, BatchedLinearSystemEnv, CartpolePolicyGradient, ChainPolicyGradient,
                            LinearPolicyGradient, cartpole_ocp, chain_mass_ocp, chain_theta_bounds, linear_system_ocp)
    cases = [(CartpolePolicyGradient, cartpole_ocp(), BatchedCartPoleSwingUpEnv(4, device="cpu")),
             (LinearPolicyGradient, linear_system_ocp(), BatchedLinearSystemEnv(4, device="cpu"))]
    ocp = chain_mass_ocp(n_mass=3, N=10)
    cases.append((ChainPolicyGradient, ocp, BatchedChainMassEnv(4, ocp, device="cpu")))
    for cls, ocp, env in cases:
        for kw in (dict(noise_scale=0.0), dict(noise_scale=-0.1), dict(noise_scale=float("nan")), dict(natural=1), dict(natural=None),
                   dict(damping=-1e-3), dict(damping=float("nan")), dict(damping="1e-3"), dict(trust_radius=0.0), dict(trust_radius=-1.0),
                   dict(theta_bounds=(torch.zeros(ocp.n_p),)), dict(theta_bounds=(torch.ones(ocp.n_p), torch.zeros(ocp.n_p))),
                   dict(theta_scale=torch.zeros(ocp.n_p)), dict(theta_scale=torch.ones(ocp.n_p + 1)), dict(lr=float("inf")), dict(gamma=1.5)):
            with pytest.raises(ValueError):
                cls(ocp, env, 6, **kw)
        with pytest.raises(ValueError):
            cls(ocp, env, 1)
        with pytest.raises(TypeError):
            cls(ocp, object(), 6)
        with pytest.raises(RuntimeError, match="no CPU fallback"):        # valid arguments, CPU environment: refused, never emulated
            cls(ocp, env, 6, natural=True, trust_radius=0.05)
    for cls in (CartpolePolicyGradient, LinearPolicyGradient):
        with pytest.raises(ValueError, match="learn_mask"):
            o = cartpole_ocp() if cls is CartpolePolicyGradient else linear_system_ocp()
            cls(o, cases[0][2] if cls is CartpolePolicyGradient else cases[1][2], 6, learn_mask=torch.ones(o.n_p + 1))
    with pytest.raises(ValueError, match="learn"):
        ChainPolicyGradient(ocp, cases[2][2], 6, learn=("m", "K"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ChainPolicyGradient(ocp, cases[2][2], 6, theta_bounds=chain_theta_bounds(ocp), trust_radius=0.02)
