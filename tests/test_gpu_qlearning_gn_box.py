"""GPU tests of the Q-learners' Gauss-Newton step inside a box and a trust region (qlearning_gn_apply_box_kernel of
csrc/qlearning_gn_kernel.hpp): mpcrl_qlearning_gn_apply_box against its torch statement ``qlearning_gn_box_step`` and against the KKT
certificate of tests/gn_box_cases.py (which does not depend on the algorithm), its info codes and argument checks, the same bits from two
launches, and LinearQLearning / ChainQLearning with a trust region and bounds end to end, eager and replayed from graphs.

Bounds (derived, not measured; eps = 2^-53): the certificate's tol_a (gn_box_cases.py), and between kernel and torch statement, on the
free block,  ||d - d_ref||_2 <= 8 K (K + 1) eps cond_2(H_FF) ||d_ref||_2  (backward stability of Cholesky, on both sides); on the active
entries the two agree bit for bit.  Every comparison prints its observed figure beside the bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gn_box_cases import agree, box_of, certificate, correlated_problem, make_cases, message

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
POISON = -7.0


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def _idx(K, spread):
    return list(range(K)) if not spread else [3 * a + 1 for a in range(K)]


def run_box(c, K, idx, n_theta, lr, damping, launches=1):
    """mpcrl_qlearning_gn_apply_box on the case c (its lo, hi, scale and theta [K] scattered to idx; NaN bounds and scales elsewhere: they are
    never read).  Checks what holds for every launch: only theta[idx] moves, step_out is 0 outside idx, theta = clamp(theta0 + step, lo, hi)
    with lo <= theta <= hi, and on a code other than 0 nothing moved.  Returns (delta [K], active [K], info [2]) of every launch, numpy."""
    lib = _lib()
    full = lambda v, fill: torch.full((n_theta,), fill, dtype=torch.float64).index_put_((torch.tensor(idx),), torch.as_tensor(np.asarray(v, dtype=np.float64)))
    lo, hi, scale = full(c["lo"], float("nan")), full(c["hi"], float("nan")), full(c["scale"], float("nan"))
    theta0 = torch.randn(n_theta, generator=torch.Generator().manual_seed(K), dtype=torch.float64)
    theta0 = theta0.index_put_((torch.tensor(idx),), torch.as_tensor(np.asarray(c["theta"], dtype=np.float64)))
    msg_d, idx_d = c["msg"].to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV)
    lo_d, hi_d, scale_d = lo.to(DEV), hi.to(DEV), scale.to(DEV)
    out = []
    for _ in range(launches):
        theta, step = theta0.to(DEV), torch.full((n_theta,), POISON, **F64)
        active, info = torch.full((K,), 9, dtype=torch.uint8, device=DEV), torch.full((2,), 77, dtype=torch.int32, device=DEV)
        rc = lib.mpcrl_qlearning_gn_apply_box(_p(msg_d), K, _p(idx_d), n_theta, lr, damping, _p(lo_d), _p(hi_d), _p(scale_d), float(c["radius"]),
                                              _p(theta), _p(step), _p(active), _p(info), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        step, theta, info = step.cpu(), theta.cpu(), info.cpu().tolist()
        off = torch.ones(n_theta, dtype=torch.bool)
        off[idx] = False
        assert float(step[off].abs().sum()) == 0.0 and torch.equal(theta[off], theta0[off])
        if info[0] == 0:
            want = torch.minimum(torch.maximum(theta0[idx] + step[idx], lo[idx]), hi[idx])
            assert torch.equal(theta[idx], want)
            assert bool((lo[idx] <= theta[idx]).all()) and bool((theta[idx] <= hi[idx]).all())
        else:
            assert torch.equal(theta, theta0) and float(step.abs().sum()) == 0.0 and int(active.sum()) == 0
        out.append((step[idx].numpy(), active.cpu().numpy(), info))
    return out


@functools.lru_cache(maxsize=None)
def _cases(K, kappa):
    """H = Q diag(ev) Q' with cond_2 = kappa as test_gn_apply_matches_solve builds it (K = 1: a scalar), count 37, damping 1e-3; the boxes
    of every kind and the torch statement's answer to each, computed once for both layouts of idx."""
    from mpc4rl_amd import qlearning_gn_box_step
    rng = np.random.default_rng(K)
    Qm = np.linalg.qr(rng.normal(size=(K, K)))[0]
    ev = np.logspace(0, -np.log10(kappa), K) if K > 1 else np.array([0.3])
    H = (Qm * ev) @ Qm.T
    H = 0.5 * (H + H.T)
    n, lr, damping = 37, 0.8, 1e-3
    b = rng.normal(size=K)
    cases = make_cases(H * n, b * n, n, K, lr, damping, seed=K)
    for c in cases:
        c["ref"] = qlearning_gn_box_step(c["msg"], K, lr, damping, c["lo"], c["hi"], c["scale"], c["radius"], c["theta"])
    return cases, lr, damping


@pytest.mark.parametrize("spread", [False, True], ids=["np=K", "np=3K+1"])
@pytest.mark.parametrize("kappa", [1e2, 1e6])
@pytest.mark.parametrize("K", [1, 2, 16, 17, 40, 64])
def test_box_kernel_matches_torch_form_and_certificate(K, kappa, spread):
    from mpc4rl_amd.qlearning import gn_box_iteration_cap
    cases, lr, damping = _cases(K, kappa)
    idx, n_theta = _idx(K, spread), (3 * K + 1 if spread else K)
    for c in cases:
        what = f"K {K} kappa {kappa:g} n_p {n_theta} {c['name']}"
        (delta, active, info), = run_box(c, K, idx, n_theta, lr, damping)
        ref, ref_active, ref_info = c["ref"]
        print(f"{what}: info {info}")
        assert info[0] == 0 == ref_info and 1 <= info[1] < gn_box_iteration_cap(K), what
        l, u = box_of(c["lo"], c["hi"], c["scale"], c["radius"], c["theta"])
        certificate(c["msg"], K, lr, damping, l, u, delta, active, what)
        agree(delta, active, ref.numpy(), ref_active.numpy(), c["msg"], K, damping, what)
        if c["expect"] == "free":
            assert int(active.sum()) == 0 and info[1] == 1
        if c["expect"] == "all":
            assert int((active != 0).sum()) == K


@pytest.mark.parametrize("K", [3, 5])
def test_box_kernel_on_correlated_problems(K):
    """The seeds of the CPU enumeration test (H = A' A, a box of +-0.3): the optimal active set is often not what the unconstrained step
    violates, so entries have to be released."""
    from mpc4rl_amd import qlearning_gn_box_step
    from mpc4rl_amd.qlearning import gn_box_iteration_cap
    released = 0
    for seed in range(12):
        H, bb, l, u = correlated_problem(K, seed)
        c = dict(msg=message(H, bb, 1), lo=l, hi=u, scale=np.ones(K), radius=np.inf, theta=np.zeros(K))
        (delta, active, info), = run_box(c, K, _idx(K, True), 3 * K + 1, 1.0, 0.0)
        ref, ref_active, ref_info = qlearning_gn_box_step(c["msg"], K, 1.0, 0.0, l, u, c["scale"], np.inf, c["theta"])
        what = f"K {K} seed {seed}"
        assert info[0] == 0 == ref_info and 1 <= info[1] < gn_box_iteration_cap(K), what
        certificate(c["msg"], K, 1.0, 0.0, l, u, delta, active, what)
        agree(delta, active, ref.numpy(), ref_active.numpy(), c["msg"], K, 0.0, what)
        z = np.linalg.solve(H, bb)
        released += int(not np.array_equal(np.where(z < l, 1, np.where(z > u, 2, 0)), active))
    print(f"K {K}: the optimal active set is not the violated set in {released} of 12 seeds")
    assert released > 0


def test_box_kernel_info_codes_and_argument_checks():
    lib = _lib()
    rng = np.random.default_rng(0)
    K, M = 5, 40
    g = rng.normal(size=(M, K))
    td = rng.normal(size=M)
    G, b = g.T @ g, g.T @ td
    idx, n_theta = _idx(K, True), 3 * K + 1
    th, inf, one = rng.normal(size=K), np.full(K, np.inf), np.ones(K)
    base = dict(msg=message(G, b, M), lo=-inf, hi=inf, scale=one, radius=0.1, theta=th)
    assert run_box(base, K, idx, n_theta, 1.0, 1e-3)[0][2][0] == 0
    assert run_box(dict(base, msg=message(G, b, 0)), K, idx, n_theta, 1.0, 1e-3)[0][2] == [-1, 0]
    lo, hi = th - 1.0, th + 1.0
    lo[3] = th[3] + 0.5                                             # l_3 = 0.5 > u_3 = 0.1
    assert run_box(dict(base, lo=lo, hi=hi), K, idx, n_theta, 1.0, 1e-3)[0][2] == [-2, 0]
    lo2 = lo.copy()
    lo2[3] = np.nan
    assert run_box(dict(base, lo=lo2, hi=hi), K, idx, n_theta, 1.0, 1e-3)[0][2] == [-2, 0]
    g[:, 3] = 0.0                                                   # singular G, damping 0: pivot 3
    sing = dict(base, msg=message(g.T @ g, g.T @ td, M))
    assert run_box(sing, K, idx, n_theta, 1.0, 0.0)[0][2] == [4, 0]
    (delta, active, info), = run_box(sing, K, idx, n_theta, 1.0, 1e-3)
    assert info[0] == 0 and delta[3] == 0.0
    # the host's checks: nothing is launched
    z = torch.zeros(3 * 64 + 8, **F64)
    i32 = torch.arange(65, dtype=torch.int32, device=DEV)
    u8, inf32 = torch.zeros(64, dtype=torch.uint8, device=DEV), torch.full((2,), 77, dtype=torch.int32, device=DEV)
    good = dict(msg=_p(z), K=3, idx=_p(i32), n_theta=10, lr=1.0, damping=1e-3, lo=_p(z), hi=_p(z), scale=_p(z), radius=0.1, theta=_p(z), step_out=_p(z),
                active=_p(u8), info=_p(inf32))

    def call(**kw):
        a = dict(good, **kw)
        return lib.mpcrl_qlearning_gn_apply_box(a["msg"], a["K"], a["idx"], a["n_theta"], a["lr"], a["damping"], a["lo"], a["hi"], a["scale"], a["radius"],
                                                a["theta"], a["step_out"], a["active"], a["info"], _stream())

    nan, big = float("nan"), float("inf")
    for kw in ([dict(K=k) for k in (0, 65, -1)] + [dict(n_theta=2)] + [{name: None} for name in ("msg", "idx", "lo", "hi", "scale", "theta", "step_out", "active", "info")]
               + [dict(radius=r) for r in (0.0, -1.0, nan)] + [dict(lr=v) for v in (nan, big, -big)] + [dict(damping=v) for v in (nan, big, -1e-3)]):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0.0
    assert call(radius=big) == 0                                   # no trust region: allowed (an all-zero message: info -1)
    torch.cuda.synchronize()
    assert inf32.tolist() == [-1, 0]


def test_box_kernel_two_launches_give_the_same_bits():
    for K, kappa in ((17, 1e6), (64, 1e2)):
        cases, lr, damping = _cases(K, kappa)
        for c in cases[2:6]:
            first, second = run_box(c, K, _idx(K, True), 3 * K + 1, lr, damping, launches=2)
            assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2], (K, c["name"])


# ---------------------------------------------------------------------- the loops
def _linear(graphs=False, **kw):
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp
    ql = LinearQLearning(linear_system_ocp(), BatchedLinearSystemEnv(8, device=DEV, seed=5), 6, noise_scale=0.1, seed=6, **kw)
    if graphs:
        ql.enable_graphs()
    return ql


def _chain(graphs=False, bounds=False, **kw):
    from mpc4rl_amd import BatchedChainMassEnv, ChainQLearning, chain_mass_ocp, chain_theta_bounds
    from mpc4rl_amd.problems import chain_param_layout
    ocp = chain_mass_ocp(3, N=10)
    off = chain_param_layout(3)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1
    p[off["D"][0]: off["D"][1]] *= 0.9
    env = BatchedChainMassEnv(4, ocp, device=DEV, p=p, w_std=0.01, vel_std=1e-2, seed=1)
    if bounds:
        kw["theta_bounds"] = chain_theta_bounds(ocp)
    ql = ChainQLearning(ocp, env, 4, noise_scale=0.05, seed=2, **kw)
    if graphs:
        ql.enable_graphs()
    return ql


def _make_bounded(name, graphs):
    return (_linear if name == "linear" else functools.partial(_chain, bounds=True))(graphs=graphs, method="gauss_newton", lr=1.0, damping=1e-3,
                                                                                    trust_radius=0.05)


@pytest.mark.parametrize("name,K", [("linear", 12), ("chain", 20)])
def test_trust_region_episodes_eager_and_from_graphs(name, K):
    """Two episodes with lr 1 and trust_radius 0.05 (the chain: inside chain_theta_bounds): no entry moves by more than 0.05 scale_a, theta
    stays in its bounds, the applied step passes the certificate on the learner's own message, and the episodes replayed from graphs, from
    the same seeds, are the same bits."""
    from mpc4rl_amd.qlearning import gn_box_iteration_cap
    runs = []
    for graphs in (False, True):
        ql = _make_bounded(name, graphs)
        kept = []
        for ep in range(2):
            theta0 = ql.theta.clone()
            st = ql.run_episode()
            torch.cuda.synchronize()
            kept += [t.clone() for t in (ql.theta, ql.msg, ql.step_out, ql.gn_active, ql.td)] + [torch.tensor([st.gn_info, st.gn_active, st.gn_iterations])]
            if graphs:
                continue
            idx = ql.learn_idx.cpu().tolist()
            assert ql.K == K == len(idx)
            lo, hi, scale = (t.cpu()[idx].numpy() for t in (ql.theta_lo, ql.theta_hi, ql.theta_scale))
            step, active = ql.step_out.cpu(), ql.gn_active.cpu().numpy()
            delta = step[idx].numpy()
            p0 = np.abs(np.asarray(ql.ocp.p0, dtype=np.float64))
            assert np.array_equal(scale, np.where(p0[idx] != 0, p0[idx], p0[idx].max()))           # the default theta_scale
            assert st.gn_info == 0 and 1 <= st.gn_iterations < gn_box_iteration_cap(K)
            assert st.gn_active == int((active != 0).sum())
            assert (np.abs(delta) <= 0.05 * scale).all()
            off = torch.ones(ql.n_p, dtype=torch.bool)
            off[idx] = False
            assert float(step[off].abs().sum()) == 0.0 and torch.equal(st.step, ql.step_out)
            new = ql.theta.cpu()
            assert torch.equal(new[off], theta0.cpu()[off])
            assert (lo <= new[idx].numpy()).all() and (new[idx].numpy() <= hi).all()
            assert np.array_equal(new[idx].numpy(), np.minimum(np.maximum(theta0.cpu()[idx].numpy() + delta, lo), hi))
            l, u = box_of(lo, hi, scale, 0.05, theta0.cpu()[idx].numpy())
            certificate(ql.msg.cpu(), K, ql.lr, ql.damping, l, u, delta, active, f"{name} episode {ep}")
            print(f"{name} episode {ep}: active {st.gn_active} of {K}, iterations {st.gn_iterations}, |step| {float(step.norm()):.3e}")
            assert torch.equal(ql.rollout_mpc.get_theta(), ql.theta) and torch.equal(ql.sample_mpc.get_theta(), ql.theta)
        runs.append(kept)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_defaults_leave_the_gauss_newton_episode_bit_for_bit():
    runs = []
    for kw in (dict(), dict(trust_radius=None, theta_bounds=None, theta_scale=None)):
        ql = _linear(method="gauss_newton", lr=0.5, damping=1e-3, **kw)
        st = ql.run_episode()
        torch.cuda.synchronize()
        assert st.gn_info == 0 and st.gn_active == 0 and st.gn_iterations == 0 and not ql.box
        runs.append([t.clone() for t in (ql.theta, ql.msg, ql.step_out, ql.td)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
