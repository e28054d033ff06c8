"""GPU tests of the batched cartpole Q-learning loop (mpc4rl_amd/qlearning_cartpole.py, csrc/qlearning_kernel.hpp): the roll-out kernel
against the launches it stands for, the TD kernel against float64 torch and the script's per-environment loop, two episodes against the
CPU oracle port, graph replay against eager, and the rank plumbing."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def test_collect_matches_separate_launches():
    """mpcrl_qlearning_cartpole_collect == mpcrl_policy_action + the clip in torch + BatchedCartPoleSwingUpEnv.step + the table writes in
    torch, bit for bit, over 60 steps with failed solves, environments that terminate mid-run and a truncation."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, _lib
    lib = _lib.load()
    E, T, sigma, lo, hi = 256, 60, 0.1, -30.0, 30.0
    g = torch.Generator(device=DEV).manual_seed(7)
    f64 = dict(dtype=torch.float64, device=DEV)
    x0 = (torch.rand(E, 4, generator=g, **f64) * 2 - 1) * torch.tensor([0.5, 1.0, 0.3, 1.0], **f64)
    x0[:, 2] += math.pi * (torch.arange(E, device=DEV) % 2)
    box, drift = torch.arange(0, E, 16, device=DEV), torch.arange(5, E, 16, device=DEV)
    x0[box] = torch.tensor([0.01, 0.0, 0.005, 0.0], **f64)            # inside the goal box: terminated at the first step
    x0[drift] = torch.tensor([0.12, -0.05, 0.0, 0.0], **f64)          # drifts into it with no force: terminated mid-run
    U0 = (torch.rand(T, E, generator=g, **f64) * 2 - 1) * 35.0        # beyond the bounds too: the clip after the noise
    ST = torch.where(torch.rand(T, E, generator=g, **f64) < 0.1, torch.randint(1, 5, (T, E), generator=g, device=DEV), 0).to(torch.int32)
    U0[(ST == 1)] = float("nan")
    eps = torch.randn(T, E, generator=g, dtype=torch.float32, device=DEV)
    for idx in (box, drift):
        U0[:, idx], ST[:, idx], eps[:, idx] = 0.0, 0, 0.0
    envs = [BatchedCartPoleSwingUpEnv(E, device=DEV, seed=0, max_episode_steps=45) for _ in range(2)]
    for env in envs:
        env.state.copy_(x0), env.steps.zero_()
    # the fused kernel
    env = envs[0]
    obs, alive = torch.zeros(E, 4, **f64), torch.ones(E, dtype=torch.uint8, device=DEV)
    row, cold = torch.zeros(E, dtype=torch.int32, device=DEV), torch.ones(E, dtype=torch.int32, device=DEV)
    S, A, Cc = torch.full((T, E, 4), -1.0, **f64), torch.full((T, E), -1.0, **f64), torch.full((T, E), -1.0, **f64)
    live = torch.full((T, E), 7, dtype=torch.uint8, device=DEV)
    for t in range(T):
        u0 = U0[t].contiguous()
        rc = lib.mpcrl_qlearning_cartpole_collect(env._par(), E, T, _p(env.state), _p(env.steps), _p(u0), _p(ST[t]), _p(eps), lo, hi, sigma,
                                                  _p(obs), _p(alive), _p(row), _p(cold), _p(S), _p(A), _p(Cc), _p(live), _stream())
        assert rc == 0
    # the same with the separate launches
    ref = envs[1]
    al = torch.ones(E, dtype=torch.bool, device=DEV)
    lo_t, hi_t = torch.tensor([lo], **f64), torch.tensor([hi], **f64)
    Sr, Ar, Cr, Lr = torch.empty_like(S), torch.empty_like(A), torch.empty_like(Cc), torch.empty_like(live)
    for t in range(T):
        u0 = U0[t].contiguous()
        a = torch.empty(E, 1, dtype=torch.float32, device=DEV)
        assert lib.mpcrl_policy_action(_p(u0), _p(ST[t]), None, _p(lo_t), _p(hi_t), E, 1, 1, 0.0, 0.0, 1, _p(a), None, _stream()) == 0
        a = torch.clamp(a[:, 0] + sigma * eps[t], -1.0, 1.0)
        old, old_steps = ref.state.clone(), ref.steps.clone()
        _, rew, term, trunc = ref.step(a)
        ref.state.copy_(torch.where(al[:, None], ref.state, old)), ref.steps.copy_(torch.where(al, ref.steps, old_steps))
        Sr[t] = old
        Ar[t] = torch.where(al, 0.5 * (hi - lo) * (a.to(torch.float64) + 1.0) + lo, torch.zeros_like(rew))
        Cr[t] = torch.where(al, rew, torch.zeros_like(rew))
        Lr[t] = al.to(torch.uint8)
        al = al & ~(term | trunc)
    torch.cuda.synchronize()
    assert torch.equal(env.state, ref.state) and torch.equal(env.steps, ref.steps) and torch.equal(obs, ref.state)
    assert torch.equal(S, Sr) and torch.equal(A, Ar) and torch.equal(Cc, Cr) and torch.equal(live, Lr)
    assert torch.equal(alive, al.to(torch.uint8)) and bool((row == T).all()) and bool((cold == 0).all())
    L = live.to(torch.int64).sum(0)
    assert bool((L[box] == 1).all())                                     # terminated at step 0
    assert bool(((L[drift] > 1) & (L[drift] < 45)).all())               # terminated mid-run
    assert int((L == 45).sum()) > E // 2                                 # truncated at max_episode_steps
    # a full table: the call writes nothing
    snap = (env.state.clone(), S.clone())
    assert lib.mpcrl_qlearning_cartpole_collect(env._par(), E, T, _p(env.state), _p(env.steps), _p(U0[0].contiguous()), _p(ST[0]), _p(eps), lo, hi,
                                                sigma, _p(obs), _p(alive), _p(row), _p(cold), _p(S), _p(A), _p(Cc), _p(live), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(env.state, snap[0]) and torch.equal(S, snap[1])
    assert lib.mpcrl_qlearning_cartpole_collect(env._par(), E, T, _p(env.state), _p(env.steps), _p(u0), _p(ST[0]), _p(eps), hi, lo, sigma,
                                                _p(obs), _p(alive), _p(row), _p(cold), _p(S), _p(A), _p(Cc), _p(live), _stream()) == -1


def _loop(q, v, dq, sq, sv, cost, L, gamma, lr):
    """scripts/cartpole_mpc_qlearning.py:236-263 per environment (n = size - 1 samples, td[:-1]), failed solves left out."""
    g, ws, cnt = np.zeros(dq.shape[-1]), 0.0, 0
    for e in range(len(L)):
        n = int(L[e]) - 1
        if n < 2:
            continue
        td = cost[: n - 1, e] + gamma * v[1:n, e] - q[: n - 1, e]
        for i in range(n - 1):
            if sq[i, e] == 0 and sv[i, e] == 0 and sq[i + 1, e] == 0 and sv[i + 1, e] == 0:
                g, ws, cnt = g + lr * td[i] * dq[i, e], ws + lr * td[i], cnt + 1
    return g, ws, cnt


def test_td_kernel_matches_float64_and_script_loop():
    from mpc4rl_amd import _lib, qlearning_td_terms
    lib = _lib.load()
    rng = np.random.default_rng(3)
    T, E, n_p, gamma, lr = 50, 600, 86, 0.99, 1e-4
    L = np.concatenate([np.arange(T + 1), rng.integers(0, T + 1, E - T - 1)])
    live = (np.arange(T)[:, None] < L[None, :]).astype(np.uint8)
    cost = rng.uniform(0, 10, (T, E)) * live
    q, v = rng.normal(50, 10, (T - 1, E)), rng.normal(50, 10, (T - 1, E))
    dq = rng.normal(size=(T - 1, E, n_p))
    sq = np.where(rng.uniform(size=(T - 1, E)) < 0.05, 2, 0).astype(np.int32)
    sv = np.where(rng.uniform(size=(T - 1, E)) < 0.05, 1, 0).astype(np.int32)
    q[sq != 0], v[sv != 0], dq[sq != 0] = np.nan, np.nan, np.nan
    d = [torch.as_tensor(a, device=DEV).contiguous() for a in (q, v, dq, sq, sv, cost, live)]
    ws = torch.zeros(int(lib.mpcrl_qlearning_td_workspace_bytes(T, E, n_p)), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        td = torch.full((T - 2, E), -5.0, dtype=torch.float64, device=DEV)
        valid = torch.full((T - 2, E), 9, dtype=torch.uint8, device=DEV)
        msg = torch.full((n_p + 2,), -5.0, dtype=torch.float64, device=DEV)
        assert lib.mpcrl_qlearning_td_grad(*[_p(t) for t in d], T, E, n_p, gamma, lr, _p(ws), _p(td), _p(valid), _p(msg), _stream()) == 0
        outs.append((msg, td, valid))
    torch.cuda.synchronize()
    (msg, td, valid), (msg2, td2, valid2) = outs
    assert torch.equal(msg, msg2) and torch.equal(td, td2) and torch.equal(valid, valid2)     # same inputs, same bits
    assert int(ws[:4].count_nonzero()) == 0                                                   # the ticket is left zero
    mr, tdr, vr = qlearning_td_terms(*[torch.as_tensor(a) for a in (q, v, dq, sq, sv, cost, live)], gamma, lr)
    assert torch.equal(valid.cpu().bool(), vr) and torch.equal(td.cpu(), tdr)
    np.testing.assert_allclose(msg.cpu().numpy(), mr.numpy(), rtol=1e-12, atol=1e-18)
    g, wsum, cnt = _loop(q, v, dq, sq, sv, cost, L, gamma, lr)
    np.testing.assert_allclose(msg[:n_p].cpu().numpy(), g, rtol=1e-12, atol=1e-15)
    assert math.isclose(float(msg[n_p]), wsum, rel_tol=1e-12) and int(msg[n_p + 1]) == cnt > 0
    # T = 2: no term, an empty message
    m0 = torch.full((n_p + 2,), 3.0, dtype=torch.float64, device=DEV)
    assert lib.mpcrl_qlearning_td_grad(*[None] * 7, 2, E, n_p, gamma, lr, None, None, None, _p(m0), _stream()) == 0
    torch.cuda.synchronize()
    assert float(m0.abs().sum()) == 0.0
    assert lib.mpcrl_qlearning_td_grad(*[_p(t) for t in d], T, E, n_p, gamma, lr, None, _p(td), None, _p(msg), _stream()) == -1


def _x0_episode(E):
    """Initial states: two environments inside the goal box, two close to it, the rest at the swing-up's start."""
    x0 = np.zeros((E, 4))
    x0[:, 2] = np.linspace(0.92, 1.08, E) * np.pi
    x0[0], x0[1] = [0.02, 0.0, 0.01, 0.0], [-0.03, 0.02, -0.01, 0.01]
    x0[2], x0[3] = [0.15, 0.0, 0.05, 0.0], [-0.1, 0.1, -0.04, 0.0]
    return x0


def _check_episode(ql, st, th, oracle_port, P):
    """The episode just run by ``ql`` (at parameters ``th``) against the oracle port."""
    lo, hi, sigma, lr, gamma = ql.lo, ql.hi, ql.noise_scale, ql.lr, ql.gamma
    S, A, Cc, live = [t.cpu().numpy() for t in (ql.S, ql.A, ql.C, ql.live)]
    eps = ql.eps.cpu().numpy()
    T, E = live.shape
    L = live.sum(0)
    assert np.array_equal(st.episode_lengths.cpu().numpy(), L)
    # the roll-out: the port's policy solves at the recorded states, warm-started along the episode like the roll-out handle, through the
    # same noise, clip and unscale
    prev, n_cmp = None, 0
    for t in range(T):
        r = oracle_port.solve(P, S[t], p=th, flags=0, warm=prev)
        prev = r
        ok = (live[t] == 1) & (r.status == 0)
        a_port = (2.0 * ((r.u0[:, 0] - lo) / (hi - lo)) - 1.0).astype(np.float32)
        a_port = np.clip(a_port + np.float32(sigma) * eps[t], np.float32(-1.0), np.float32(1.0))
        a_rec = (A[t] - lo) / (0.5 * (hi - lo)) - 1.0
        assert np.all(np.abs(a_rec - a_port)[ok] <= 1e-6), (t, np.max(np.abs(a_rec - a_port)[ok]))
        n_cmp += int(ok.sum())
    assert n_cmp >= 0.9 * L.sum()
    # the sweep: Q, dQ/dp (u0 pinned, cold) and V (from the Q solve's iterate) of every sample row at the episode's parameters
    n = T - 1
    s, a = S[:n].reshape(n * E, 4), A[:n].reshape(n * E, 1)
    oq = oracle_port.solve(P, s, p=th, u0fix=a)
    ov = oracle_port.solve(P, s, p=th, warm=oq, flags=0)         # V from the Q solve's iterate, as the sweep's V solve starts
    rq, rv = ql.last_sweep
    valid = ql.valid.cpu().numpy().astype(bool)
    rows = np.zeros((n, E), bool)
    rows[:-1] |= valid
    rows[1:] |= valid
    rows = rows.reshape(-1)
    rel = lambda got, want: (np.abs(got - want) / np.maximum(np.abs(want), 1.0)).reshape(got.shape[0], -1).max(1)   # noqa: E731
    v_gpu = rv.V.cpu().numpy()
    v_cold = oracle_port.solve(P, s, p=th, flags=0).V              # (diagnostics only: V from the cold start)
    assert rows.sum() > 0 and np.all(oq.status[rows] == 0) and np.all(ov.status[rows] == 0), \
        (np.nonzero(rows & (ov.status != 0))[0], rel(v_gpu, v_cold)[rows & (ov.status != 0)])
    for name, got, want in (("Q", rq.V.cpu().numpy(), oq.V), ("V", v_gpu, ov.V), ("dQ_dp", rq.dV_dp.cpu().numpy(), oq.dV)):
        err = rel(got, want)[rows]
        assert err.max() < 1e-6, (name, err.max(), np.nonzero(rows)[0][err >= 1e-6], rel(v_gpu, v_cold)[rows][err >= 1e-6])
    # the step: the script's formula on the port's numbers, over the valid terms
    qp, vp, dqp = oq.V.reshape(n, E), ov.V.reshape(n, E), oq.dV.reshape(n, E, -1)
    td = Cc[: n - 1] + gamma * vp[1:] - qp[:-1]
    dp = (lr * td)[..., None] * dqp[: n - 1]
    step_ref = dp[valid].mean(0)
    # (td is a difference of costs of O(|Q|): its error scale is that of the terms it is made of, not of itself)
    scale = (lr * (np.abs(Cc[: n - 1]) + gamma * np.abs(vp[1:]) + np.abs(qp[:-1])))[..., None] * np.abs(dqp[: n - 1])
    got = st.step.cpu().numpy()
    np.testing.assert_allclose(got[:3], step_ref[:3], rtol=1e-6, atol=1e-6 * float(scale[valid][:, :3].mean(0).max()))
    assert np.all(got[3:] == 0.0) and np.abs(got[:3]).max() > 0.0
    assert abs(st.td_error_mean - td[valid].mean()) <= 1e-6 * max(1.0, float(np.abs(qp[:-1][valid]).mean()))


def test_two_episodes_against_oracle_port(oracle_port):
    """Two episodes of E = 8, T = 40 with environments that end early (goal box, truncation at 30 steps), checked against the CPU oracle
    port: the recorded actions, Q / V / dQ/dp of the rows that enter the step, the step itself and the parameters after it."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, CartpoleQLearning, cartpole_ocp
    from oracle.problems import make_cartpole
    P = make_cartpole()
    E, T = 8, 40
    for noise in (0.1, 0.0):
        env = BatchedCartPoleSwingUpEnv(E, device=DEV, seed=1, max_episode_steps=30)
        ql = CartpoleQLearning(cartpole_ocp(), env, T, lr=1e-4, gamma=0.99, noise_scale=noise, seed=2)
        x0 = torch.as_tensor(_x0_episode(E), device=DEV)
        for ep in range(2 if noise > 0 else 1):
            th = ql.theta.clone()
            st = ql.run_episode(x0)
            torch.cuda.synchronize()
            L = st.episode_lengths.cpu().numpy()
            assert L.min() < 30 and L.max() == 30 and st.converged_fraction > 0.9
            _check_episode(ql, st, th.cpu().numpy(), oracle_port, P)
            assert torch.equal(ql.theta, th + st.step)
            assert torch.equal(ql.rollout_mpc.get_theta(), ql.theta) and torch.equal(ql.sample_mpc.get_theta(), ql.theta)


def test_graphs_equal_eager():
    """Two episodes replayed from the captured graphs give the bits of two eager episodes: theta, table, statistics."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, CartpoleQLearning, cartpole_ocp
    E, T = 96, 24
    runs = []
    for graphs in (False, True):
        env = BatchedCartPoleSwingUpEnv(E, device=DEV, seed=5, max_episode_steps=20)
        ql = CartpoleQLearning(cartpole_ocp(), env, T, lr=1e-3, seed=6)
        if graphs:
            ql.enable_graphs()
        out = []
        for ep in range(2):
            x0 = torch.as_tensor(_x0_episode(E), device=DEV) if ep == 1 else None
            st = ql.run_episode(x0)
            out.append((st, ql.theta.clone(), [t.clone() for t in (ql.S, ql.A, ql.C, ql.live, ql.td, ql.valid, ql.msg)]))
        runs.append(out)
    torch.cuda.synchronize()
    for (se, te, tabs_e), (sg, tg, tabs_g) in zip(*runs):
        assert torch.equal(te, tg)
        for a, b in zip(tabs_e, tabs_g):
            assert torch.equal(a, b)
        assert torch.equal(se.step, sg.step) and torch.equal(se.episode_lengths, sg.episode_lengths)
        assert (se.total_cost, se.td_error_mean, se.converged_fraction) == (sg.total_cost, sg.td_error_mean, sg.converged_fraction)
    assert float(runs[0][0][0].step.abs().max()) > 0.0


def test_nccl_world1_group_gives_the_same_step():
    """The rank plumbing: with the `nccl` (= RCCL) process group of world size 1 the episode's message goes through the collective and
    the step is that of group=None."""
    import socket
    import torch.distributed as dist
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, CartpoleQLearning, cartpole_ocp
    E, T = 64, 16
    steps = []
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        for group in (None, dist.group.WORLD):
            env = BatchedCartPoleSwingUpEnv(E, device=DEV, seed=9)
            ql = CartpoleQLearning(cartpole_ocp(), env, T, lr=1e-3, seed=4, group=group)
            st = ql.run_episode()
            steps.append((st.step, ql.theta.clone()))
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert torch.equal(steps[0][0], steps[1][0]) and torch.equal(steps[0][1], steps[1][1])
    assert float(steps[0][0].abs().max()) > 0.0
