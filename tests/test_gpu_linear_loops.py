"""GPU tests of the linear system's device loops (csrc/linear_loop_kernel.hpp, mpc4rl_amd/qlearning_linear.py, mpc4rl_amd/ppo.py): the
two roll-out kernels and mpcrl_env_linear_step against their torch statements bit for bit, the argument checks, LinearQLearning end to
end, against BatchedQLearning and replayed from graphs, and BatchedPPO on the linear system.

Bit-for-bit comparisons use an environment whose A, B, noise bounds, states, actions and draws are dyadic numbers of a few bits, so that
every product and sum of the step is exact: the kernels are compiled with floating-point contraction, the torch statement rounds once per
operation, and the two are the same bits exactly where that cannot matter (tests/test_linear_loops_cpu.py).  With the reference's A, B and
arbitrary inputs they agree to a few roundings: ROUND = 1e-14 relative (at most 8 roundings of 2^-53 on sums of positive-magnitude terms
no larger than 3 times the result or 1) is the bound used there."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
DYADIC = dict(A=[[0.875, 0.375], [0.0, 1.125]], B=[[0.0625], [0.25]], lb_noise=-0.125, ub_noise=0.0)
ROUND = 1e-14


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _rel(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / np.where(want != 0.0, np.abs(want), 1.0))) if got.size else 0.0


def _close(got, want):
    """to a few roundings, relative to max(|want|, 1)"""
    if want.numel() == 0:
        return got.numel() == 0
    return float(((got.cpu() - want.cpu()).abs() / want.cpu().abs().clamp(min=1.0)).max()) <= ROUND


def _grid(g, shape, lo, hi, den, dtype=torch.float64):
    """integers in [lo, hi] over den: numbers of a few bits"""
    return (torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64) / den).to(dtype).to(DEV)


def _inputs(E, seed, dyadic=True):
    """States on both sides of the box, solves of every status with NaN and inf controls, draws that clip at both ends."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(E, device=DEV)
    if dyadic:
        state, u0 = _grid(g, (E, 2), -32, 32, 16), _grid(g, (E,), -24, 24, 16)
    else:
        state, u0 = (torch.rand(E, 2, generator=g, dtype=torch.float64) * 4 - 2).to(DEV), (torch.rand(E, generator=g, dtype=torch.float64) * 3 - 1.5).to(DEV)
    side = torch.tensor([[-1.0, 1.5], [-0.5, -0.5], [1.5, 0.5], [0.5, 0.5]], **F64)       # new state: both sides, below, above, inside
    state[: min(E, 4)] = side[: min(E, 4)]
    status = torch.where(i % 5 == 2, 4, torch.where(i % 5 == 1, 2, torch.where(i % 5 == 4, 1, 0))).to(torch.int32)
    if E > 1:
        u0[i % 7 == 3], u0[i % 11 == 5] = float("nan"), float("inf")
    return g, i, state, u0, status


def _env(E, dyadic=True):
    from mpc4rl_amd import BatchedLinearSystemEnv, linear_env_par
    env = BatchedLinearSystemEnv(E, device=DEV, seed=0, **(DYADIC if dyadic else {}))
    par = linear_env_par(env)
    return env, par, (C.c_double * 12)(*par)


# ---------------------------------------------------------------------- 1. the roll-out kernels against their torch statements
def _ql_case(E, sigma, rows, dyadic):
    """One call of mpcrl_qlearning_linear_collect and what the torch statement says every buffer holds afterwards."""
    from mpc4rl_amd import _lib, linear_collect_terms
    lib = _lib.load()
    T, lo, hi = 5, -1.0, 1.0
    env, par, par_c = _env(E, dyadic)
    g, i, state, u0, status = _inputs(E, 100 + E, dyadic)
    if dyadic:
        eps, u01 = _grid(g, (T, E), -32, 32, 8, torch.float32), _grid(g, (T, E), 0, 15, 16)
    else:
        eps, u01 = torch.randn(T, E, generator=g).to(DEV) * 2, torch.rand(T, E, generator=g, dtype=torch.float64).to(DEV)
    row = torch.tensor(rows, dtype=torch.int32, device=DEV)[i % len(rows)].contiguous()
    env.state.copy_(state)
    obs, cold = torch.full((E, 2), -7.0, **F64), torch.ones(E, dtype=torch.int32, device=DEV)
    S, A, Cc = torch.full((T, E, 2), -7.0, **F64), torch.full((T, E), -7.0, **F64), torch.full((T, E), -7.0, **F64)
    before = [t.clone() for t in (state, obs, cold, row, S, A, Cc)]
    assert lib.mpcrl_qlearning_linear_collect(par_c, E, T, _p(env.state), _p(u0), _p(status), _p(eps), _p(u01), lo, hi, sigma, _p(obs), _p(row),
                                              _p(cold), _p(S), _p(A), _p(Cc), _stream()) == 0
    torch.cuda.synchronize()
    # the statement, on the CPU: the lanes whose row lies inside the table step and write that row; the others touch nothing
    st0, ob0, co0, ro0, S0, A0, C0 = [t.cpu() for t in before]
    on = (ro0 >= 0) & (ro0 < T)
    r = ro0.clamp(0, T - 1).long()
    e = torch.arange(E)
    act, new, cost = linear_collect_terms(par, st0, u0.cpu(), status.cpu(), eps.cpu()[r, e], u01.cpu()[r, e], lo, hi, sigma)
    S0[r[on], e[on]], A0[r[on], e[on]], C0[r[on], e[on]] = st0[on], act[on], cost[on]
    want = (torch.where(on[:, None], new, st0), torch.where(on[:, None], new, ob0), torch.where(on, 0, co0).to(torch.int32),
            torch.where(on, ro0 + 1, ro0).to(torch.int32), S0, A0, C0)
    good = ((status == 0) | (status == 2)) & torch.isfinite(u0)
    return (env.state, obs, cold, row, S, A, Cc), want, dict(on=on, act=act, new=new, cost=cost, good=good.cpu(), u0=u0.cpu())


@pytest.mark.parametrize("sigma", [0.0, 0.5])
@pytest.mark.parametrize("E,rows", [(300, (0, 4, 5)), (1, (0,)), (1, (4,)), (1, (5,))])
def test_qlearning_collect_equals_its_statement_bitwise(E, rows, sigma):
    """Rows 0, T - 1 and T (a full table: that lane writes nothing anywhere — the whole buffers are compared), two workgroups with a ragged
    tail and a single lane, statuses 0, 1, 2, 4, NaN and inf controls, sigma = 0 (the action is u0 itself) and sigma > 0 with samples that
    clip at both ends, new states on each side of the box."""
    got, want, x = _ql_case(E, sigma, rows, dyadic=True)
    for name, a, b in zip(("state", "obs", "cold", "row", "S", "A", "C"), got, want):
        assert torch.equal(a.cpu(), b), name
    if E > 1:
        on, act, new = x["on"], x["act"], x["new"]
        assert 0 < int(on.sum()) < E and 0 < int(x["good"].sum()) < E
        pen = torch.round((x["cost"] - 0.5 * (new * new).sum(1) - 0.5 * act * act) / 100.0)
        assert sorted(set(pen.tolist())) == [0.0, 1.0, 2.0]                     # no side, one side, both sides of the box
        assert bool(torch.isfinite(act).all()) and float(act[~x["good"]].abs().max()) == (0.0 if sigma == 0.0 else 1.0)
        if sigma == 0.0:
            assert torch.equal(act[x["good"]], x["u0"][x["good"]]) and float(act.abs().max()) > 1.0      # u0 itself, not clipped
        else:
            assert float(act.min()) == -1.0 and float(act.max()) == 1.0 and int(((act > -1.0) & (act < 1.0)).sum()) > 0


def _ppo_tables(T, E):
    return ([torch.full((T, E, 2) if k in (0, 5) else (T, E), -7.0, **F64) for k in range(6)]
            + [torch.full((T, E), 9, dtype=torch.uint8, device=DEV) for _ in range(3)])       # OBS ACT LOGP VAL REW NEXT | TERM DONE OK


def _ppo_call(lib, par_c, E, T, t, env, steps, u0, status, eps, u01, value, log_std, lo, hi, rs, L, reset, tabs, obs, ended):
    return lib.mpcrl_ppo_linear_collect(par_c, E, T, t, _p(env.state), _p(steps), _p(u0), _p(status), _p(eps), _p(u01), _p(value), _p(log_std), lo, hi,
                                        rs, L, reset, *[_p(x) for x in tabs], _p(obs), _p(ended), _stream())


@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("E", [300, 1])
def test_ppo_collect_equals_its_statements_bitwise(E, t):
    """Row t = 0 and t = T - 1 of the tables, the environments, the counters, obs and ended after mpcrl_ppo_linear_collect against
    ppo_collect_terms + ppo_linear_collect_terms, torch.equal (log_std = 0: sigma = 1 and the log probability's arithmetic is exact up to
    its last subtraction); counters one short of episode_length for a third of the lanes, so some restart and some go on."""
    from mpc4rl_amd import _lib, ppo_collect_terms, ppo_linear_collect_terms
    lib = _lib.load()
    T, L, lo, hi, rs = 3, 3, -1.0, 1.0, -0.5
    env, par, par_c = _env(E)
    g, i, state, u0, status = _inputs(E, 200 + E)
    eps, u01, value = _grid(g, (E,), -32, 32, 8, torch.float32), _grid(g, (E,), 0, 15, 16), _grid(g, (E,), -64, 64, 8)
    steps = ((i + 2) % 3).to(torch.int64).contiguous()
    env.state.copy_(state)
    log_std = torch.zeros(1, **F64)
    reset = (C.c_double * 2)(0.5, 0.5)
    tabs = _ppo_tables(T, E)
    obs, ended = torch.full((E, 2), -7.0, **F64), torch.full((E,), 9, dtype=torch.int32, device=DEV)
    steps0 = steps.clone()
    assert _ppo_call(lib, par_c, E, T, t, env, steps, u0, status, eps, u01, value, log_std, lo, hi, rs, L, reset, tabs, obs, ended) == 0
    torch.cuda.synchronize()
    mu, act, logp, ok = ppo_collect_terms(u0.cpu(), status.cpu(), eps.cpu(), 0.0, lo, hi)
    nxt, rew, done, new, cnt = ppo_linear_collect_terms(par, state.cpu(), steps0.cpu(), act, u01.cpu(), rs, L)
    OBS, ACT, LOGP, VAL, REW, NEXT, TERM, DONE, OK = [x.cpu() for x in tabs]
    for name, a, b in (("OBS", OBS[t], state.cpu()), ("ACT", ACT[t], act), ("LOGP", LOGP[t], logp), ("VAL", VAL[t], value.cpu()), ("REW", REW[t], rew),
                       ("NEXT", NEXT[t], nxt), ("DONE", DONE[t].bool(), done), ("OK", OK[t].bool(), ok), ("state", env.state.cpu(), new),
                       ("obs", obs.cpu(), new), ("steps", steps.cpu(), cnt), ("ended", ended.cpu().bool(), done)):
        assert torch.equal(a, b), name
    assert int(TERM[t].sum()) == 0 and torch.equal(done, steps0.cpu() == 2) and bool((new[done] == 0.5).all())
    for x in (OBS, ACT, LOGP, VAL, REW, NEXT, TERM, DONE, OK):                     # the other rows are untouched
        for row in set(range(T)) - {t}:
            assert bool((x[row] == (9 if x.dtype == torch.uint8 else -7.0)).all())
    if E > 1:
        assert 0 < int(done.sum()) < E and 0 < int(ok.sum()) < E
        assert float(act.min()) < -1.0 and float(act.max()) > 1.0 and float(nxt.abs().max()) < 10.0      # the environment saw the clip
        assert int((rew <= -50.0).sum()) > 0 and int((rew <= -100.0).sum()) > 0 and int((rew > -50.0).sum()) > 0


def test_reference_parameters_agree_to_rounding():
    """The reference's A, B and noise bounds with arbitrary states, controls and draws: the three kernels against the torch statements to
    a few roundings (nothing here is exact, so contraction shows)."""
    from mpc4rl_amd import _lib, linear_env_step_terms
    lib = _lib.load()
    got, want, _ = _ql_case(300, 0.3, (0, 4, 5), dyadic=False)
    for name, a, b in zip(("state", "obs", "cold", "row", "S", "A", "C"), got, want):
        assert (torch.equal(a.cpu(), b) if name in ("cold", "row", "A") else _close(a, b)), name
    E = 300
    env, par, par_c = _env(E, dyadic=False)
    g, i, state, u0, status = _inputs(E, 7, dyadic=False)
    act, u01 = u0.nan_to_num(0.0, 1.0, -1.0).contiguous(), torch.rand(E, generator=g, dtype=torch.float64).to(DEV)
    env.state.copy_(state)
    obs, cost = torch.empty(E, 2, **F64), torch.empty(E, **F64)
    assert lib.mpcrl_env_linear_step(par_c, E, _p(env.state), _p(act), _p(u01), _p(obs), 0, _p(cost), _stream()) == 0
    torch.cuda.synchronize()
    new, c = linear_env_step_terms(par, state.cpu(), act.cpu(), u01.cpu())
    assert _close(obs, new) and _close(env.state, new) and _close(cost, c)


# ---------------------------------------------------------------------- 2. the refactored environment kernel
@pytest.mark.parametrize("E", [300, 1])
def test_env_linear_step_equals_the_shared_step_function_bitwise(E):
    """mpcrl_env_linear_step (through BatchedLinearSystemEnv.step's export) on the inputs of the roll-out kernels' tests equals
    linear_env_step's statement bit for bit, and so the rows the roll-out kernels write for the same inputs."""
    from mpc4rl_amd import _lib, linear_env_step_terms
    lib = _lib.load()
    env, par, par_c = _env(E)
    g, i, state, u0, status = _inputs(E, 300 + E)
    act, u01 = u0.nan_to_num(0.0, 1.0, -1.0).contiguous(), _grid(g, (E,), 0, 15, 16)
    env.state.copy_(state)
    obs, cost = torch.full((E, 2), -7.0, **F64), torch.full((E,), -7.0, **F64)
    assert lib.mpcrl_env_linear_step(par_c, E, _p(env.state), _p(act), _p(u01), _p(obs), 0, _p(cost), _stream()) == 0
    obs32 = torch.full((E, 2), -7.0, dtype=torch.float32, device=DEV)
    st2, cost2 = state.clone(), torch.full((E,), -7.0, **F64)
    assert lib.mpcrl_env_linear_step(par_c, E, _p(st2), _p(act), _p(u01), _p(obs32), 1, _p(cost2), _stream()) == 0
    torch.cuda.synchronize()
    new, c = linear_env_step_terms(par, state.cpu(), act.cpu(), u01.cpu())
    assert torch.equal(env.state.cpu(), new) and torch.equal(obs.cpu(), new) and torch.equal(cost.cpu(), c)
    assert torch.equal(st2.cpu(), new) and torch.equal(obs32.cpu(), new.float()) and torch.equal(cost2.cpu(), c)
    if E > 1:
        assert int((c >= 200.0).sum()) > 0 and int((c < 100.0).sum()) > 0


# ---------------------------------------------------------------------- 3. argument errors
def test_argument_errors():
    from mpc4rl_amd import _lib
    lib = _lib.load()
    E, T = 4, 3
    env, par, par_c = _env(E)
    z = torch.zeros(T, E, 2, **F64)
    zi, zl, zf = torch.zeros(E, dtype=torch.int32, device=DEV), torch.zeros(E, dtype=torch.int64, device=DEV), torch.zeros(T, E, dtype=torch.float32, device=DEV)
    u8 = torch.zeros(T, E, dtype=torch.uint8, device=DEV)

    def ql(E=E, T=T, S=z, par_c=par_c):
        return lib.mpcrl_qlearning_linear_collect(par_c, E, T, _p(env.state), _p(z), _p(zi), _p(zf), _p(z), -1.0, 1.0, 0.0, _p(z), _p(zi), _p(zi), _p(S),
                                                  _p(z), _p(z), _stream())

    def ppo(E=E, T=T, t=0, L=3, NEXT=z, reset=(C.c_double * 2)(0.5, 0.5)):
        return lib.mpcrl_ppo_linear_collect(par_c, E, T, t, _p(env.state), _p(zl), _p(z), _p(zi), _p(zf), _p(z), _p(z), _p(z), -1.0, 1.0, -1.0, L, reset,
                                            _p(z), _p(z), _p(z), _p(z), _p(z), _p(NEXT), _p(u8), _p(u8), _p(u8), _p(z), _p(zi), _stream())

    assert ql(S=None) == -1 and ql(T=0) == -1 and ql(E=-1) == -1 and ql(par_c=None) == -1
    assert ppo(NEXT=None) == -1 and ppo(t=T) == -1 and ppo(t=-1) == -1 and ppo(L=0) == -1 and ppo(T=0) == -1 and ppo(E=-1) == -1 and ppo(reset=None) == -1
    assert ql(E=0) == 0 and ppo(E=0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- 4. LinearQLearning end to end
def _check_episode(ql, st, theta0, x0):
    from mpc4rl_amd import linear_collect_terms, qlearning_td_terms
    T, E, n = ql.T, ql.E, ql.T - 1
    S, A, Cc = ql.S.cpu(), ql.A.cpu(), ql.C.cpu()
    assert torch.equal(S[0], x0.cpu()) and len(ql.last) == T
    for t in range(T):
        r = ql.last[t]
        assert bool(((r.status == 0) | (r.status == 2)).all())
        act, new, cost = linear_collect_terms(ql.par, S[t], r.u0.cpu(), r.status.cpu(), ql.eps[t].cpu(), ql.u01[t].cpu(), ql.lo, ql.hi, ql.noise_scale)
        assert torch.equal(A[t], act), t                          # no product in it that contraction could fuse
        assert _close(Cc[t], cost) and _close(S[t + 1] if t + 1 < T else ql.env.state, new), t
    assert torch.equal(ql.obs, ql.env.state) and bool((ql.row == T).all()) and bool((ql.cold == 0).all())
    rq, rv = ql.last_sweep
    msg, td, valid = qlearning_td_terms(rq.V.reshape(n, E).cpu(), rv.V.reshape(n, E).cpu(), rq.dV_dp.reshape(n, E, -1).cpu(), rq.status.reshape(n, E).cpu(),
                                        rv.status.reshape(n, E).cpu(), Cc, ql.live.cpu(), ql.gamma, ql.lr)
    assert torch.equal(ql.valid.cpu().bool(), valid) and torch.equal(ql.td.cpu(), td)
    np.testing.assert_allclose(ql.msg.cpu().numpy(), msg.numpy(), rtol=1e-12, atol=1e-18)
    count = float(ql.msg[-1])
    assert count == (T - 2) * E == float(valid.sum()) and st.converged_fraction == 1.0
    assert torch.equal(st.step, ql.step_out) and np.array_equal(ql.step_out.cpu().numpy(), ql.msg[: ql.n_p].cpu().numpy() / max(1.0, count))
    assert torch.equal(ql.theta, theta0 + ql.step_out) and int((ql.step_out != 0.0).sum()) > 3
    assert torch.equal(ql.rollout_mpc.get_theta(), ql.theta) and torch.equal(ql.sample_mpc.get_theta(), ql.theta)
    assert math.isclose(st.total_cost, float(Cc.sum()) / E, rel_tol=1e-12) and math.isclose(st.td_error_mean, float(td.sum()) / count, rel_tol=1e-12)


@pytest.mark.parametrize("noise_scale", [0.0, 0.25])
def test_linear_qlearning_two_episodes(noise_scale):
    """E = 5, T = 4, the default OCP, two episodes (the second from given initial states): the table rows against linear_collect_terms on
    the learner's own solves and draws, the TD step against qlearning_td_terms on its sweep, theta moved by step_out."""
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp
    E, T = 5, 4
    ocp = linear_system_ocp()
    ql = LinearQLearning(ocp, BatchedLinearSystemEnv(E, device=DEV, seed=1), T, lr=1e-3, noise_scale=noise_scale, seed=2)
    assert ql.gamma == ocp.gamma and ql.rollout_mpc.gamma == ocp.gamma and ql.sample_mpc.gamma == ocp.gamma and float(ql.learn_mask.sum()) == 12.0
    x1 = torch.tensor([[0.5, 0.5], [0.2, -0.3], [0.8, 0.1], [0.1, 0.6], [0.6, -0.5]], **F64)
    for x0 in (None, x1):
        theta0 = ql.theta.clone()
        st = ql.run_episode(x0)
        torch.cuda.synchronize()
        _check_episode(ql, st, theta0, torch.full((E, 2), 0.5, **F64) if x0 is None else x0)
    assert ql.episodes == 2


def test_linear_qlearning_T2_is_an_empty_step():
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp
    ql = LinearQLearning(linear_system_ocp(), BatchedLinearSystemEnv(5, device=DEV, seed=1), 2, lr=1e-3)
    theta0 = ql.theta.clone()
    st = ql.run_episode()
    torch.cuda.synchronize()
    assert float(ql.msg.abs().sum()) == 0.0 and torch.equal(ql.theta, theta0) and float(st.step.abs().sum()) == 0.0
    assert st.converged_fraction == 1.0 and st.total_cost > 0.0


# ---------------------------------------------------------------------- 5. against the class it succeeds
def test_linear_qlearning_agrees_with_batched_qlearning():
    """One episode of each from the same reset, without noise or exploration.  The two differ in how their solves start (per-instance cold
    mask against reset(); the V solve from the Q solve's iterate against cold), so they agree to the solver's tolerance, not bit for bit.
    Measured on the MI355X: the largest difference of the parameter step is 2.7e-12, 1.8e-9 of the step's norm (1.5e-3); the C table, and
    S and A with it, are the same bits (the roll-out solves start from the same cold iterates).  The bounds are ten times that: 1.8e-8 of
    the norm, far inside the 1e-4 ceiling, and equality of the tables.  A wrong sign or a row off by one is of order 1."""
    from mpc4rl_amd import BatchedLinearSystemEnv, BatchedQLearning, LinearQLearning, linear_system_ocp
    E, T, lr = 5, 6, 1e-3
    ocp = linear_system_ocp()
    new = LinearQLearning(ocp, BatchedLinearSystemEnv(E, device=DEV, seed=1, lb_noise=0.0, ub_noise=0.0), T, lr=lr, noise_scale=0.0)
    old = BatchedQLearning(ocp, BatchedLinearSystemEnv(E, device=DEV, seed=1, lb_noise=0.0, ub_noise=0.0), T, lr=lr, device=DEV)
    s_new, s_old = new.run_episode(), old.run_episode()
    torch.cuda.synchronize()
    S, A, Cc = old.last_episode
    norm = float(s_old.step.norm())
    d_step, d_C = float((s_new.step - s_old.step).abs().max()), float((new.C - Cc).abs().max())
    d_S, d_A = float((new.S - S).abs().max()), float((new.A - A.reshape(T, E)).abs().max())
    print(f"step norm {norm:.6e}; max |step difference| {d_step:.3e} ({d_step / norm:.3e} of the norm); max |C difference| {d_C:.3e}; "
          f"S {d_S:.3e}, A {d_A:.3e}; theta {float((new.theta - old.theta).abs().max()):.3e}")
    assert s_new.converged_fraction == 1.0 and s_old.converged_fraction == 1.0
    assert norm > 0.0 and float(Cc.abs().max()) > 0.0
    assert d_step <= 10.0 * 1.8e-9 * norm
    assert d_C == 0.0 and d_S == 0.0 and d_A == 0.0


# ---------------------------------------------------------------------- 6. graphs
def test_linear_qlearning_graphs_equal_eager():
    """Two episodes replayed from the captured graphs (the second from given initial states) give the bits of two eager episodes of a
    learner with the same seeds: theta, S, A, C, the TD terms and the message."""
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp
    E, T = 96, 6
    x1 = torch.rand(E, 2, generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(DEV) * torch.tensor([1.0, 1.2], **F64) - torch.tensor([0.0, 0.6], **F64)
    runs = []
    for graphs in (False, True):
        ql = LinearQLearning(linear_system_ocp(), BatchedLinearSystemEnv(E, device=DEV, seed=5), T, lr=1e-3, noise_scale=0.1, seed=6)
        if graphs:
            ql.enable_graphs()
        out = []
        for x0 in (None, x1):
            st = ql.run_episode(x0)
            out.append((st, ql.theta.clone(), [t.clone() for t in (ql.S, ql.A, ql.C, ql.td, ql.valid, ql.msg)]))
        runs.append(out)
    torch.cuda.synchronize()
    for (se, te, tabs_e), (sg, tg, tabs_g) in zip(*runs):
        assert torch.equal(te, tg) and torch.equal(se.step, sg.step)
        for a, b in zip(tabs_e, tabs_g):
            assert torch.equal(a, b)
        assert (se.total_cost, se.td_error_mean, se.converged_fraction) == (sg.total_cost, sg.td_error_mean, sg.converged_fraction)
    assert float(runs[0][0][0].step.abs().max()) > 0.0 and not torch.equal(runs[0][0][1], runs[0][1][1])


# ---------------------------------------------------------------------- 7. PPO on the linear system
@pytest.mark.parametrize("value_kernels", [False, True])
def test_ppo_on_the_linear_system(value_kernels):
    """E = 96, n_steps = 4, episode_length = 3: truncations fall inside a roll-out and across its boundary.  Two roll-outs against
    ppo_collect_terms + ppo_linear_collect_terms + ppo_gae on the recorded solves, one minibatch against ppo_surrogate_terms, learn(2)."""
    from mpc4rl_amd import (BatchedLinearSystemEnv, BatchedPPO, linear_system_ocp, ppo_collect_terms, ppo_gae, ppo_linear_collect_terms,
                            ppo_surrogate_terms)
    from mpc4rl_amd.qlearning_linear import linear_env_par
    E, T, B, L = 96, 4, 128, 3
    env = BatchedLinearSystemEnv(E, device=DEV, seed=3)
    ppo = BatchedPPO(linear_system_ocp(), env, n_steps=T, batch_size=B, n_epochs=1, lr=1e-3, ent_coef=0.01, log_std_init=-1.0, seed=11,
                     value_kernels=value_kernels, episode_length=L)
    par = linear_env_par(env)
    assert float(ppo.learn_mask.sum()) == 12.0 and ppo.OBS.shape == (T, E, 2) and ppo.obs.shape == (E, 2)
    rec, step = [], ppo._collect_step

    def recording(t):
        before = (env.state.clone(), ppo.steps.clone(), ppo.ended.clone())
        step(t)
        rec.append(before + ppo.last_collect)

    ppo._collect_step = recording
    for it in range(2):
        del rec[:]
        ppo.collect()
        torch.cuda.synchronize()
        ls = float(ppo.log_std)
        for t in range(T):
            s0, n0, cold, r, eps, u01, value = [x.cpu() if torch.is_tensor(x) else x for x in rec[t]]
            mu, act, logp, ok = ppo_collect_terms(r.u0.cpu(), r.status.cpu(), eps, ls, ppo.lo, ppo.hi)
            assert _rel(ppo.ACT[t].cpu().numpy(), act.numpy()) <= 1e-12 and _rel(ppo.LOGP[t].cpu().numpy(), logp.numpy()) <= 1e-12
            assert torch.equal(ppo.OK[t].cpu().bool(), ok) and bool(ok.all())
            nxt, rew, done, new, cnt = ppo_linear_collect_terms(par, s0, n0, ppo.ACT[t].cpu(), u01, ppo.reward_scale, L)
            assert torch.equal(ppo.OBS[t].cpu(), s0) and torch.equal(ppo.VAL[t].cpu(), value)
            assert _close(ppo.NEXT[t], nxt) and _close(ppo.REW[t], rew)
            assert torch.equal(ppo.DONE[t].cpu().bool(), done) and bool(done.all()) == ((it * T + t) % L == L - 1) == bool(done.any())
            nxt_state, nxt_cold = (rec[t + 1][0], rec[t + 1][2]) if t + 1 < T else (env.state, ppo.ended)
            assert torch.equal(nxt_cold.cpu().bool(), done)                       # the rows that ended start the next solve cold
            assert bool((nxt_state.cpu()[done] == 0.5).all()) and _close(nxt_state.cpu()[~done], new[~done])
            assert torch.equal((ppo.steps if t + 1 == T else rec[t + 1][1]).cpu(), cnt)
        assert int(ppo.TERM.sum()) == 0
        adv, ret = ppo_gae(ppo.REW.cpu(), ppo.VAL.cpu(), ppo.VNEXT.cpu(), ppo.TERM.cpu(), ppo.DONE.cpu(), ppo.gamma, ppo.gae_lambda)
        assert _rel(ppo.ADV.cpu().numpy(), adv.numpy()) <= 1e-12 and _rel(ppo.RET.cpu().numpy(), ret.numpy()) <= 1e-12
    ppo._collect_step = step
    # one minibatch
    box, solve = {}, ppo.sample_mpc.solve

    def recording_solve(*a, **k):
        box["r"] = solve(*a, **k)
        return box["r"]

    ppo.sample_mpc.solve = recording_solve
    idx = torch.randperm(T * E, generator=torch.Generator().manual_seed(1))[:B].to(DEV).contiguous()
    theta0, ls0 = ppo.theta.clone(), ppo.log_std.clone()
    ppo._minibatch(idx)
    torch.cuda.synchronize()
    ppo.sample_mpc.solve = solve
    r = box["r"]
    ref = ppo_surrogate_terms(idx.cpu(), ppo.ACT.cpu(), ppo.LOGP.cpu(), ppo.ADV.cpu(), ppo.OK.cpu(), r.u0.cpu(), r.status.cpu(), r.dpi_dp.cpu(), float(ls0),
                              ppo.lo, ppo.hi, ppo.clip_range, ppo.ent_coef, ppo.lr, ppo.normalize_advantage)
    got = ppo.msg.cpu()
    # Here the re-solve runs at the roll-out's parameters, so the ratios are 1 (to the solver's tolerance) and two of the statistics are
    # sums that cancel: entry n_p + 2, sum loss = -sum of the NORMALISED advantages, which is zero up to rounding, and entry n_p + 3,
    # sum (r - 1) - log r.  A bound relative to such a sum's own value means nothing; they are held to 1e-12 of the sum of the magnitudes of
    # their terms, which is at most B (normalised advantages have unit variance, so sum |A_b| <= B; |r - 1| + |log r| << 1).  Every other
    # entry is held to the 1e-12 relative of tests/test_gpu_ppo.py.
    loss, kl = ppo.n_p + 2, ppo.n_p + 3
    assert ppo.normalize_advantage
    keep = ~np.isin(np.arange(ppo.n_p + 8), (loss, kl))
    per = np.abs(got.numpy() - ref.numpy()) / np.where(ref.numpy() != 0.0, np.abs(ref.numpy()), 1.0)
    err, err_c = float(per[keep].max()), float(np.abs(got.numpy() - ref.numpy())[[loss, kl]].max())
    print(f"value_kernels={value_kernels}: surrogate message rel err per entry {per.tolist()}; cancelling sums: got {got[[loss, kl]].tolist()}, "
          f"want {ref[[loss, kl]].tolist()}; count {int(got[ppo.n_p + 1])}, gradient {got[:ppo.n_p].tolist()}")
    assert err <= 1e-12 and err_c <= 1e-12 * B and int(got[ppo.n_p + 1]) == B
    assert int((got[: ppo.n_p] != 0.0).sum()) > 3                                 # more than the cartpole's three columns
    assert np.array_equal(ppo.step_out.cpu().numpy(), got[: ppo.n_p].numpy() / B) and torch.equal(ppo.theta, theta0 + ppo.step_out)
    assert int((ppo.theta != theta0).sum()) > 3 and float(ppo.log_std) != float(ls0)
    assert torch.equal(ppo.rollout_mpc.get_theta(), ppo.theta) and torch.equal(ppo.sample_mpc.get_theta(), ppo.theta)
    # two whole iterations
    ppo.learn(2)
    st = ppo.last_stats()
    torch.cuda.synchronize()
    print("PPO statistics on the linear system:", st)
    assert torch.isfinite(ppo.theta).all() and torch.isfinite(ppo.log_std).all() and torch.isfinite(ppo.ADV).all()
    assert all(bool(torch.isfinite(p).all()) for p in ppo.policy.value_net.parameters())
    assert all(math.isfinite(v) for v in st.values()) and st["valid_fraction"] == 1.0
