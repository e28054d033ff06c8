"""GPU tests of the chain of masses as a plant and of its Q-learning loop (csrc/chain_env_kernel.hpp, mpc4rl_amd/envs.py
BatchedChainMassEnv, mpc4rl_amd/qlearning_chain.py): the two kernels against their torch statements, against each other and against the
model inside the solver, the argument checks on device pointers, ChainQLearning end to end, replayed from graphs and against
BatchedQLearning.

The kernels are compiled with floating-point contraction and the torch statement rounds once per operation, so new states and costs are
compared to TOL = 1e-12, every entry scaled by max(1, |reference|): about 10^4 unit roundoffs for a map a few hundred operations deep, six
orders below the effect of a dropped RK stage or a wrong weight.  What is copied or selected (S rows, actions, rows, masks, observations)
is compared bit for bit.  Every comparison prints its observed maximum."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
TOL = 1e-12
POISON = -7.0


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _err(got, want):
    """the largest difference, every entry scaled by max(1, |want|)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) if want.numel() else 0.0


_OCPS = {}


def _ocp(n_mass, N=8):
    from mpc4rl_amd import chain_mass_ocp
    if (n_mass, N) not in _OCPS:
        _OCPS[(n_mass, N)] = chain_mass_ocp(n_mass, N=N)
    return _OCPS[(n_mass, N)]


def _points(n_mass, E, seed):
    """States around x0, controls beyond the bounds, per-row dynamics parameters x U(0.8, 1.2), standard-normal draws (all on the CPU)."""
    from mpc4rl_amd.problems import chain_param_layout
    ocp = _ocp(n_mass)
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(ocp.x0) + 0.05 * torch.randn(E, nx, generator=g, dtype=torch.float64)
    u = torch.rand(E, 3, generator=g, dtype=torch.float64) * 3.0 - 1.5
    rows = torch.tensor(ocp.p0).repeat(E, 1)
    nd = off["C"][1]
    rows[:, :nd] *= 0.8 + 0.4 * torch.rand(E, nd, generator=g, dtype=torch.float64)
    wn = torch.randn(E, 3 * M, generator=g, dtype=torch.float64)
    return ocp, g, x, u, rows, wn


# ---------------------------------------------------------------------- 1. the plant against its statement
@pytest.mark.parametrize("E", [1, 63, 65, 130])
@pytest.mark.parametrize("n_mass", [3, 4, 5, 6, 7])
def test_env_chain_step_equals_its_statement(n_mass, E):
    """mpcrl_env_chain_step against chain_env_step_terms on both sides of a 64-lane block, with a shared and a per-row p, w_std 0 (wn NULL)
    and 0.05, double and float observations: new state and cost to TOL, obs == state bitwise, the float obs == state.float().
    Not run on the MI355X yet: no largest value is on record (every case prints its own)."""
    from mpc4rl_amd import _lib, chain_env_step_terms
    lib = _lib.load()
    ocp, g, x, u, rows, wn = _points(n_mass, E, 1000 + 10 * n_mass + E)
    x_ss = torch.tensor(ocp.consts)
    worst = 0.0
    for per_row in (False, True):
        p = rows if per_row else rows[0].clone()
        for w_std in (0.0, 0.05):
            new, cost = chain_env_step_terms(ocp, p, x_ss, x, u, wn if w_std else None, w_std)
            for f32 in (0, 1):
                state, obs = x.to(DEV).contiguous(), torch.full((E, ocp.nx), POISON, dtype=torch.float32 if f32 else torch.float64, device=DEV)
                c = torch.full((E,), POISON, **F64)
                pd, xd, ud, wd = p.to(DEV).contiguous(), x_ss.to(DEV), u.to(DEV).contiguous(), wn.to(DEV).contiguous()
                rc = lib.mpcrl_env_chain_step(n_mass, ocp.dT, ocp.rk_steps, _p(pd), ocp.n_p if per_row else 0, _p(xd), E, _p(state), _p(ud),
                                              _p(wd) if w_std else None, w_std, _p(obs), f32, _p(c), _stream())
                assert rc == 0
                torch.cuda.synchronize()
                e_x, e_c = _err(state, new), _err(c, cost)
                print(f"n_mass {n_mass} E {E} per_row {per_row} w_std {w_std} f32 {f32}: new state {e_x:.3e}, cost {e_c:.3e}")
                worst = max(worst, e_x, e_c)
                assert e_x <= TOL and e_c <= TOL
                assert torch.equal(obs, state.float() if f32 else state)
                assert torch.equal(ud.cpu(), u) and torch.equal(pd.cpu(), p)                  # inputs untouched
        assert float((chain_env_step_terms(ocp, rows, x_ss, x, u, None, 0.0)[0] - new).abs().max()) > 1e-5     # the noise is felt
    print(f"n_mass {n_mass} E {E}: largest {worst:.3e}")


# ---------------------------------------------------------------------- 2. the collect kernel against its statement, on poisoned tables
def _collect_case(n_mass, E, rows_of, sigma, w_std=0.05, per_row=True):
    """One call of mpcrl_qlearning_chain_collect and what the statement says every buffer holds afterwards."""
    from mpc4rl_amd import _lib, chain_collect_terms
    lib = _lib.load()
    T = 3
    ocp, g, x, u0, rows, _ = _points(n_mass, E, 2000 + 10 * n_mass + E)
    M, nx = n_mass - 2, ocp.nx
    i = torch.arange(E)
    status = torch.where(i % 5 == 2, 4, torch.where(i % 5 == 1, 2, torch.where(i % 5 == 4, 1, 0))).to(torch.int32)
    if E > 1:
        u0[i % 7 == 3, 1], u0[i % 11 == 5, 2] = float("nan"), float("inf")               # one component only
    eps = (torch.randn(T, E, 3, generator=g) * 8.0).float()                               # sigma eps clips at both ends
    wn = torch.randn(T, E, 3 * M, generator=g, dtype=torch.float64)
    row = torch.tensor(rows_of, dtype=torch.int32)[i % len(rows_of)].contiguous()
    p = rows if per_row else rows[0].clone()
    x_ss = torch.tensor(ocp.consts)
    lo, hi = [-1.0, -0.5, -1.0], [1.0, 1.0, 0.25]
    d = lambda t: t.to(DEV).contiguous()
    state, obs, cold = d(x), torch.full((E, nx), POISON, **F64), torch.ones(E, dtype=torch.int32, device=DEV)
    S, A, Cc = torch.full((T, E, nx), POISON, **F64), torch.full((T, E, 3), POISON, **F64), torch.full((T, E), POISON, **F64)
    row_d, pd, xd, ud, sd, ed, wd = d(row), d(p), d(x_ss), d(u0), d(status), d(eps), d(wn)
    rc = lib.mpcrl_qlearning_chain_collect(n_mass, ocp.dT, ocp.rk_steps, _p(pd), ocp.n_p if per_row else 0, _p(xd), w_std, E, T, _p(state), _p(ud),
                                           _p(sd), _p(ed), _p(wd) if w_std else None, (C.c_double * 3)(*lo), (C.c_double * 3)(*hi), sigma, _p(obs), _p(row_d),
                                           _p(cold), _p(S), _p(A), _p(Cc), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    on = (row >= 0) & (row < T)
    r = row.clamp(0, T - 1).long()
    act, new, cost = chain_collect_terms(ocp, p, x_ss, x, u0, status, eps[r, i], wn[r, i], w_std, lo, hi, sigma)
    S0, A0, C0 = torch.full((T, E, nx), POISON, dtype=torch.float64), torch.full((T, E, 3), POISON, dtype=torch.float64), torch.full((T, E), POISON, dtype=torch.float64)
    S0[r[on], i[on]], A0[r[on], i[on]], C0[r[on], i[on]] = x[on], act[on], cost[on]
    want = dict(state=torch.where(on[:, None], new, x), obs=torch.where(on[:, None], new, torch.full_like(x, POISON)),
                cold=torch.where(on, 0, 1).to(torch.int32), row=torch.where(on, row + 1, row).to(torch.int32), S=S0, A=A0, C=C0)
    got = dict(state=state, obs=obs, cold=cold, row=row_d, S=S, A=A, C=Cc)
    good = ((status == 0) | (status == 2)) & torch.isfinite(u0).all(1)
    return got, want, dict(on=on, act=act, good=good, u0=u0, r=r, i=i, status=status, pd=pd, wd=wd, ocp=ocp, lo=lo, hi=hi)


def _check_collect(got, want, x):
    on = x["on"]
    for name in ("A", "S", "row", "cold"):                                          # copies and selections: the bits
        assert torch.equal(got[name].cpu(), want[name]), name
    assert torch.equal(got["obs"], got["state"]) if bool(on.all()) else torch.equal(got["obs"].cpu()[on], got["state"].cpu()[on])
    assert torch.equal(got["obs"].cpu()[~on], want["obs"][~on]) and torch.equal(got["state"].cpu()[~on], want["state"][~on])     # untouched
    e_x, e_c = _err(got["state"], want["state"]), _err(got["C"], want["C"])
    assert e_x <= TOL and e_c <= TOL, (e_x, e_c)
    return max(e_x, e_c)


@pytest.mark.parametrize("sigma", [0.0, 0.25])
@pytest.mark.parametrize("E,rows_of", [(65, (0, 2, 3, -1)), (1, (0,)), (1, (2,)), (1, (3,)), (1, (-1,))])
@pytest.mark.parametrize("n_mass", [3, 5])
def test_collect_equals_its_statement_on_poisoned_tables(n_mass, E, rows_of, sigma):
    """T = 3; rows 0, T - 1, T and -1 (a row outside the table: that lane writes nothing anywhere — the whole poisoned buffers are
    compared); two workgroups with a ragged tail and a single lane; statuses 0, 1, 2, 4, a NaN or an inf in ONE component of u0 (a zero
    action in all three before the noise); sigma = 0 (A is u0's bits, beyond the bounds) and sigma > 0 with draws that clip at both ends
    of per-component bounds.  A, the S row, row, cold and obs are exact; the new state and C hold to TOL.
    Not run on the MI355X yet: no largest value is on record (every case prints its own)."""
    got, want, x = _collect_case(n_mass, E, rows_of, sigma)
    worst = _check_collect(got, want, x)
    print(f"n_mass {n_mass} E {E} rows {rows_of} sigma {sigma}: new state / C largest {worst:.3e}")
    if E > 1:
        on, act, good, u0 = x["on"], x["act"], x["good"], x["u0"]
        assert 0 < int(on.sum()) < E and 0 < int(good.sum()) < E
        assert sorted(set(x["status"][~good].tolist())) == [0, 1, 2, 4] and bool(torch.isfinite(act).all())
        if sigma == 0.0:
            assert float(act[~good].abs().max()) == 0.0                            # rejected: zero in all three components
            assert torch.equal(act[good], u0[good]) and float(act.abs().max()) > 1.0      # u0 itself, not clipped
        else:
            lo, hi = torch.tensor(x["lo"], dtype=torch.float64), torch.tensor(x["hi"], dtype=torch.float64)
            assert bool((act >= lo).all()) and bool((act <= hi).all())
            for j in range(3):
                assert bool((act[:, j] == lo[j]).any()) and bool((act[:, j] == hi[j]).any()) and bool(((act[:, j] > lo[j]) & (act[:, j] < hi[j])).any())


def test_collect_with_a_shared_p_and_without_noise():
    """p_stride = 0 and w_std = 0 with a NULL wn: the other two paths of the collect kernel's arguments."""
    from mpc4rl_amd import _lib
    got, want, x = _collect_case(4, 65, (0, 1, 2), 0.25, w_std=0.0, per_row=False)
    _check_collect(got, want, x)


# ---------------------------------------------------------------------- 3. one step function
@pytest.mark.parametrize("n_mass", [3, 5, 7])
def test_collect_and_env_step_share_their_step_function_bitwise(n_mass):
    """The collect kernel's new state and cost equal mpcrl_env_chain_step's bit for bit for the same action and draws."""
    from mpc4rl_amd import _lib
    lib = _lib.load()
    E = 65
    got, want, x = _collect_case(n_mass, E, (0, 1, 2), 0.25)
    ocp, r, i = x["ocp"], x["r"], x["i"]
    _, _, x0, _, _, _ = _points(n_mass, E, 2000 + 10 * n_mass + E)
    state, cost = x0.to(DEV).contiguous(), torch.full((E,), POISON, **F64)
    act = got["A"][r.to(DEV), i.to(DEV)].contiguous()
    wn = x["wd"][r.to(DEV), i.to(DEV)].contiguous()
    assert torch.equal(got["S"][r.to(DEV), i.to(DEV)], state)
    assert lib.mpcrl_env_chain_step(n_mass, ocp.dT, ocp.rk_steps, _p(x["pd"]), ocp.n_p, _p(torch.tensor(ocp.consts, **F64)), E, _p(state), _p(act),
                                    _p(wn), 0.05, None, 0, _p(cost), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(state, got["state"]) and torch.equal(cost, got["C"][r.to(DEV), i.to(DEV)])
    assert float((state.cpu() - x0).abs().max()) > 1e-3


# ---------------------------------------------------------------------- 4. the plant is the model's map
def test_plant_is_the_models_map():
    """n_mass 3, N 8, E 4, p = ocp.p0, no disturbance: after MPCBatch.solve(x0) with status 0 everywhere, env.step(u0) from x0 reproduces
    row 1 of the stored x iterate to the solver's tolerance ocp.tol = 1e-5 (scaled) — the iterate satisfies x_1 = F(x_0, u_0) to that
    residual.  A plant that is not the model's map misses by orders more."""
    from mpc4rl_amd import BatchedChainMassEnv, MPCBatch
    E = 4
    ocp = _ocp(3)
    env = BatchedChainMassEnv(E, ocp, device=DEV, seed=2)
    x0 = env.reset()
    mpc = MPCBatch(ocp, E, DEV)
    r = mpc.solve(x0, cold=True)
    assert bool((r.status == 0).all())
    xs = mpc.get_iterate()[0]
    assert _err(xs[:, 0], x0) <= ocp.tol
    obs, cost, term, trunc = env.step(r.u0)
    torch.cuda.synchronize()
    err = _err(obs, xs[:, 1])
    print(f"plant against the solver's x_1: {err:.3e} (moved {float((obs - x0).abs().max()):.3e})")
    assert err <= ocp.tol and float((obs - x0).abs().max()) > 100 * ocp.tol
    assert torch.equal(obs, env.state) and not bool(term.any()) and not bool(trunc.any()) and float(cost.min()) > 0.0


# ---------------------------------------------------------------------- 5. ChainQLearning end to end
def _learner(n_mass, E, T, lr, seed=2, graphs=False, **kw):
    from mpc4rl_amd import BatchedChainMassEnv, ChainQLearning
    from mpc4rl_amd.problems import chain_param_layout
    ocp = _ocp(n_mass)
    off = chain_param_layout(n_mass)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1
    p[off["D"][0]: off["D"][1]] *= 0.9
    env = BatchedChainMassEnv(E, ocp, device=DEV, p=p, w_std=0.01, vel_std=1e-2, seed=seed - 1)
    ql = ChainQLearning(ocp, env, T, lr=lr, noise_scale=0.05, seed=seed, **kw)
    if graphs:
        ql.enable_graphs()
    return ql


def _check_episode(ql, st, theta0, x0):
    from mpc4rl_amd import chain_collect_terms, qlearning_td_terms
    T, E, n, env = ql.T, ql.E, ql.T - 1, ql.env
    S, A, Cc = ql.S.cpu(), ql.A.cpu(), ql.C.cpu()
    assert torch.equal(S[0], x0.cpu()) and len(ql.last) == T
    worst = 0.0
    for t in range(T):
        r = ql.last[t]
        assert bool(((r.status == 0) | (r.status == 2)).all())
        act, new, cost = chain_collect_terms(ql.ocp, env.p.cpu(), env.x_ss.cpu(), S[t], r.u0.cpu(), r.status.cpu(), ql.eps[t].cpu(), ql.wn[t].cpu(),
                                             env.w_std, list(ql.lo_v), list(ql.hi_v), ql.noise_scale)
        assert torch.equal(A[t], act), t                          # no product in it that contraction could fuse
        e_c, e_x = _err(Cc[t], cost), _err(S[t + 1] if t + 1 < T else env.state, new)
        worst = max(worst, e_c, e_x)
        assert e_c <= TOL and e_x <= TOL, (t, e_c, e_x)
    assert torch.equal(ql.obs, env.state) and bool((ql.row == T).all()) and bool((ql.cold == 0).all())
    rq, rv = ql.last_sweep
    msg, td, valid = qlearning_td_terms(rq.V.reshape(n, E).cpu(), rv.V.reshape(n, E).cpu(), rq.dV_dp.reshape(n, E, -1).cpu(), rq.status.reshape(n, E).cpu(),
                                        rv.status.reshape(n, E).cpu(), Cc, ql.live.cpu(), ql.gamma, ql.lr)
    assert torch.equal(ql.valid.cpu().bool(), valid) and torch.equal(ql.td.cpu(), td)
    np.testing.assert_allclose(ql.msg.cpu().numpy(), msg.numpy(), rtol=1e-12, atol=1e-18)
    count = float(ql.msg[-1])
    print(f"table rows largest {worst:.3e}; count {count}, converged {st.converged_fraction}, |step| {float(ql.step_out.norm()):.3e}, "
          f"iterations Q {int(rq.iters[:, 0].max())} V {int(rv.iters[:, 0].max())}")
    assert count == (T - 2) * E == float(valid.sum()) and st.converged_fraction == 1.0         # no instance is left out
    mask = ql.learn_mask.cpu() != 0.0
    step = ql.step_out.cpu()
    assert torch.equal(st.step, ql.step_out) and np.array_equal(step[mask].numpy(), (ql.msg[: ql.n_p].cpu() / max(1.0, count))[mask].numpy())
    assert torch.equal(ql.theta, theta0 + ql.step_out) and float(step[~mask].abs().max()) == 0.0 and int((step[mask] != 0.0).sum()) > 3
    assert torch.equal(ql.rollout_mpc.get_theta(), ql.theta) and torch.equal(ql.sample_mpc.get_theta(), ql.theta)
    assert math.isclose(st.total_cost, float(Cc.sum()) / E, rel_tol=1e-12) and math.isclose(st.td_error_mean, float(td.sum()) / count, rel_tol=1e-12)


@pytest.mark.parametrize("n_mass,E,T,lr", [(3, 4, 5, 1e-5), (5, 3, 4, 1e-6)])
def test_chain_qlearning_two_episodes(n_mass, E, T, lr):
    """N = 8, two eager episodes (the second from given initial states), m x 1.1 and D x 0.9 in the plant, vel_std 1e-2, noise_scale 0.05,
    w_std 0.01: the table rows against chain_collect_terms on the learner's own solves and draws, the TD step against qlearning_td_terms
    on its sweep, theta moved by step_out inside the learn mask only, both handles at theta, every term valid."""
    from mpc4rl_amd import BatchedChainMassEnv
    from mpc4rl_amd.problems import chain_param_layout
    ql = _learner(n_mass, E, T, lr)
    ocp, off = ql.ocp, chain_param_layout(n_mass)[4]
    assert ql.NX == ocp.nx and ql.NU == 3 and ql.gamma == ocp.gamma and ql.A.shape == (T, E, 3) and ql.wn.shape == (T, E, 3 * (n_mass - 2))
    assert float(ql.learn_mask.sum()) == off["C"][1] and float(ql.learn_mask[off["C"][1]:].sum()) == 0.0      # m, D, L, C
    ws = ql.workspace_bytes()
    assert ws == (ql.rollout_mpc.workspace_bytes(), ql.sample_mpc.workspace_bytes()) and ws[1] > ws[0] > 0
    twin = BatchedChainMassEnv(E, ocp, device=DEV, seed=1)                         # the learner's environment, reset once
    g = torch.Generator().manual_seed(9)
    x1 = torch.tensor(ocp.x0) + 0.02 * torch.randn(E, ocp.nx, generator=g, dtype=torch.float64)
    for x0 in (None, x1.to(DEV)):
        theta0 = ql.theta.clone()
        st = ql.run_episode(x0)
        torch.cuda.synchronize()
        _check_episode(ql, st, theta0, twin.reset() if x0 is None else x0)
    assert ql.episodes == 2


def test_one_control_learners_keep_their_shapes():
    """LinearQLearning after the generalisation of DeviceQLearning to NU controls: A and eps [T, E], float bounds, zero buffers before the
    first episode."""
    from mpc4rl_amd import BatchedLinearSystemEnv, LinearQLearning, linear_system_ocp
    ql = LinearQLearning(linear_system_ocp(), BatchedLinearSystemEnv(4, device=DEV), 3)
    assert ql.NU == 1 and ql.A.shape == (3, 4) and ql.eps.shape == (3, 4) and ql.S.shape == (3, 4, 2) and ql.eps.dtype == torch.float32
    assert (ql.lo, ql.hi) == (-1.0, 1.0) and not hasattr(ql, "lo_v") and float(ql.obs.abs().sum()) == 0.0 and float(ql.S.abs().sum()) == 0.0


def test_chain_qlearning_T2_is_an_empty_step():
    ql = _learner(3, 4, 2, 1e-5)
    theta0 = ql.theta.clone()
    st = ql.run_episode()
    torch.cuda.synchronize()
    assert float(ql.msg.abs().sum()) == 0.0 and torch.equal(ql.theta, theta0) and float(st.step.abs().sum()) == 0.0
    assert st.converged_fraction == 1.0 and st.total_cost > 0.0


def test_chain_qlearning_learn_blocks():
    """learn = ("Q", "w"): the mask is those blocks and nothing else moves."""
    from mpc4rl_amd.problems import chain_param_layout
    ql = _learner(3, 4, 4, 1e-7, learn=("Q", "w"))
    off = chain_param_layout(3)[4]
    mask = torch.zeros(ql.n_p, dtype=torch.bool)
    mask[off["Q"][0]: off["Q"][1]], mask[off["w"][0]: off["w"][1]] = True, True
    assert torch.equal(ql.learn_mask.cpu() != 0.0, mask)
    ql.run_episode()
    torch.cuda.synchronize()
    step = ql.step_out.cpu()
    assert float(step[~mask].abs().max()) == 0.0 and int((step[mask] != 0.0).sum()) > 3


# ---------------------------------------------------------------------- 6. graphs
def test_chain_qlearning_graphs_equal_eager():
    """n_mass 3, N 8, E 65, T 4: two episodes replayed from the captured graphs (the second from given initial states) give the bits of
    two eager episodes of a learner with the same seeds: theta, S, A, C, the TD terms and the message."""
    E, T = 65, 4
    ocp = _ocp(3)
    x1 = (torch.tensor(ocp.x0) + 0.02 * torch.randn(E, ocp.nx, generator=torch.Generator().manual_seed(4), dtype=torch.float64)).to(DEV)
    runs = []
    for graphs in (False, True):
        ql = _learner(3, E, T, 1e-5, seed=6, graphs=graphs)
        out = []
        for x0 in (None, x1):
            st = ql.run_episode(x0)
            out.append((st, ql.theta.clone(), [t.clone() for t in (ql.S, ql.A, ql.C, ql.td, ql.valid, ql.msg)]))
        runs.append(out)
    torch.cuda.synchronize()
    for (se, te, tabs_e), (sg, tg, tabs_g) in zip(*runs):
        assert torch.equal(te, tg) and torch.equal(se.step, sg.step)
        for name, a, b in zip(("S", "A", "C", "td", "valid", "msg"), tabs_e, tabs_g):
            assert torch.equal(a, b), name
        assert (se.total_cost, se.td_error_mean, se.converged_fraction) == (sg.total_cost, sg.td_error_mean, sg.converged_fraction)
    assert float(runs[0][0][0].step.abs().max()) > 0.0 and not torch.equal(runs[0][0][1], runs[0][1][1])


# ---------------------------------------------------------------------- 7. against the torch form
STEP_BOUND = 1e-7          # of the step's norm (see the test's docstring); the ceiling is 1e-4


def test_chain_qlearning_agrees_with_batched_qlearning():
    """One episode of each from the same reset, n_mass 3, N 8, E 4, T 5, without noise or exploration, every block learned (BatchedQLearning
    has no mask).  BatchedQLearning takes the chain environment as it is and is the reference.  S, A and C are the same bits: the roll-outs
    start from the same cold iterates and step through the same kernel function.  The parameter steps differ only through how the V solve
    starts (from the Q solve's iterate against cold).  The bound is meant to be ten times the difference measured on the MI355X; this
    test has NOT run there yet, so STEP_BOUND stands on an estimate instead: the oracle's C++ port gave 1e-11 relative between a warm and
    a cold V; without plant mismatch or noise the TD errors are only the receding horizon's, some 1e-3 of V, so a step that is linear in
    them moves by about 1e-11 / 1e-3 = 1e-8 of its norm, and ten times that is 1e-7 — three orders inside the 1e-4 ceiling.  The test
    prints the figure that should replace the estimate."""
    from mpc4rl_amd import BatchedChainMassEnv, BatchedQLearning, ChainQLearning
    E, T, lr = 4, 5, 1e-5
    ocp = _ocp(3)
    new = ChainQLearning(ocp, BatchedChainMassEnv(E, ocp, device=DEV, seed=1), T, lr=lr, noise_scale=0.0, learn=ChainQLearning.BLOCKS)
    old = BatchedQLearning(ocp, BatchedChainMassEnv(E, ocp, device=DEV, seed=1), T, lr=lr, device=DEV)
    s_new, s_old = new.run_episode(), old.run_episode()
    torch.cuda.synchronize()
    S, A, Cc = old.last_episode
    norm = float(s_old.step.norm())
    d_step = float((s_new.step - s_old.step).abs().max())
    d_S, d_A, d_C = float((new.S - S).abs().max()), float((new.A - A).abs().max()), float((new.C - Cc).abs().max())
    print(f"step norm {norm:.6e}; max |step difference| {d_step:.3e} ({d_step / norm:.3e} of the norm); S {d_S:.3e}, A {d_A:.3e}, C {d_C:.3e}; "
          f"theta {float((new.theta - old.theta).abs().max()):.3e}")
    assert s_new.converged_fraction == 1.0 and s_old.converged_fraction == 1.0
    assert norm > 0.0 and float(Cc.abs().max()) > 0.0 and float(A.abs().max()) > 0.0
    assert STEP_BOUND <= 1e-4 and d_step <= STEP_BOUND * norm
    assert torch.equal(new.S, S) and torch.equal(new.A, A) and torch.equal(new.C, Cc)


# ---------------------------------------------------------------------- 8. argument errors on device pointers
def test_argument_errors():
    from mpc4rl_amd import _lib
    lib = _lib.load()
    E, T, n_mass = 4, 3, 3
    ocp = _ocp(n_mass)
    nx, n_p = ocp.nx, ocp.n_p
    p, x_ss = torch.tensor(ocp.p0, **F64).repeat(E, 1), torch.tensor(ocp.consts, **F64)
    state = torch.tensor(ocp.x0, **F64).repeat(E, 1)
    z = torch.zeros(T, E, nx, **F64)
    zi, zf = torch.zeros(E, dtype=torch.int32, device=DEV), torch.zeros(T, E, 3, dtype=torch.float32, device=DEV)
    row = torch.full((E,), T, dtype=torch.int32, device=DEV)                      # a full table: a call that does launch writes nothing
    lo, hi = (C.c_double * 3)(-1.0, -1.0, -1.0), (C.c_double * 3)(1.0, 1.0, 1.0)
    host = (C.c_double * (E * nx))()

    st2, c2 = state.clone(), torch.zeros(E, **F64)                                 # what the two valid calls of step write

    def step(n_mass=n_mass, Ts=0.2, rk=2, p=p, stride=n_p, B=E, state=_p(st2), action=z, wn=z, w_std=0.05, cost=c2):
        return lib.mpcrl_env_chain_step(n_mass, Ts, rk, _p(p), stride, _p(x_ss), B, state, _p(action), _p(wn), w_std, None, 0, _p(cost), _stream())

    def coll(n_mass=n_mass, Ts=0.2, rk=2, p=p, stride=n_p, E=E, T=T, state=_p(state), S=z, wn=z, w_std=0.05, lo=lo, hi=hi):
        return lib.mpcrl_qlearning_chain_collect(n_mass, Ts, rk, _p(p), stride, _p(x_ss), w_std, E, T, state, _p(z), _p(zi), _p(zf), _p(wn), lo, hi, 0.0,
                                                 _p(z), _p(row), _p(zi), _p(S), _p(z), _p(z), _stream())

    for f in (step, coll):
        assert f(n_mass=2) == -1 and f(n_mass=8) == -1 and f(rk=0) == -1 and f(Ts=0.0) == -1 and f(Ts=-1.0) == -1
        assert f(stride=n_p + 1) == -1 and f(stride=1) == -1 and f(p=None) == -1 and f(state=None) == -1
        assert f(wn=None) == -1 and f(wn=None, w_std=0.0) == 0
        assert f(state=C.cast(host, C.c_void_p)) == -1                            # not device memory
    assert step(B=-1) == -1 and step(action=None) == -1 and step(cost=None) == -1 and step(B=0) == 0
    assert coll(E=-1) == -1 and coll(T=0) == -1 and coll(S=None) == -1 and coll(lo=None) == -1 and coll(hi=lo) == -1 and coll(E=0) == 0
    assert coll() == 0 and coll(stride=0) == 0 and step() == 0 and step(stride=0) == 0
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0.0 and bool((row == T).all()) and torch.equal(state, torch.tensor(ocp.x0, **F64).repeat(E, 1))
    assert bool(torch.isfinite(st2).all()) and not torch.equal(st2, state) and float(c2.min()) > 0.0
