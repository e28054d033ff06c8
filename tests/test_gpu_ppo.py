"""GPU tests of batched PPO with the MPC as Gaussian actor (mpc4rl_amd/ppo.py, csrc/ppo_kernel.hpp): the roll-out kernel against its
torch statement and the environment kernels it stands for, the GAE and surrogate kernels against their torch float64 statements, the
surrogate's parameter gradient through the solver against central finite differences, and two iterations of the learner."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _rel(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / np.where(want != 0.0, np.abs(want), 1.0))) if got.size else 0.0


class _Tables:
    def __init__(self, T, E):
        self.OBS, self.NEXT = torch.full((T, E, 4), -7.0, **F64), torch.full((T, E, 4), -7.0, **F64)
        self.ACT, self.LOGP, self.VAL, self.REW = (torch.full((T, E), -7.0, **F64) for _ in range(4))
        self.TERM, self.DONE, self.OK = (torch.full((T, E), 9, dtype=torch.uint8, device=DEV) for _ in range(3))

    def all(self):
        return (self.OBS, self.ACT, self.LOGP, self.VAL, self.REW, self.NEXT, self.TERM, self.DONE, self.OK)


def _collect(lib, env, T, t, u0, status, eps, u01, value, log_std, lo, hi, rs, tab, obs, ended):
    return lib.mpcrl_ppo_cartpole_collect(env._par(), env.num_envs, T, t, _p(env.state), _p(env.steps), _p(u0), _p(status), _p(eps), _p(u01), _p(value),
                                          _p(log_std), lo, hi, rs, *[_p(x) for x in tab.all()], _p(obs), _p(ended), _stream())


@pytest.mark.parametrize("E", [1, 63, 64, 65, 257])
def test_collect_matches_torch_statement_and_environment_kernels(E):
    """Row t of the tables and the environments after mpcrl_ppo_cartpole_collect: ACT, LOGP against ppo_collect_terms at 1e-12; the state,
    reward, flags and the reset pattern bit-equal to mpcrl_env_cartpole_step (with the clip of the recorded action) followed by
    mpcrl_env_cartpole_reset.  Environment 0 sits one step from truncation, environment E // 2 inside the terminal box (E = 1: both)."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, _lib, ppo_collect_terms
    lib = _lib.load()
    T, t, lo, hi, rs, ls = 3, 1, -30.0, 30.0, -0.5, 0.4
    g = torch.Generator(device=DEV).manual_seed(E)
    x0 = (torch.rand(E, 4, generator=g, **F64) * 2 - 1) * torch.tensor([0.5, 1.0, 0.3, 1.0], **F64)
    x0[:, 2] += math.pi * (torch.arange(E, device=DEV) % 2)
    x0[E // 2] = torch.tensor([0.01, 0.0, 0.005, 0.0], **F64)
    i = torch.arange(E, device=DEV)
    status = torch.where(i % 7 == 3, 4, torch.where(i % 7 == 5, 2, torch.where(i % 13 == 9, 1, 0))).to(torch.int32)
    u0 = (torch.rand(E, generator=g, **F64) * 2 - 1) * 33.0                # beyond the bounds too
    u0[i % 11 == 6] = float("nan")
    status[E // 2], u0[E // 2] = 0, 0.0                                    # zero action, no noise: the environment stays in the box
    eps = torch.randn(E, generator=g, dtype=torch.float32, device=DEV) * 2.0   # sigma eps beyond +-1 for many: the clip
    eps[E // 2] = 0.0
    u01 = torch.rand(E, generator=g, **F64)
    value = torch.randn(E, generator=g, **F64)
    log_std = torch.tensor([ls], **F64)
    envs = [BatchedCartPoleSwingUpEnv(E, device=DEV, seed=0, max_episode_steps=45) for _ in range(2)]
    for env in envs:
        env.state.copy_(x0), env.steps.copy_(i % 5)
        env.steps[0] = 44
    env, ref = envs
    tab = _Tables(T, E)
    obs, ended = torch.full((E, 4), -7.0, **F64), torch.full((E,), 9, dtype=torch.int32, device=DEV)
    assert _collect(lib, env, T, t, u0, status, eps, u01, value, log_std, lo, hi, rs, tab, obs, ended) == 0
    torch.cuda.synchronize()
    # the torch statement
    mu, act, logp, ok = ppo_collect_terms(u0.cpu(), status.cpu(), eps.cpu(), ls, lo, hi)
    e_act, e_logp = _rel(tab.ACT[t].cpu().numpy(), act.numpy()), _rel(tab.LOGP[t].cpu().numpy(), logp.numpy())
    print(f"E={E}: ACT rel err {e_act:.2e}, LOGP rel err {e_logp:.2e}")
    assert e_act <= 1e-12 and e_logp <= 1e-12
    assert torch.equal(tab.OK[t].cpu().bool(), ok) and torch.equal(tab.VAL[t], value) and torch.equal(tab.OBS[t], x0)
    if E >= 63:
        assert {0, 2, 4} <= set(status.tolist()) and int(torch.isnan(u0).sum()) > 0 and 0 < int(ok.sum()) < E
        assert float(mu[~ok].abs().max()) == 0.0
    # the environment kernels on the recorded action
    a_applied = tab.ACT[t].clamp(-1.0, 1.0)
    nxt, rew, term, trunc = ref.step(a_applied)
    done = term | trunc
    assert torch.equal(tab.NEXT[t], nxt) and torch.equal(tab.REW[t], rs * rew)
    assert torch.equal(tab.TERM[t].bool(), term) and torch.equal(tab.DONE[t].bool(), done)
    assert bool(trunc[0]) and bool(term[E // 2]) and (E == 1 or not bool(done.all()))
    ref_obs = torch.empty(E, 4, **F64)
    assert lib.mpcrl_env_cartpole_reset(E, _p(ref.state), _p(ref.steps), _p(done.to(torch.uint8)), _p(u01), _p(ref_obs), 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(env.state, ref.state) and torch.equal(env.steps, ref.steps) and torch.equal(obs, ref_obs)
    assert torch.equal(ended.bool(), done) and bool((env.steps[done] == 0).all())
    # the other rows are untouched
    for x in tab.all():
        for row in (0, 2):
            assert bool((x[row] == (9 if x.dtype == torch.uint8 else -7.0)).all())
    # misuse
    assert _collect(lib, env, T, T, u0, status, eps, u01, value, log_std, lo, hi, rs, tab, obs, ended) == -1
    assert _collect(lib, env, T, -1, u0, status, eps, u01, value, log_std, lo, hi, rs, tab, obs, ended) == -1
    assert _collect(lib, env, T, t, u0, status, eps, u01, value, log_std, hi, lo, rs, tab, obs, ended) == -1
    assert _collect(lib, env, T, t, u0, status, eps, u01, None, log_std, lo, hi, rs, tab, obs, ended) == -1


@pytest.mark.parametrize("E", [1, 65, 257])
@pytest.mark.parametrize("T", [1, 2, 33])
def test_gae_kernel_matches_torch_statement(T, E):
    from mpc4rl_amd import _lib, ppo_gae
    lib = _lib.load()
    rng = np.random.default_rng(1000 * T + E)
    gamma, lam = 0.99, 0.95
    rew, val, vnext = rng.normal(-2, 1, (T, E)), rng.normal(-20, 5, (T, E)), rng.normal(-20, 5, (T, E))
    term, trunc = rng.uniform(size=(T, E)) < 0.15, rng.uniform(size=(T, E)) < 0.15
    trunc[T - 1, ::3] = True
    done = term | trunc
    c = [torch.as_tensor(a) for a in (rew, val, vnext, term.astype(np.uint8), done.astype(np.uint8))]
    d = [x.to(DEV).contiguous() for x in c]
    adv, ret = torch.full((T, E), -7.0, **F64), torch.full((T, E), -7.0, **F64)
    assert lib.mpcrl_ppo_gae(*[_p(x) for x in d], T, E, gamma, lam, _p(adv), _p(ret), _stream()) == 0
    torch.cuda.synchronize()
    adv_ref, ret_ref = ppo_gae(*c, gamma, lam)
    e_adv, e_ret = _rel(adv.cpu().numpy(), adv_ref.numpy()), _rel(ret.cpu().numpy(), ret_ref.numpy())
    print(f"T={T} E={E}: ADV rel err {e_adv:.2e}, RET rel err {e_ret:.2e}")
    assert e_adv <= 1e-12 and e_ret <= 1e-12
    assert lib.mpcrl_ppo_gae(*[_p(x) for x in d], 0, E, gamma, lam, _p(adv), _p(ret), _stream()) == -1
    assert lib.mpcrl_ppo_gae(*[_p(x) for x in d[:4]], None, T, E, gamma, lam, _p(adv), _p(ret), _stream()) == -1


def _surrogate_inputs(M, n_p, seed):
    """A minibatch over a table of 2 M + 5 rows: ratios on both sides of the clip band, advantages of both signs, rows left out for every
    reason (OK = 0, a rejected re-solve, NaN u0_new, a non-finite table entry, an index outside the table) where M allows."""
    from mpc4rl_amd import ppo_collect_terms
    rng = np.random.default_rng(seed)
    n_rows, lo, hi, ls = 2 * M + 5, -30.0, 30.0, -0.5
    u0 = rng.uniform(-20, 20, n_rows)
    status = np.where(rng.uniform(size=n_rows) < 0.1, 4, np.where(rng.uniform(size=n_rows) < 0.1, 2, 0)).astype(np.int32)
    eps = rng.normal(size=n_rows).astype(np.float32)
    _, act, logp, ok = ppo_collect_terms(torch.as_tensor(u0), torch.as_tensor(status), torch.as_tensor(eps), ls, lo, hi)
    adv = torch.as_tensor(rng.normal(0.3, 1.0, n_rows))
    idx = rng.permutation(n_rows)[:M].astype(np.int64)
    u0_new = u0[idx] + rng.uniform(-1, 1, M) * 0.8 * math.exp(ls) * 0.5 * (hi - lo)
    status_new = np.where(rng.uniform(size=M) < 0.08, 4, np.where(rng.uniform(size=M) < 0.1, 2, 0)).astype(np.int32)
    dpi = rng.normal(size=(M, 1, n_p))
    dpi[status_new == 4] = np.nan
    if M > 8:
        u0_new[3], dpi[3] = np.nan, np.inf
        adv[idx[5]] = float("inf")
        idx[6], idx[7] = -1, n_rows
        dpi[8, 0, n_p - 1] = np.nan                               # a NaN entry of a row that may be left in: read as nan_to_num does
    return dict(idx=torch.as_tensor(idx), act=act, logp=logp, adv=adv, ok=ok.to(torch.uint8), u0_new=torch.as_tensor(u0_new),
                status_new=torch.as_tensor(status_new), dpi_dp=torch.as_tensor(dpi), log_std=ls, lo=lo, hi=hi)


def _surrogate_call(lib, c, ws, clip, ent, lr, norm, msg):
    M, n_p = c["idx"].numel(), c["dpi_dp"].shape[-1]
    return lib.mpcrl_ppo_surrogate_grad(_p(c["idx"]), M, c["act"].numel(), _p(c["act"]), _p(c["logp"]), _p(c["adv"]), _p(c["ok"]), _p(c["u0_new"]),
                                        _p(c["status_new"]), _p(c["dpi_dp"]), n_p, _p(c["log_std"]), c["lo"], c["hi"], clip, ent, lr, norm, _p(ws),
                                        _p(msg), _stream())


@pytest.mark.parametrize("M,n_p", [(M, n_p) for n_p in (3, 83) for M in (1, 127, 129, 300)] + [(520, 251)])
def test_surrogate_kernel_matches_torch_statement(M, n_p):
    """msg of mpcrl_ppo_surrogate_grad against ppo_surrogate_terms at 1e-12 relative on every entry, with and without advantage
    normalisation; the call repeated gives equal bits; the workspace is all zero afterwards.  (520, 251): five workgroups, the last one
    ragged, and n_p + 6 = 257 entries — a second chunk, of one entry, in the final sum."""
    from mpc4rl_amd import _lib, ppo_surrogate_terms
    lib = _lib.load()
    clip, ent, lr = 0.2, 0.01, 3e-3
    c = _surrogate_inputs(M, n_p, 100 * M + n_p)
    d = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}
    d["log_std"] = torch.tensor([c["log_std"]], **F64)
    nb = int(lib.mpcrl_ppo_surrogate_workspace_bytes(M, n_p))
    assert nb >= 16 + 8 * (n_p + 6) * ((M + 127) // 128)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    for norm in (1, 0):
        msgs = []
        for _ in range(2):
            msg = torch.full((n_p + 8,), -5.0, **F64)
            assert _surrogate_call(lib, d, ws, clip, ent, lr, norm, msg) == 0
            msgs.append(msg)
        torch.cuda.synchronize()
        assert torch.equal(msgs[0], msgs[1])                                   # same inputs, same bits
        assert int(ws.count_nonzero()) == 0                                    # the workspace is left zero
        ref = ppo_surrogate_terms(**c, clip_range=clip, ent_coef=ent, lr=lr, normalize_adv=bool(norm))
        got = msgs[0].cpu()
        assert torch.isfinite(got).all() and torch.isfinite(ref).all()
        err = _rel(got.numpy(), ref.numpy())
        print(f"M={M} n_p={n_p} normalize={norm}: count {int(got[n_p + 1])}, clipped {int(got[n_p + 4])}, max rel err {err:.2e}")
        assert int(got[n_p + 1]) == int(ref[n_p + 1]) and (M == 1 or 0 < int(got[n_p + 1]) < M)
        assert err <= 1e-12
    msg = torch.zeros(n_p + 8, **F64)
    assert _surrogate_call(lib, d, None, clip, ent, lr, 1, msg) == -1
    assert _surrogate_call(lib, d, ws, 0.0, ent, lr, 1, msg) == -1
    assert _surrogate_call(lib, {**d, "lo": 30.0}, ws, clip, ent, lr, 1, msg) == -1
    assert lib.mpcrl_ppo_surrogate_workspace_bytes(0, n_p) == -1


def test_log_std_apply_is_the_masked_mean():
    from mpc4rl_amd import _lib
    lib = _lib.load()
    n_p = 5
    for count, want in ((4.0, 0.25 - 0.75 / 4.0), (0.0, 0.25 - 0.75)):
        msg = torch.zeros(n_p + 8, **F64)
        msg[n_p], msg[n_p + 1] = -0.75, count
        ls = torch.tensor([0.25], **F64)
        assert lib.mpcrl_ppo_log_std_apply(_p(msg), n_p, _p(ls), _stream()) == 0
        torch.cuda.synchronize()
        assert float(ls) == want
    assert lib.mpcrl_ppo_log_std_apply(None, n_p, _p(ls), _stream()) == -1


def test_surrogate_gradient_through_the_solver_vs_finite_differences(oracle_port):
    """The chain solve (du0*/dp) -> mpcrl_ppo_surrogate_grad: msg[0:3] / (-lr) against central finite differences of the summed surrogate
    over (M, m, l) through re-solves at theta (1 +- delta), delta = 1e-5 relative, tolerance 1e-4 relative (the project's
    finite-difference rule, SURVEY.md §8d, as tests/test_gpu_surface.py applies it).  64 near-upright states, drawn so that the CPU oracle
    port converges on all of them at the nominal parameters (asserted below); one roll-out row at the nominal theta with fixed eps, fixed
    advantages (no normalisation), the surrogate evaluated at theta' = 1.01 theta so that the ratios are not 1.  Instances whose re-solve
    is not status 0 at theta', theta' (1 + delta) and theta' (1 - delta) of every component are left out: at most 10 %."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, MPCBatch, _lib, cartpole_ocp
    from oracle.problems import make_cartpole
    lib = _lib.load()
    B, lr, clip, ls = 64, 1e-3, 0.2, -1.0
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, 4)) * np.array([0.3, 0.5, 0.15, 0.5])
    assert np.all(oracle_port.solve(make_cartpole(), x0, flags=0, tol=1e-10).status == 0)
    ocp = cartpole_ocp(tol=1e-10)
    n_p, lo, hi = ocp.n_p, float(ocp.lbu[0]), float(ocp.ubu[0])
    mpc = MPCBatch(ocp, B, DEV)
    x0t = torch.as_tensor(x0, **F64)
    # the roll-out row at the nominal parameters, through the roll-out kernel
    r0 = mpc.solve(x0t, cold=True)
    env = BatchedCartPoleSwingUpEnv(B, device=DEV, seed=0)
    env.state.copy_(x0t)
    tab = _Tables(1, B)
    eps = torch.as_tensor(rng.normal(size=B).astype(np.float32), device=DEV)
    log_std = torch.tensor([ls], **F64)
    obs, ended = torch.zeros(B, 4, **F64), torch.zeros(B, dtype=torch.int32, device=DEV)
    assert _collect(lib, env, 1, 0, r0.u0, r0.status, eps, torch.rand(B, **F64), torch.zeros(B, **F64), log_std, lo, hi, -1.0, tab, obs, ended) == 0
    adv = torch.as_tensor(rng.normal(0.2, 1.0, B), **F64)
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    th1 = np.array(ocp.p0, float)
    th1[:3] *= 1.01
    points = {"0": th1}
    for k in range(3):
        for sgn in (+1, -1):
            th = th1.copy()
            th[k] += sgn * 1e-5 * th1[k]
            points[f"{k}{'+' if sgn > 0 else '-'}"] = th
    res, ok = {}, tab.OK[0].bool() & (r0.status == 0)
    for name, th in points.items():
        mpc.set_theta(torch.as_tensor(th))
        res[name] = mpc.solve(x0t, sens_pi=(name == "0"), cold=True)
        ok = ok & (res[name].status == 0)
    okt = ok.to(torch.uint8).contiguous()
    ws = torch.zeros(int(lib.mpcrl_ppo_surrogate_workspace_bytes(B, n_p)), dtype=torch.uint8, device=DEV)
    zeros = torch.zeros(B, 1, n_p, **F64)

    def surrogate(r):
        msg = torch.zeros(n_p + 8, **F64)
        assert lib.mpcrl_ppo_surrogate_grad(_p(idx), B, B, _p(tab.ACT), _p(tab.LOGP), _p(adv), _p(okt), _p(r.u0), _p(r.status),
                                            _p(zeros if r.dpi_dp is None else r.dpi_dp), n_p, _p(log_std), lo, hi, clip, 0.0, lr, 0, _p(ws), _p(msg),
                                            _stream()) == 0
        return msg.cpu().numpy()

    m0 = surrogate(res["0"])
    n_in = int(okt.sum())
    assert int(m0[n_p + 1]) == n_in and n_in >= 0.9 * B
    grad = m0[:3] / (-lr)
    fd = np.array([(surrogate(res[f"{k}+"])[n_p + 2] - surrogate(res[f"{k}-"])[n_p + 2]) / (2e-5 * th1[k]) for k in range(3)])
    err = np.abs(grad - fd) / np.maximum(np.abs(fd), 1.0)
    print("surrogate gradient", grad, "finite differences", fd, "rel err", err, "instances", n_in, "clipped rows", int(m0[n_p + 4]),
          "mean ratio", m0[n_p + 5] / n_in)
    assert np.abs(m0[n_p + 5] / n_in - 1.0) > 1e-6 and np.abs(fd).min() > 0.0        # the ratios moved; the gradient is not trivially zero
    assert err.max() < 1e-4
    assert np.all(m0[3:n_p] == 0.0)                                                   # W / yref entries: du0*/dp is zero there


def test_two_learn_iterations_are_finite_and_reproducible():
    """BatchedPPO, E = 128, n_steps = 4, batch_size = 256, n_epochs = 2: two learn iterations give finite theta, log_std and statistics and
    move them; a second learner with the same seed reproduces theta and log_std bit for bit.  (The valid fraction is printed.)"""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedPPO, cartpole_ocp
    outs = []
    for _ in range(2):
        env = BatchedCartPoleSwingUpEnv(128, device=DEV, seed=3)
        ppo = BatchedPPO(cartpole_ocp(), env, n_steps=4, batch_size=256, n_epochs=2, lr=1e-4, ent_coef=0.01, log_std_init=-1.0, seed=11)
        th0 = ppo.theta.clone()
        ppo.learn(2)
        st = ppo.last_stats()
        torch.cuda.synchronize()
        outs.append((ppo.theta.clone(), ppo.log_std.clone(), st))
        assert torch.isfinite(ppo.theta).all() and torch.isfinite(ppo.log_std).all() and all(math.isfinite(v) for v in st.values())
        assert torch.isfinite(ppo.ADV).all() and torch.isfinite(ppo.RET).all()
        assert float((ppo.theta - th0)[:3].abs().max()) > 0.0 and torch.equal(ppo.theta[3:], th0[3:]) and float(ppo.log_std) != -1.0
        assert torch.equal(ppo.rollout_mpc.get_theta(), ppo.theta) and torch.equal(ppo.sample_mpc.get_theta(), ppo.theta)
        assert int(ppo._ws.count_nonzero()) == 0 and ppo.iterations == 2
    print("PPO statistics after two iterations:", outs[0][2])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2]
