"""CPU checks of batched PPO with the MPC as Gaussian actor (mpc4rl_amd/ppo.py): the C ABI's new symbols, the torch statements of the
GAE and surrogate kernels against stable_baselines3's formulas written as a per-environment loop and against torch autograd, the exact
ratio of an unchanged policy, and the constructor's argument checks."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcrl_ppo_cartpole_collect", "mpcrl_ppo_gae", "mpcrl_ppo_surrogate_workspace_bytes", "mpcrl_ppo_surrogate_grad", "mpcrl_ppo_log_std_apply"]


def test_new_symbols_in_header_and_binding_abi_still_132():
    """The five PPO symbols are declared and bound; they are additions, so header and binding still say 132."""
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.EXPORTS, name
    assert int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 132


def _sb3_loop(rew, val, vnext, term, done, gamma, lam):
    """stable_baselines3's RolloutBuffer.compute_returns_and_advantage per environment; the time-limit bootstrap as SB3's
    OnPolicyAlgorithm.collect_rollouts does it: gamma V(terminal_obs) added to the reward of a row that is truncated and not terminated."""
    T, E = rew.shape
    adv = np.zeros((T, E))
    for e in range(E):
        last = 0.0
        for t in reversed(range(T)):
            r = rew[t, e]
            if done[t, e] and not term[t, e]:
                r = r + gamma * vnext[t, e]
            nnt = 0.0 if done[t, e] else 1.0                  # episode_starts[t + 1]
            delta = r + gamma * vnext[t, e] * nnt - val[t, e]
            last = delta + gamma * lam * nnt * last
            adv[t, e] = last
    return adv, adv + val


@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("case", ["none", "all_terminated", "truncated_last", "terminated_and_truncated", "mixed"])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_gae_matches_sb3_loop(T, case, lam):
    from mpc4rl_amd import ppo_gae
    E, gamma = 7, 0.99
    rng = np.random.default_rng(100 * T + len(case))
    rew, val, vnext = rng.normal(-2, 1, (T, E)), rng.normal(-20, 5, (T, E)), rng.normal(-20, 5, (T, E))
    term, trunc = np.zeros((T, E), bool), np.zeros((T, E), bool)
    if case == "all_terminated":
        term[:] = True
    elif case == "truncated_last":
        trunc[T - 1] = True
    elif case == "terminated_and_truncated":
        term[T // 2], trunc[T // 2] = True, True
    elif case == "mixed":
        term, trunc = rng.uniform(size=(T, E)) < 0.3, rng.uniform(size=(T, E)) < 0.3
    done = term | trunc
    adv, ret = ppo_gae(*[torch.as_tensor(a) for a in (rew, val, vnext)], torch.as_tensor(term.astype(np.uint8)), torch.as_tensor(done.astype(np.uint8)),
                       gamma, lam)
    adv_ref, ret_ref = _sb3_loop(rew, val, vnext, term, done, gamma, lam)
    np.testing.assert_allclose(adv.numpy(), adv_ref, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(ret.numpy(), ret_ref, rtol=1e-12, atol=0.0)
    if lam == 0.0:                                             # one-step TD errors
        np.testing.assert_allclose(adv.numpy(), rew + gamma * vnext * ~term - val, rtol=1e-12, atol=0.0)


def _surrogate_case(seed, n_p=5):
    """A minibatch whose rows cover A > 0 / A < 0 times r below, inside and above the clip band, plus rows that must never reach a sum."""
    from mpc4rl_amd import ppo_collect_terms
    rng = np.random.default_rng(seed)
    n_rows, M, lo, hi, ls = 96, 64, -30.0, 30.0, -0.5
    u0 = rng.uniform(-20, 20, n_rows)
    status = np.zeros(n_rows, np.int32)
    status[:6] = [2, 4, 1, 0, 0, 0]
    u0[3] = np.nan
    eps = rng.normal(size=n_rows).astype(np.float32)
    _, act, logp, ok = ppo_collect_terms(torch.as_tensor(u0), torch.as_tensor(status), torch.as_tensor(eps), ls, lo, hi)
    adv = torch.as_tensor(rng.normal(0.3, 1.0, n_rows))
    idx = torch.as_tensor(np.concatenate([np.arange(8), 8 + rng.permutation(n_rows - 8)[: M - 8]]))
    # the re-solve: the mean moves by up to 0.8 sigma either way, so that the ratio leaves the band on both sides
    u0_new = np.nan_to_num(u0)[idx.numpy()] + rng.uniform(-1, 1, M) * 0.8 * math.exp(ls) * 0.5 * (hi - lo)
    status_new = np.zeros(M, np.int32)
    status_new[8:12] = [4, 1, 2, 0]
    u0_new[11] = np.nan
    dpi = rng.normal(size=(M, 1, n_p))
    dpi[8], dpi[11], dpi[1] = np.nan, np.nan, np.inf          # rows left out: their sensitivities may be anything
    dpi[20, 0, 2] = np.nan                                     # a NaN entry of a row that is left in: read as nan_to_num does
    return dict(idx=idx, act=act, logp=logp, adv=adv, ok=ok.to(torch.uint8), u0_new=torch.as_tensor(u0_new), status_new=torch.as_tensor(status_new),
                dpi_dp=torch.as_tensor(dpi), log_std=ls, lo=lo, hi=hi)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_surrogate_terms_match_autograd(normalize, ent_coef):
    from mpc4rl_amd import ppo_surrogate_terms
    c = _surrogate_case(11)
    clip, lr, n_p = 0.2, 3e-3, c["dpi_dp"].shape[-1]
    msg = ppo_surrogate_terms(**c, clip_range=clip, ent_coef=ent_coef, lr=lr, normalize_adv=normalize)
    assert msg.shape == (n_p + 8,) and torch.isfinite(msg).all()
    # the rows that may enter: by the rule, spelled out
    j = c["idx"]
    st, un = c["status_new"], c["u0_new"]
    valid = c["ok"][j].bool() & ((st == 0) | (st == 2)) & torch.isfinite(un)
    expect_out = {1, 2, 3, 8, 9, 11}                           # OK = 0 (status 4, 1, NaN u0 in the roll-out), status_new 4 / 1, NaN u0_new
    assert set(torch.nonzero(~valid).reshape(-1).tolist()) == expect_out
    assert int(msg[n_p + 1]) == int(valid.sum()) == c["idx"].numel() - len(expect_out)
    # autograd through the surrogate of the valid rows
    a, lp_old, ad = c["act"][j][valid], c["logp"][j][valid], c["adv"][j][valid]
    A = (ad - ad.mean()) / (ad.std() + 1e-8) if normalize else ad
    u = un[valid].clone().requires_grad_(True)
    ls = torch.tensor(c["log_std"], dtype=torch.float64, requires_grad=True)
    mu = 2.0 * ((u - c["lo"]) / (c["hi"] - c["lo"])) - 1.0
    lp = -((a - mu) ** 2) / (2.0 * torch.exp(ls) ** 2) - ls - 0.5 * math.log(2.0 * math.pi)
    r = torch.exp(lp - lp_old)
    loss = -torch.minimum(r * A, torch.clamp(r, 1.0 - clip, 1.0 + clip) * A)
    entropy = ls + 0.5 + 0.5 * math.log(2.0 * math.pi)
    (loss.sum() - ent_coef * int(valid.sum()) * entropy).backward()
    # the test's own inputs hold all six combinations of the advantage's sign and the ratio's region
    rd, below, above = r.detach(), r.detach() < 1.0 - clip, r.detach() > 1.0 + clip
    for sign in (A > 0, A < 0):
        for region in (below, above, ~below & ~above):
            assert int((sign & region).sum()) >= 2
    G = torch.nan_to_num(c["dpi_dp"].reshape(-1, n_p)[valid])
    ref = torch.cat([-lr * (u.grad[:, None] * G).sum(0), (-lr * ls.grad).reshape(1)])
    np.testing.assert_allclose(msg[: n_p + 1].numpy(), ref.numpy(), rtol=1e-12, atol=0.0)
    # the statistics
    assert math.isclose(float(msg[n_p + 2]), float(loss.detach().sum()), rel_tol=1e-12)
    assert math.isclose(float(msg[n_p + 3]), float(((rd - 1.0) - torch.log(rd)).sum()), rel_tol=1e-12)
    assert int(msg[n_p + 4]) == int((below | above).sum())
    assert math.isclose(float(msg[n_p + 5]), float(rd.sum()), rel_tol=1e-12)
    assert math.isclose(float(msg[n_p + 6]), float(ad.sum()), rel_tol=1e-12)
    assert math.isclose(float(msg[n_p + 7]), float(ad.var() * (ad.numel() - 1)), rel_tol=1e-12)


def test_unchanged_policy_has_ratio_one_exactly():
    """With u0_new the roll-out's u0 and LOGP from ppo_collect_terms: r = 1, approximate KL = 0 and clip count = 0 exactly."""
    from mpc4rl_amd import ppo_collect_terms, ppo_surrogate_terms
    rng = np.random.default_rng(5)
    E, n_p, lo, hi, ls = 50, 4, -30.0, 30.0, 0.3
    u0, status = torch.as_tensor(rng.uniform(-35, 35, E)), torch.as_tensor((rng.uniform(size=E) < 0.2).astype(np.int32) * 2)
    eps = torch.as_tensor(rng.normal(size=E).astype(np.float32))
    _, act, logp, ok = ppo_collect_terms(u0, status, eps, ls, lo, hi)
    assert bool(ok.all())
    msg = ppo_surrogate_terms(torch.arange(E), act, logp, torch.as_tensor(rng.normal(size=E)), ok.to(torch.uint8), u0, status,
                              torch.as_tensor(rng.normal(size=(E, 1, n_p))), ls, lo, hi, clip_range=0.2, ent_coef=0.0, lr=1e-3, normalize_adv=True)
    assert float(msg[n_p + 1]) == E and float(msg[n_p + 5]) == float(E)           # count, sum of r
    assert float(msg[n_p + 3]) == 0.0 and float(msg[n_p + 4]) == 0.0               # approximate KL, clipped rows
    assert float(msg[:n_p].abs().max()) > 0.0


def test_single_valid_row_is_not_normalised():
    """One valid row has no standard deviation: its advantage is used as it is (SB3 normalises only minibatches of more than one row)."""
    from mpc4rl_amd import ppo_surrogate_terms
    c = _surrogate_case(11)
    ok = torch.zeros_like(c["ok"])
    ok[int(c["idx"][20])] = 1
    a = {**c, "ok": ok}
    m1 = ppo_surrogate_terms(**a, clip_range=0.2, ent_coef=0.0, lr=1e-3, normalize_adv=True)
    m0 = ppo_surrogate_terms(**a, clip_range=0.2, ent_coef=0.0, lr=1e-3, normalize_adv=False)
    assert int(m1[-7]) == 1 and torch.equal(m1, m0) and torch.isfinite(m1).all()


def test_constructor_argument_checks():
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedLinearSystemEnv, BatchedPPO, cartpole_ocp, linear_system_ocp
    ocp, env = cartpole_ocp(), BatchedCartPoleSwingUpEnv(4, device="cpu")
    with pytest.raises(ValueError, match="multiple of batch_size"):
        BatchedPPO(ocp, env, n_steps=3, batch_size=5)                 # 12 samples, minibatches of 5
    for kw in (dict(n_steps=0), dict(n_steps=-2), dict(n_steps=2.0), dict(n_steps=True), dict(batch_size=0), dict(n_epochs=0), dict(gamma=0.0),
               dict(gamma=1.5), dict(gae_lambda=-0.1), dict(gae_lambda=1.1), dict(clip_range=0.0), dict(clip_range=float("nan")),
               dict(lr=float("inf")), dict(reward_scale=0.0)):
        with pytest.raises(ValueError):
            BatchedPPO(ocp, env, **{"n_steps": 3, "batch_size": 4, **kw})
    with pytest.raises(ValueError):
        BatchedPPO(linear_system_ocp(), env, n_steps=3, batch_size=4)
    with pytest.raises(TypeError):
        BatchedPPO(ocp, BatchedLinearSystemEnv(4, device="cpu"), n_steps=3, batch_size=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # valid arguments, CPU environment: refused, never emulated
        BatchedPPO(ocp, env, n_steps=3, batch_size=4)
