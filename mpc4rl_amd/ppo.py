"""Batched PPO with the MPC as Gaussian actor: the learner the reference declares and never finishes.

``rlmpc/ppo/policies.py:26-134`` defines ``MPCActorCriticPolicy(ActorCriticPolicy)`` whose ``forward``, ``evaluate_actions`` and
``predict_values`` raise NotImplementedError; only ``_predict`` works, one observation at a time through ``mpc.get_action``.  What the
stub lacks is what the engine has: the policy mean and its parameter Jacobian du0*/dp for a whole batch in one call.  The policy is
    a ~ N(mu, sigma^2),   mu = scale_action(u0*(s; theta)),   sigma = exp(log_std)        (one learnable, state-independent log_std)
and PPO's clipped surrogate is differentiated through mu with dpi/dp of the re-solve.  Per roll-out step the loop is ONE batched solve
over the E environments, one critic forward, ONE launch of mpcrl_ppo_cartpole_collect (sample, log probability, environment step, row t
of the roll-out tables, resets, the next observation and cold mask) and one mpcrl_get_iterate_rows; after the roll-out one critic
forward over the next states and ONE launch of mpcrl_ppo_gae.  Per minibatch of an epoch: mpcrl_set_iterate_rows (the re-solve starts
from the iterate the roll-out's solve ended with), ONE solve with du0*/dp, mpcrl_ppo_surrogate_grad (the message [-lr sum g dpi/dp,
-lr sum g_log_std, count, statistics]), the all-reduce of that message when there are ranks, mpcrl_qlearning_apply (theta, a masked
mean) and mpcrl_ppo_log_std_apply, and the value network's MSE step.

The value function is an nx -> 64 -> 64 -> 1 tanh MLP (activation_fn = nn.Tanh, Adam with eps = 1e-5, as the reference constructor
says), float32; all PPO arithmetic outside it is fp64.  By default it is a torch module run by the framework.  With
``value_kernels=True`` (csrc/value_kernel.hpp) its parameters and gradients are views of two flat float32 buffers, ``predict_values``
is ONE launch of mpcrl_value_forward on the float64 observations (one per roll-out step, one over all T E next states), and a
minibatch's value step is mpcrl_value_mse_grad on the tables themselves with ``idx`` (two launches: the forward pass, the MSE over the
valid rows and the backward pass by hand, message [gradient / world, loss, count]), ONE all-reduce of that message when there are
ranks, one cast-copy into the flat gradient buffer and the same fused Adam step.  The default stays the framework path.
``ppo_collect_terms``, ``ppo_gae``, ``ppo_surrogate_terms`` and ``ppo_value_terms`` state the kernels in torch (CPU-capable; what the
tests hold the kernels to).  There is no CPU path for the learner: the solver has none.

The chain of masses (``chain_mass_ocp(...)`` with a ``BatchedChainMassEnv``) has three controls: the policy is the diagonal Gaussian
    a ~ N(mu, diag(sigma^2)),   mu_j = scale_action(u0*)_j,   sigma_j = exp(log_std_j)        (one log_std per control, as SB3 keeps them)
whose log probability is the sum of the three one-control terms.  Its roll-out step is mpcrl_ppo_chain_collect (csrc/ppo_chain_kernel.hpp;
the plant takes the PHYSICAL controls, unscale_action of the clipped sample), its surrogate mpcrl_ppo_surrogate_grad_nu with
du0*/dp [3][n_p] per row of the minibatch, and its message carries the two further log_std sums after the one-control layout, so
mpcrl_qlearning_apply and the all-reduce are the same calls.  ``ppo_chain_collect_terms`` and ``ppo_surrogate_terms_nu`` state the two in torch.

Differences from stable_baselines3's PPO, on purpose: the stored action is the unclipped sample and the environment sees its clip to
[-1, 1] (SB3 does the same); a row whose roll-out solve or re-solve was not accepted (status other than 0 / 2, or u0 not finite) is left
out of the surrogate — selected out, never multiplied by 0; advantages are normalised over the valid rows of the minibatch; the policy
step is plain gradient descent with ``lr`` on theta's learnable entries and log_std (the MPC's parameters are a handful of physical
quantities, the Q-learning and TD3 loops step them the same way), Adam is kept for the value network; there is no gradient clipping
and no value clipping.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from .batch import MPCBatch
from .envs import BatchedCartPoleSwingUpEnv, BatchedChainMassEnv, BatchedLinearSystemEnv, _chain_dims
from .problems import chain_param_layout
from .qlearning_chain import chain_env_step_terms
from .qlearning_linear import linear_env_par, linear_env_step_terms

_HALF_LOG_2PI = 0.9189385332046727
MSG_EXTRA = 8        # message entries after the n_p gradient entries (include/mpcrl.h, mpcrl_ppo_surrogate_grad)


# ---------------------------------------------------------------------- the kernels' arithmetic in torch float64
def _solve_ok(u0: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    return ((status == 0) | (status == 2)) & torch.isfinite(u0)


def _mean(u0: torch.Tensor, ok: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    u = torch.where(ok, u0, torch.zeros_like(u0))                  # selected: u0 of a rejected solve may be NaN
    return torch.where(ok, 2.0 * ((u - lo) / (hi - lo)) - 1.0, torch.zeros_like(u))


def _log_prob(a: torch.Tensor, mu: torch.Tensor, log_std: torch.Tensor) -> torch.Tensor:
    sigma = torch.exp(log_std)
    d = a - mu
    return -(d * d) / (2.0 * (sigma * sigma)) - log_std - _HALF_LOG_2PI


def _f64(t, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    return torch.as_tensor(t, dtype=torch.float64, device=None if like is None else like.device)


def ppo_collect_terms(u0: torch.Tensor, status: torch.Tensor, eps: torch.Tensor, log_std, lo: float, hi: float
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The policy half of one roll-out step in torch (what mpcrl_ppo_cartpole_collect computes before the environment step).  u0 [E]
    (or [E, 1]), status [E], eps [E] standard-normal draws, log_std a scalar (tensor or float).  Returns
        mu [E] = ok ? 2 (u0 - lo) / (hi - lo) - 1 : 0,   act [E] = mu + exp(log_std) eps (unclipped),   logp [E],   ok [E] bool."""
    u = _f64(u0).reshape(-1)
    ls = _f64(log_std, u).reshape(())
    ok = _solve_ok(u, status.reshape(-1))
    mu = _mean(u, ok, lo, hi)
    act = mu + torch.exp(ls) * eps.reshape(-1).to(torch.float64)
    return mu, act, _log_prob(act, mu, ls), ok


def ppo_linear_collect_terms(par, state: torch.Tensor, steps: torch.Tensor, act: torch.Tensor, u01: torch.Tensor, reward_scale: float,
                              episode_length: int, reset_state=(0.5, 0.5)):
    """The environment half of one roll-out step on the linear system in torch (what mpcrl_ppo_linear_collect computes after the sample;
    the policy half is ``ppo_collect_terms``).  par: the 12 doubles of ``qlearning_linear.linear_env_par``; state [E, 2], steps [E] int64
    (steps since the last reset), act [E] the unclipped sample, u01 [E] the environment's noise.  The environment sees clip(act, -1, 1);
    the plant never terminates, an episode is truncated after ``episode_length`` steps and restarts at ``reset_state``.  Returns
        NEXT [E, 2] (the state after the step, before any reset),  REW [E] = reward_scale * cost,  DONE [E] bool = steps + 1 >= episode_length,
        the state [E, 2] and the step count [E] after the resets."""
    applied = torch.clamp(act.to(torch.float64).reshape(-1), -1.0, 1.0)
    nxt, cost = linear_env_step_terms(par, state.to(torch.float64), applied, u01.to(torch.float64))
    n = steps.to(torch.int64) + 1
    done = n >= episode_length
    rs = torch.as_tensor(reset_state, dtype=torch.float64, device=nxt.device).reshape(1, 2)
    return nxt, reward_scale * cost, done, torch.where(done[:, None], rs.expand_as(nxt), nxt), torch.where(done, torch.zeros_like(n), n)


def _collect_terms_nu(u0: torch.Tensor, status: torch.Tensor, eps: torch.Tensor, log_std, lo, hi):
    """``ppo_collect_terms`` for nu controls: u0, eps [E, nu], log_std, lo, hi of length nu.  ok = status in {0, 2} and ALL nu entries of u0
    finite; mu, act [E, nu]; logp [E] = the sum of the one-control terms over the controls, in their order."""
    ls, lo_t, hi_t = _f64(log_std).reshape(-1), _f64(lo).reshape(-1), _f64(hi).reshape(-1)
    nu = ls.numel()
    u = _f64(u0).reshape(-1, nu)
    st = status.reshape(-1)
    ok = ((st == 0) | (st == 2)) & torch.isfinite(u).all(1)
    mu = _mean(u, ok[:, None], lo_t, hi_t)
    act = mu + torch.exp(ls) * eps.reshape(-1, nu).to(torch.float64)
    terms = _log_prob(act, mu, ls)
    logp = terms[:, 0]
    for c in range(1, nu):
        logp = logp + terms[:, c]
    return mu, act, logp, ok


def ppo_chain_collect_terms(ocp_or_dims, p: torch.Tensor, x_ss: torch.Tensor, state: torch.Tensor, steps: torch.Tensor, u0: torch.Tensor,
                            status: torch.Tensor, eps: torch.Tensor, wn: Optional[torch.Tensor], w_std: float, log_std, lo, hi,
                            reward_scale: float, episode_length: int, x_reset: torch.Tensor, vel_std: float, rn: Optional[torch.Tensor]) -> dict:
    """One roll-out step of PPO on the chain of masses in torch float64 (what mpcrl_ppo_chain_collect computes).  ocp_or_dims, p, x_ss,
    wn [E, 3 M], w_std: the plant, as ``chain_env_step_terms`` takes them; state [E, nx]; steps [E] int64 (steps since the last reset);
    u0 [E, 3], status [E]: the solve; eps [E, 3] float32 standard normals; log_std, lo, hi: 3 each; x_reset [nx]; rn [E, 3 M] standard
    normals (None: vel_std is 0).
        ok = status in {0, 2} and all three u0 finite;   mu_j = ok ? 2 (u0_j - lo_j) / (hi_j - lo_j) - 1 : 0;   act_j = mu_j + exp(log_std_j) eps_j;
        logp = sum_j log N(act_j; mu_j, sigma_j^2);      applied_j = lo_j + 0.5 (clip(act_j, -1, 1) + 1) (hi_j - lo_j)        (unscale_action)
        next, cost = chain_env_step_terms(state, applied);   rew = reward_scale * cost;   done = steps + 1 >= episode_length;
        a done environment restarts at x_reset, + vel_std * rn on the 3 M velocity entries, with steps = 0.
    Returns a dict: mu, act [E, 3], logp [E], ok [E] bool, applied [E, 3], next [E, nx] (before any reset), rew [E], done [E] bool,
    state [E, nx] and steps [E] after the resets."""
    mu, act, logp, ok = _collect_terms_nu(u0, status, eps, log_std, lo, hi)
    lo_t, hi_t = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
    applied = lo_t + (0.5 * (torch.clamp(act, -1.0, 1.0) + 1.0)) * (hi_t - lo_t)
    x = state.to(torch.float64)
    nxt, cost = chain_env_step_terms(ocp_or_dims, p, x_ss, x, applied, wn, w_std)
    n = steps.to(torch.int64) + 1
    done = n >= episode_length
    fresh = _f64(x_reset).reshape(1, -1).repeat(nxt.shape[0], 1)
    if rn is not None and vel_std != 0.0:
        na = rn.shape[-1]
        fresh[:, fresh.shape[1] - na:] += vel_std * rn.to(torch.float64).reshape(-1, na)
    return dict(mu=mu, act=act, logp=logp, ok=ok, applied=applied, next=nxt, rew=reward_scale * cost, done=done,
                state=torch.where(done[:, None], fresh, nxt), steps=torch.where(done, torch.zeros_like(n), n))


def ppo_gae(rew: torch.Tensor, val: torch.Tensor, vnext: torch.Tensor, term: torch.Tensor, done: torch.Tensor, gamma: float,
            gae_lambda: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Generalised advantage estimates in torch (what mpcrl_ppo_gae computes); all [T, E]:
        delta_t = rew_t + gamma (1 - term_t) vnext_t - val_t;  adv_t = delta_t + gamma lambda (1 - done_t) adv_{t+1}, adv_T = 0;  ret = adv + val
    Returns adv, ret."""
    T = rew.shape[0]
    nt, nd = 1.0 - term.to(torch.float64), 1.0 - done.to(torch.float64)
    adv = torch.zeros_like(rew)
    run = torch.zeros_like(rew[0])
    gl = gamma * gae_lambda
    for t in range(T - 1, -1, -1):
        delta = (rew[t] + (gamma * nt[t]) * vnext[t]) - val[t]
        run = delta + (gl * nd[t]) * run
        adv[t] = run
    return adv, adv + val


def ppo_surrogate_terms(idx: torch.Tensor, act: torch.Tensor, logp: torch.Tensor, adv: torch.Tensor, ok: torch.Tensor,
                        u0_new: torch.Tensor, status_new: torch.Tensor, dpi_dp: torch.Tensor, log_std, lo: float, hi: float,
                        clip_range: float, ent_coef: float, lr: float, normalize_adv: bool) -> torch.Tensor:
    """The policy half of one minibatch update in torch (what mpcrl_ppo_surrogate_grad computes).  idx [M] rows of the flattened tables
    act, logp, adv, ok; u0_new [M] (or [M, 1]), status_new [M], dpi_dp [M, 1, n_p] of the re-solve.  Returns msg [n_p + 8]:
        [-lr sum g_mu 2/(hi-lo) dpi/dp (n_p), -lr (sum g_ls - ent_coef count), count, sum loss, sum (r - 1) - log r, rows with |r - 1| > eps,
         sum r, sum ADV, sum (ADV - mean)^2]     over the valid rows (include/mpcrl.h)."""
    act, logp, adv, okf = act.reshape(-1), logp.reshape(-1), adv.reshape(-1), ok.reshape(-1)
    n_rows, M = act.numel(), idx.numel()
    zero = torch.zeros(M, dtype=torch.float64, device=act.device)
    inr = (idx >= 0) & (idx < n_rows)
    j = idx.clamp(0, n_rows - 1)
    a, lp_old, ad = act[j], logp[j], adv[j]
    u = _f64(u0_new).reshape(-1)
    ls = _f64(log_std, act).reshape(())
    valid = inr & (okf[j] != 0) & _solve_ok(u, status_new.reshape(-1)) & torch.isfinite(a) & torch.isfinite(lp_old) & torch.isfinite(ad)
    sel = lambda t: torch.where(valid, t, zero)                       # noqa: E731  (selected out, never multiplied by 0)
    a, lp_old, ad = sel(a), sel(lp_old), sel(ad)
    n = valid.sum().to(torch.float64)
    s1 = ad.sum()
    mean = s1 / torch.clamp(n, min=1.0)
    s2 = sel((ad - mean) ** 2).sum()
    A = ad
    if normalize_adv:
        std = torch.sqrt(s2 / torch.clamp(n - 1.0, min=1.0))
        A = torch.where(n > 1.0, (ad - mean) / (std + 1e-8), ad)
    mu = _mean(u, valid, lo, hi)
    logr = _log_prob(a, mu, ls) - lp_old
    r = torch.exp(logr)
    l1, l2 = r * A, torch.clamp(r, 1.0 - clip_range, 1.0 + clip_range) * A
    flat = ((A > 0.0) & (r > 1.0 + clip_range)) | ((A < 0.0) & (r < 1.0 - clip_range))     # the clipped branch is the minimum
    var = torch.exp(ls) ** 2
    d = a - mu
    live = valid & ~flat
    g_mu = torch.where(live, -(A * r) * (d / var), zero)
    g_ls = torch.where(live, -(A * r) * (d * d / var - 1.0), zero)
    G = torch.nan_to_num(dpi_dp.reshape(M, -1))
    G = torch.where(valid[:, None], G, torch.zeros_like(G))
    grad = ((g_mu * (2.0 / (hi - lo)))[:, None] * G).sum(0)
    tail = torch.stack([-lr * (g_ls.sum() - ent_coef * n), n, sel(-torch.minimum(l1, l2)).sum(), sel((r - 1.0) - logr).sum(),
                        sel(((r - 1.0).abs() > clip_range).to(torch.float64)).sum(), sel(r).sum(), s1, s2])
    return torch.cat([-lr * grad, tail])


def ppo_surrogate_terms_nu(idx: torch.Tensor, act: torch.Tensor, logp: torch.Tensor, adv: torch.Tensor, ok: torch.Tensor,
                           u0_new: torch.Tensor, status_new: torch.Tensor, dpi_dp: torch.Tensor, log_std, lo, hi,
                           clip_range: float, ent_coef: float, lr: float, normalize_adv: bool) -> torch.Tensor:
    """``ppo_surrogate_terms`` for a diagonal Gaussian over nu = dpi_dp.shape[-2] controls (what mpcrl_ppo_surrogate_grad_nu computes):
    act [..., nu] (nu = 1: [...] too), u0_new [M, nu], dpi_dp [M, nu, n_p], log_std, lo, hi of length nu (nu = 1: scalars too).  A row is
    valid when all nu entries of u0_new and of act are finite (and the rest as there); logp is the sum of the one-control terms in the
    controls' order.  Returns msg [n_p + 8 + (nu - 1)]: entries [0, n_p + 8) in the layout of ``ppo_surrogate_terms`` with
        [0, n_p) = -lr sum_b sum_c g_mu,bc 2/(hi_c - lo_c) dpi_dp[b, c],      [n_p] = -lr (sum g_ls,0 - ent_coef count),
    then [n_p + 8 + c - 1] = -lr (sum g_ls,c - ent_coef count) for c = 1 .. nu-1.  With nu = 1 it is ``ppo_surrogate_terms`` bit for bit."""
    nu, n_p = int(dpi_dp.shape[-2]), int(dpi_dp.shape[-1])
    logp, adv, okf = logp.reshape(-1), adv.reshape(-1), ok.reshape(-1)
    n_rows, M = logp.numel(), idx.numel()
    act = act.reshape(n_rows, nu)
    zero = torch.zeros(M, dtype=torch.float64, device=act.device)
    inr = (idx >= 0) & (idx < n_rows)
    j = idx.clamp(0, n_rows - 1)
    a, lp_old, ad = act[j], logp[j], adv[j]
    u = _f64(u0_new).reshape(M, nu)
    ls, lo_v, hi_v = (_f64(v, act).reshape(-1) for v in (log_std, lo, hi))
    st = status_new.reshape(-1)
    valid = (inr & (okf[j] != 0) & ((st == 0) | (st == 2)) & torch.isfinite(u).all(1) & torch.isfinite(a).all(1) & torch.isfinite(lp_old)
             & torch.isfinite(ad))
    sel = lambda t: torch.where(valid, t, zero)                       # noqa: E731  (selected out, never multiplied by 0)
    lp_old, ad = sel(lp_old), sel(ad)
    n = valid.sum().to(torch.float64)
    s1 = ad.sum()
    mean = s1 / torch.clamp(n, min=1.0)
    s2 = sel((ad - mean) ** 2).sum()
    A = ad
    if normalize_adv:
        std = torch.sqrt(s2 / torch.clamp(n - 1.0, min=1.0))
        A = torch.where(n > 1.0, (ad - mean) / (std + 1e-8), ad)
    d, var, lp = [], [], None
    for c in range(nu):
        ac = sel(a[:, c])
        mu = _mean(u[:, c], valid, float(lo_v[c]), float(hi_v[c]))
        term = _log_prob(ac, mu, ls[c])
        lp = term if c == 0 else lp + term
        d.append(ac - mu)
        var.append(torch.exp(ls[c]) ** 2)
    logr = lp - lp_old
    r = torch.exp(logr)
    l1, l2 = r * A, torch.clamp(r, 1.0 - clip_range, 1.0 + clip_range) * A
    flat = ((A > 0.0) & (r > 1.0 + clip_range)) | ((A < 0.0) & (r < 1.0 - clip_range))     # the clipped branch is the minimum
    live = valid & ~flat
    g_mu = [torch.where(live, -(A * r) * (d[c] / var[c]), zero) for c in range(nu)]
    g_ls = [torch.where(live, -(A * r) * (d[c] * d[c] / var[c] - 1.0), zero) for c in range(nu)]
    G = torch.nan_to_num(dpi_dp.reshape(M, nu, n_p))
    G = torch.where(valid[:, None, None], G, torch.zeros_like(G))
    w = torch.stack([g_mu[c] * (2.0 / (float(hi_v[c]) - float(lo_v[c]))) for c in range(nu)], 1)      # [M, nu]
    grad = (w.reshape(M * nu)[:, None] * G.reshape(M * nu, n_p)).sum(0)
    tail = torch.stack([-lr * (g_ls[0].sum() - ent_coef * n), n, sel(-torch.minimum(l1, l2)).sum(), sel((r - 1.0) - logr).sum(),
                        sel(((r - 1.0).abs() > clip_range).to(torch.float64)).sum(), sel(r).sum(), s1, s2]
                       + [-lr * (g_ls[c].sum() - ent_coef * n) for c in range(1, nu)])
    return torch.cat([-lr * grad, tail])


def ppo_value_terms(OBS: torch.Tensor, RET: torch.Tensor, idx: torch.Tensor, value_net: nn.Module, vf_coef: float
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The value half of one minibatch update in torch (what mpcrl_value_mse_grad computes).  OBS [..., nx] and RET [...] are the
    roll-out tables (flattened here), idx [M] rows of them, ``value_net`` the MLP in any dtype (float64: the yardstick of the tests).
        valid_b = 0 <= idx[b] < n_rows and OBS[idx[b]], RET[idx[b]] finite          (selected out, never multiplied by 0)
        e_b     = valid_b ? V(OBS[idx[b]]) - RET[idx[b]] : 0,      loss = vf_coef sum e_b^2 / max(1, count)
    with OBS and RET rounded to float32 first, as the kernel loads them.  Returns loss (0-dim), count (0-dim int64) and d loss / d
    parameters through autograd, flat in ``value_net.parameters()`` order."""
    params = list(value_net.parameters())
    dt = params[0].dtype
    nx = OBS.shape[-1]
    obs, ret = OBS.reshape(-1, nx), RET.reshape(-1)
    n_rows, M = ret.numel(), idx.numel()
    inr = (idx >= 0) & (idx < n_rows)
    if n_rows > 0:
        j = idx.clamp(0, n_rows - 1)
        o, r = obs[j], ret[j]
    else:
        o, r = obs.new_zeros(M, nx), ret.new_zeros(M)
    valid = inr & torch.isfinite(o).all(dim=1) & torch.isfinite(r)
    x = torch.where(valid[:, None], o, torch.zeros_like(o)).to(torch.float32).to(dt)
    y = torch.where(valid, r, torch.zeros_like(r)).to(torch.float32).to(dt)
    v = value_net(x).reshape(M)
    e = torch.where(valid, v - y, torch.zeros_like(v))
    n = valid.sum()
    loss = vf_coef * (e * e).sum() / torch.clamp(n, min=1).to(dt)
    grads = torch.autograd.grad(loss, params)
    return loss.detach(), n, torch.cat([g.reshape(-1) for g in grads])


# ---------------------------------------------------------------------- the policy
class MPCActorCriticPolicy:
    """The surface of rlmpc/ppo/policies.py:26-134 (``MPCActorCriticPolicy(ActorCriticPolicy)``), batched and without stable-baselines3:
    ``_predict``, ``forward``, ``evaluate_actions``, ``predict_values`` with the reference's argument names.  ``mpc`` is an
    ``OcpDescription`` (the reference passes its MPC object: here the policy owns a batched handle of ``batch`` instances built from
    it); ``observation_space`` / ``action_space`` only need ``.shape``; ``lr_schedule`` is a callable of the remaining progress.
    Every method is ONE batched solve where the reference solves one observation (or raises).  Actions are the scaled ones in [-1, 1]
    (``MPC.scale_action``), float64 [B, 1]; the Gaussian's mean is the MPC's action, ``log_std`` a learnable scalar on the device
    (``log_std_init`` as in the reference signature), the value function an nx -> 64 -> 64 -> 1 ``activation_fn`` MLP with the
    reference's optimiser settings (Adam, eps = 1e-5).  ``value_kernels=True`` (net_arch (64, 64), nn.Tanh, at most 16 observations;
    ValueError otherwise): the network's parameters and gradients are views of the flat float32 buffers ``value_flat`` /
    ``value_grad_flat`` (``td3.flatten_parameters``) and ``predict_values`` is one mpcrl_value_forward launch without an autograd
    graph; the module stays usable as a torch module (nothing may rebind its ``p.data`` or ``p.grad``).

    An OCP with nu = 2 or 3 controls (the chain of masses: 3) gives a diagonal Gaussian: ``log_std`` has shape (nu,), ``lo`` / ``hi`` are
    tuples of nu floats, actions are [B, nu], ``log_prob`` is the sum over the controls and the entropy
    sum_j log_std_j + nu (1/2 + 1/2 log 2 pi).  With nu = 1 every shape and value is as described above.  The chain's observations (15 to
    33) are beyond the value kernels' 16: its value function is the torch MLP."""

    def __init__(self, observation_space, action_space, lr_schedule, mpc, batch: int = 1, device=None, activation_fn=nn.Tanh,
                 ortho_init: bool = True, log_std_init: float = 0.0, net_arch=(64, 64), optimizer_class=torch.optim.Adam,
                 optimizer_kwargs=None, generator: Optional[torch.Generator] = None, value_kernels: bool = False):
        if getattr(mpc, "nu", None) not in (1, 2, 3):
            raise ValueError("MPCActorCriticPolicy: one to three controls (1 <= nu <= 3)")
        self.nu = nu = int(mpc.nu)
        obs_dim = int(observation_space.shape[0]) if observation_space is not None else mpc.nx
        self.value_kernels = bool(value_kernels)
        if self.value_kernels and (tuple(net_arch) != (64, 64) or activation_fn is not nn.Tanh or not 1 <= obs_dim <= 16):
            raise ValueError("value_kernels=True: the library kernels are written for net_arch=(64, 64), activation_fn=nn.Tanh and "
                             f"1 <= observations <= 16 (got {tuple(net_arch)}, {getattr(activation_fn, '__name__', activation_fn)}, {obs_dim})")
        self.observation_space, self.action_space, self.ocp = observation_space, action_space, mpc
        self.mpc = MPCBatch(mpc, batch, device)
        dev = self.mpc.device
        self.device = dev
        if self.value_kernels and not (dev.type == "cuda" and torch.version.hip):
            raise RuntimeError("value_kernels=True needs a HIP device; there is no CPU fallback")
        if nu == 1:
            self.lo, self.hi = float(mpc.lbu[0]), float(mpc.ubu[0])
        else:                # per control; the tensors are what the torch expressions broadcast
            self.lo, self.hi = tuple(float(v) for v in mpc.lbu), tuple(float(v) for v in mpc.ubu)
            self._lo_t, self._hi_t = (torch.tensor(v, dtype=torch.float64, device=dev) for v in (self.lo, self.hi))
        self.theta = torch.as_tensor(mpc.p0, dtype=torch.float64, device=dev).clone()
        self.log_std = torch.full((nu,), float(log_std_init), dtype=torch.float64, device=dev)     # never rebound: kernels hold its address
        self.obs_dim = obs_dim
        layers, last = [], obs_dim
        for h in net_arch:
            layers += [nn.Linear(last, h), activation_fn()]
            last = h
        layers.append(nn.Linear(last, 1))
        self.value_net = nn.Sequential(*layers)
        if ortho_init:       # SB3's ActorCriticPolicy._build: gain sqrt(2) for the hidden layers, 1 for the value head
            lin = [m for m in self.value_net if isinstance(m, nn.Linear)]
            for k, m in enumerate(lin):
                nn.init.orthogonal_(m.weight, gain=1.0 if k == len(lin) - 1 else math.sqrt(2.0))
                nn.init.zeros_(m.bias)
        self.value_net.to(dev)
        self.value_flat = self.value_grad_flat = None
        if self.value_kernels:
            from .td3 import flatten_parameters
            self.value_flat, self.value_grad_flat = flatten_parameters(self.value_net)
        if optimizer_kwargs is None:
            optimizer_kwargs = {}
            if optimizer_class == torch.optim.Adam:
                optimizer_kwargs["eps"] = 1e-5                           # policies.py:50-54
                if dev.type == "cuda":                                   # no host synchronisation in a step
                    optimizer_kwargs.update(fused=True, capturable=True)
        self.optimizer = optimizer_class(self.value_net.parameters(), lr=float(lr_schedule(1)), **optimizer_kwargs)
        self.gen = generator
        self.training = True

    def _solve_mean(self, obs: torch.Tensor):
        r = self.mpc.solve(obs.to(torch.float64))
        if self.nu > 1:      # mu [B, nu]; a solve is accepted when all of its controls are numbers
            u = r.u0.reshape(-1, self.nu)
            ok = ((r.status == 0) | (r.status == 2)) & torch.isfinite(u).all(1)
            return _mean(u, ok[:, None], self._lo_t, self._hi_t), ok
        u = r.u0.reshape(-1)
        ok = _solve_ok(u, r.status)
        return _mean(u, ok, self.lo, self.hi), ok

    def _sample(self, mu: torch.Tensor, deterministic: bool) -> torch.Tensor:
        if deterministic:
            return mu
        eps = torch.randn(mu.shape, dtype=torch.float32, device=mu.device, generator=self.gen)
        return mu + torch.exp(self.log_std if self.nu > 1 else self.log_std[0]) * eps.to(torch.float64)

    def _log_prob(self, a: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """[B]: nu = 1 the one term; else the sum of the controls' terms in their order (a, mu [B, nu])."""
        if self.nu == 1:
            return _log_prob(a, mu, self.log_std[0])
        terms = _log_prob(a, mu, self.log_std)
        lp = terms[:, 0]
        for c in range(1, self.nu):
            lp = lp + terms[:, c]
        return lp

    def predict_values(self, obs: torch.Tensor) -> torch.Tensor:
        """[B, 1] float64: the value network at the observations (``value_kernels``: one launch, no autograd graph)."""
        if not self.value_kernels:
            return self.value_net(obs.to(torch.float32)).to(torch.float64)
        o = obs.to(device=self.device, dtype=torch.float64).reshape(-1, self.obs_dim).contiguous()
        out = torch.empty(o.shape[0], 1, dtype=torch.float64, device=self.device)
        _lib.call("mpcrl_value_forward", o, o.shape[0], self.obs_dim, self.value_flat, out, device=self.device)
        return out

    def _predict(self, observation: torch.Tensor, deterministic: bool = True) -> torch.Tensor:
        mu, _ = self._solve_mean(observation)
        a = self._sample(mu, deterministic)
        return a if self.nu > 1 else a[:, None]

    def forward(self, obs: torch.Tensor, deterministic: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """actions [B, nu] (the unclipped sample, or the mean), values [B, 1], log_prob [B]."""
        mu, _ = self._solve_mean(obs)
        a = self._sample(mu, deterministic)
        return (a if self.nu > 1 else a[:, None]), self.predict_values(obs), self._log_prob(a, mu)

    __call__ = forward

    def evaluate_actions(self, obs: torch.Tensor, actions: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """values [B, 1], log_prob [B] of ``actions`` under the current policy, entropy [B] of the Gaussian (log_std + 1/2 log 2 pi e;
        nu controls: sum_j log_std_j + nu (1/2 + 1/2 log 2 pi))."""
        mu, _ = self._solve_mean(obs)
        if self.nu > 1:
            a = actions.to(torch.float64).reshape(-1, self.nu)
            ent = (self.log_std.sum() + self.nu * (0.5 + _HALF_LOG_2PI)).expand(a.shape[0])
            return self.predict_values(obs), self._log_prob(a, mu), ent
        a = actions.to(torch.float64).reshape(-1)
        ent = (self.log_std[0] + (0.5 + _HALF_LOG_2PI)).expand(a.shape[0])
        return self.predict_values(obs), _log_prob(a, mu, self.log_std[0]), ent

    def set_training_mode(self, mode: bool) -> None:
        self.value_net.train(mode)
        self.training = mode


class _Box:
    def __init__(self, n: int):
        self.shape = (n,)


# ---------------------------------------------------------------------- the learner
class BatchedPPO:
    """PPO (clipped surrogate, GAE) of the cartpole, the linear-system or the chain-of-masses MPC's parameters over E = ``env.num_envs``
    parallel environments per rank: ``cartpole_ocp()`` with a ``BatchedCartPoleSwingUpEnv``, or ``linear_system_ocp()`` with a
    ``BatchedLinearSystemEnv`` and ``episode_length`` (that plant never terminates and its environment counts no steps: the learner
    truncates an episode after ``episode_length`` steps and restarts it at the environment's reset state; the roll-out step is
    mpcrl_ppo_linear_collect, the reward is the step's cost, all 12 parameters A, B, b, V_0, f are learned), or ``chain_mass_ocp(...)`` with
    a ``BatchedChainMassEnv`` built for the same (n_mass, Ts, rk_steps) and ``episode_length``.  The cartpole's limit is the environment's
    ``max_episode_steps``.

    The chain of masses: three controls, a diagonal Gaussian (``MPCActorCriticPolicy``); ``ACT`` is [T, E, 3], ``log_std`` (3,), every
    other table as for one control.  The roll-out step is mpcrl_ppo_chain_collect: the reward is the step's cost l(s, a) (of the state
    before the step, see ``BatchedChainMassEnv``) times ``reward_scale``, the plant's parameters are read from ``env.p`` at every step,
    a truncated chain restarts as ``env.reset()`` draws it (x0 plus ``env.vel_std`` N(0, 1) on the velocities); the disturbance draws
    ``wn`` and the reset draws ``rn`` are one [T, E, 3 M] tensor each per roll-out from ``env.gen``.  The first observation is
    ``env.reset()`` — x0 with perturbed velocities, never the zero state, where the masses coincide and the ODE divides by zero (what
    ``ChainQLearning._initial_obs`` avoids).  ``learn`` (chain only): the blocks of theta that are learned, any of ``ChainQLearning.BLOCKS``
    with its default (m, D, L, C) and its mask; ``last_stats()["log_std"]`` is the mean of the three.  The value function is the torch
    MLP (``value_kernels=True`` is refused above 16 observations).  Sizing: the stored-iterate tables are T E rows of
    (N + 1) nx + N nu + N nx + 10 (N + 1)(nx + nu) doubles — about 93 KB per row at n_mass 5, N 40, so T = 4, E = 256 is 95 MB — and the
    two handles hold E and ``batch_size`` chain instances at about 2 MB each at that size (``ChainQLearning``'s docstring);
    ``workspace_bytes()`` returns what the library reports for them.

    ``collect()`` rolls out ``n_steps`` = T steps of all environments into [T, E] tables on the device and computes advantages and
    returns; ``train()`` runs ``n_epochs`` passes over the T E samples in minibatches of ``batch_size``; ``learn(n)`` loops the two.
    Neither synchronises with the host; ``last_stats()`` reads the statistics when asked.  The reference environment's ``reward`` is the
    quadratic cost x^2 + theta^2: the default ``reward_scale = -1`` makes PPO maximise its negative (as BatchedTD3).  theta's
    learnable entries are the OCP's model block (cartpole: M, m, l); ``lr`` steps them and log_std, ``lr_value`` the value network (loss
    ``vf_coef`` x MSE against the returns).  With a process ``group`` every rank owns its environments and handles; per minibatch the
    surrogate's message and the value gradients are all-reduced, so all ranks hold the same theta, log_std and value network.
    ``value_kernels=True`` runs the value function as library kernels (the module docstring; ``MPCActorCriticPolicy``); the default is
    the framework path."""

    def __init__(self, ocp, env, n_steps: int = 32, batch_size: int = 256, n_epochs: int = 4, gamma: float = 0.99, gae_lambda: float = 0.95,
                 clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5, lr: float = 1e-4, lr_value: float = 3e-4,
                 reward_scale: float = -1.0, normalize_advantage: bool = True, seed: int = 0, device=None, group=None,
                 log_std_init: float = 0.0, value_kernels: bool = False, episode_length: Optional[int] = None,
                 learn: Optional[Sequence[str]] = None):
        model = getattr(ocp, "model", None)
        self.linear = model == _lib.MODEL_LINEAR
        self.chain = model == _lib.MODEL_CHAIN
        if learn is not None and not self.chain:
            raise ValueError("learn is for the chain of masses; the cartpole and the linear system learn their model block")
        if self.chain:
            from .qlearning_chain import ChainQLearning
            n_mass, Ts, rk_steps = _chain_dims(ocp)
            if isinstance(episode_length, bool) or not isinstance(episode_length, int) or episode_length < 1:
                raise ValueError("episode_length must be an int >= 1 with the chain of masses (its plant never ends an episode)")
            if not isinstance(env, BatchedChainMassEnv):
                raise TypeError("BatchedPPO with the chain-of-masses OCP needs a BatchedChainMassEnv")
            if (env.n_mass, env.Ts, env.rk_steps, env.nx) != (n_mass, Ts, rk_steps, ocp.nx):
                raise ValueError("the environment was built for another chain (n_mass, Ts, rk_steps)")
            learn = ("m", "D", "L", "C") if learn is None else ((learn,) if isinstance(learn, str) else tuple(learn))
            for key in learn:
                if key not in ChainQLearning.BLOCKS:
                    raise ValueError(f"learn: unknown block {key!r} (one of {', '.join(ChainQLearning.BLOCKS)})")
        elif self.linear:
            if ocp.nu != 1 or ocp.nx != 2:
                raise ValueError("BatchedPPO needs the cartpole OCP (cartpole_ocp()) or the linear-system OCP (linear_system_ocp())")
            if isinstance(episode_length, bool) or not isinstance(episode_length, int) or episode_length < 1:
                raise ValueError("episode_length must be an int >= 1 with the linear system (its environment has no step limit)")
            if not isinstance(env, BatchedLinearSystemEnv):
                raise TypeError("BatchedPPO with the linear-system OCP needs a BatchedLinearSystemEnv")
        else:
            if model != _lib.MODEL_CARTPOLE or ocp.nu != 1 or ocp.nx != 4:
                raise ValueError("BatchedPPO needs the cartpole OCP (cartpole_ocp()), the linear-system OCP (linear_system_ocp()) or the "
                                 "chain-of-masses OCP (chain_mass_ocp())")
            if not isinstance(env, BatchedCartPoleSwingUpEnv):
                raise TypeError("BatchedPPO needs a BatchedCartPoleSwingUpEnv")
            if episode_length is not None:
                raise ValueError("episode_length is for the linear system; the cartpole's limit is the environment's max_episode_steps")
        for name, v in (("n_steps", n_steps), ("batch_size", batch_size), ("n_epochs", n_epochs)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an int >= 1")
        if (n_steps * env.num_envs) % batch_size != 0:
            raise ValueError(f"n_steps * num_envs = {n_steps * env.num_envs} is not a multiple of batch_size = {batch_size}")
        if not (0.0 < gamma <= 1.0) or not (0.0 <= gae_lambda <= 1.0):
            raise ValueError("gamma must lie in (0, 1], gae_lambda in [0, 1]")
        if not (math.isfinite(clip_range) and clip_range > 0.0):
            raise ValueError("clip_range must be finite and > 0")
        for name, v in (("ent_coef", ent_coef), ("vf_coef", vf_coef), ("lr", lr), ("lr_value", lr_value), ("log_std_init", log_std_init)):
            if not math.isfinite(v):
                raise ValueError(f"{name} must be finite")
        if not (math.isfinite(reward_scale) and reward_scale != 0.0):
            raise ValueError("reward_scale must be finite and not 0")
        dev = env.device if device is None else torch.device(device)
        if dev.type != "cuda" or env.device.type != "cuda":
            raise RuntimeError("BatchedPPO runs on a HIP device (the environment's state too); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if env.device.index is not None and env.device != dev:
            raise ValueError("the environment must live on the learner's device (its state is updated in place by the library)")
        self.ocp, self.env, self.device, self.group = ocp, env, dev, group
        self.T, self.E, self.B, self.n_epochs = n_steps, env.num_envs, batch_size, n_epochs
        self.gamma, self.gae_lambda, self.clip_range, self.ent_coef, self.vf_coef = float(gamma), float(gae_lambda), float(clip_range), float(ent_coef), float(vf_coef)
        self.lr, self.reward_scale, self.normalize_advantage = float(lr), float(reward_scale), bool(normalize_advantage)
        T, E, B = self.T, self.E, self.B
        rank = torch.distributed.get_rank(group) if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        self.gen = torch.Generator(device=dev).manual_seed(seed + 1000 * rank)     # exploration / shuffling differ per rank
        torch.manual_seed(seed)                                                    # identical value network on every rank
        self.policy = MPCActorCriticPolicy(_Box(ocp.nx), _Box(ocp.nu), lambda _: lr_value, ocp, batch=E, device=dev, log_std_init=log_std_init,
                                           generator=self.gen, value_kernels=value_kernels)
        self.value_kernels = self.policy.value_kernels
        self.rollout_mpc = self.policy.mpc                        # keeps one warm-start iterate per environment
        self.sample_mpc = MPCBatch(ocp, B, dev)                   # the minibatch re-solves: mu and dpi/dp
        self.theta, self.log_std = self.policy.theta, self.policy.log_std          # updated in place
        self.n_p = ocp.n_p
        self.learn_mask = torch.zeros_like(self.theta)
        nu = self.nu = ocp.nu
        if self.chain:                                            # the blocks ``learn`` names (ChainQLearning's mask)
            self.n_mass, self.Ts, self.rk_steps, self.M, self.learn_blocks = n_mass, Ts, rk_steps, n_mass - 2, learn
            off = chain_param_layout(n_mass)[4]
            for key in learn:
                self.learn_mask[off[key][0]: off[key][1]] = 1.0
        else:
            self.learn_mask[: ocp.n_model_p] = 1.0                # cartpole: (M, m, l); linear system: all of A, B, b, V_0, f
        self.lo, self.hi = self.policy.lo, self.policy.hi
        f64 = dict(dtype=torch.float64, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        # the roll-out tables, [T, E]; every buffer keeps its address
        nx = self.nx = ocp.nx
        self.OBS, self.NEXT = torch.zeros(T, E, nx, **f64), torch.zeros(T, E, nx, **f64)
        self.LOGP, self.VAL, self.REW = (torch.zeros(T, E, **f64) for _ in range(3))
        self.ACT = torch.zeros(T, E, nu, **f64) if nu > 1 else torch.zeros(T, E, **f64)
        self.ADV, self.RET, self.VNEXT = (torch.zeros(T, E, **f64) for _ in range(3))
        self.TERM, self.DONE, self.OK = (torch.zeros(T, E, **u8) for _ in range(3))
        # the iterates the roll-out's solves ended with, row t E + e (what the minibatch re-solves start from)
        N, nw = ocp.N, ocp.nx + ocp.nu
        self.iters = tuple(torch.zeros(T * E, n, **f64) for n in ((N + 1) * ocp.nx, N * ocp.nu, N * ocp.nx, 10 * (N + 1) * nw))
        self._rows = torch.arange(T * E, dtype=torch.int64, device=dev).reshape(T, E)
        self.obs = env.reset().to(dev).to(torch.float64).contiguous()
        if self.chain:
            self.episode_length = episode_length
            self.steps = torch.zeros(E, dtype=torch.int64, device=dev)      # steps since the last reset (the environment keeps no count)
            self.lo_v, self.hi_v = (C.c_double * nu)(*self.lo), (C.c_double * nu)(*self.hi)
            self.x_reset = torch.as_tensor(ocp.x0, **f64).clone().contiguous()           # what BatchedChainMassEnv.reset starts from
            self.wn, self.rn = (torch.zeros(T, E, 3 * self.M, **f64) for _ in range(2))  # drawn per roll-out (collect)
        if self.linear:
            self.episode_length = episode_length
            self.steps = torch.zeros(E, dtype=torch.int64, device=dev)      # steps since the last reset (the environment keeps no count)
            self._par_c = (C.c_double * 12)(*linear_env_par(env))           # the environment's parameters, read here
            self._reset_c = (C.c_double * 2)(*env.state[0].tolist())        # what BatchedLinearSystemEnv.reset writes
        self.ended = torch.ones(E, dtype=torch.int32, device=dev)             # the first solve starts every instance cold
        self.msg = torch.zeros(self.n_p + MSG_EXTRA + nu - 1, **f64)    # (the log_std sums of the controls after the first follow)
        self.step_out = torch.zeros(self.n_p, **f64)
        self._stat = torch.zeros(MSG_EXTRA - 1, **f64)              # since the last train(): count, loss, kl, clipped, r, ADV sums
        self._stat_rows = 0
        self._ws = (_lib.workspace("mpcrl_ppo_surrogate_workspace_bytes_nu", B, self.n_p, nu, device=dev) if nu > 1 else
                    _lib.workspace("mpcrl_ppo_surrogate_workspace_bytes", B, self.n_p, device=dev))
        self._vloss = torch.zeros((), dtype=torch.float32, device=dev)      # vf_coef x MSE of the last minibatch (summed over the ranks)
        if self.value_kernels:
            self.n_value = self.policy.value_flat.numel()
            # written in full by every call: no initialisation (so not _lib.workspace, which zeroes)
            self._vws = torch.empty(_lib.call("mpcrl_value_workspace_bytes", B, ocp.nx), dtype=torch.uint8, device=dev)
            self.vmsg = torch.zeros(self.n_value + 2, **f64)               # [gradient / world, loss, count]
            self._vloss = self.vmsg[self.n_value]
        # the roll-out handle holds an iterate from here on, so that its first solve is the per-instance cold start of the cold mask
        self.rollout_mpc.solve(self.obs, cold=True)
        self.iterations = 0

    # ------------------------------------------------------------------ pieces
    def _call(self, name: str, *args) -> int:
        return _lib.call(name, *args, device=self.device)

    def _collect_step(self, t: int) -> None:
        env, dev = self.env, self.device
        r = self.rollout_mpc.solve(self.obs, cold_mask=self.ended)            # the policy mean of every environment, one launch
        with torch.no_grad():
            value = self.policy.predict_values(self.obs).reshape(self.E).contiguous()
        if self.chain:
            return self._collect_step_chain(t, r, value)
        eps = torch.randn(self.E, dtype=torch.float32, device=dev, generator=self.gen)
        u01 = torch.rand(self.E, generator=env.gen, dtype=torch.float64, device=dev)
        tables = (self.OBS, self.ACT, self.LOGP, self.VAL, self.REW, self.NEXT, self.TERM, self.DONE, self.OK, self.obs, self.ended)
        if self.linear:      # u01: the environment's noise of this step; truncation at episode_length, restart at the reset state
            self._call("mpcrl_ppo_linear_collect", self._par_c, self.E, self.T, t, env.state, self.steps, r.u0, r.status, eps, u01, value,
                       self.log_std, self.lo, self.hi, self.reward_scale, self.episode_length, self._reset_c, *tables)
        else:
            self._call("mpcrl_ppo_cartpole_collect", env._par(), self.E, self.T, t, env.state, env.steps, r.u0, r.status, eps, u01, value,
                       self.log_std, self.lo, self.hi, self.reward_scale, *tables)
        self.last_collect = (r, eps, u01, value)                              # the step's solve and draws (what the tests re-state it from)
        self.rollout_mpc.get_iterate_rows(*self.iters, index=self._rows[t])

    def _collect_step_chain(self, t: int, r, value: torch.Tensor) -> None:
        env, dev = self.env, self.device
        if not (env.p.is_contiguous() and env.p.dtype == torch.float64 and env.p.device.type == "cuda"):
            raise ValueError("env.p must stay a contiguous float64 tensor on the environment's device")
        eps = torch.randn(self.E, self.nu, dtype=torch.float32, device=dev, generator=self.gen)
        wn, rn = self.wn[t], self.rn[t]                                       # this step's rows of the roll-out's draws
        self._call("mpcrl_ppo_chain_collect", self.n_mass, self.Ts, self.rk_steps, env.p, 0 if env.p.dim() == 1 else self.n_p, env.x_ss,
                   env.w_std, self.E, self.T, t, env.state, self.steps, r.u0, r.status, eps, wn, value, self.log_std, self.lo_v, self.hi_v,
                   self.reward_scale, self.episode_length, self.x_reset, env.vel_std, rn, self.OBS, self.ACT, self.LOGP, self.VAL, self.REW,
                   self.NEXT, self.TERM, self.DONE, self.OK, self.obs, self.ended)
        self.last_collect = (r, eps, wn, value, rn)                           # the step's solve and draws (what the tests re-state it from)
        self.rollout_mpc.get_iterate_rows(*self.iters, index=self._rows[t])

    def workspace_bytes(self) -> Tuple[int, int]:
        """Bytes of device memory of the roll-out handle (E instances) and of the minibatch handle (batch_size instances)."""
        return self.rollout_mpc.workspace_bytes(), self.sample_mpc.workspace_bytes()

    def collect(self) -> None:
        """One roll-out: T steps of all E environments into the tables, then advantages and returns."""
        if self.chain:
            for buf in (self.wn, self.rn):
                torch.randn(*buf.shape, generator=self.env.gen, dtype=torch.float64, device=self.device, out=buf)
        for t in range(self.T):
            self._collect_step(t)
        with torch.no_grad():
            self.VNEXT.copy_(self.policy.predict_values(self.NEXT.reshape(-1, self.nx)).reshape(self.T, self.E))
        self._call("mpcrl_ppo_gae", self.REW, self.VAL, self.VNEXT, self.TERM, self.DONE, self.T, self.E, self.gamma, self.gae_lambda,
                   self.ADV, self.RET)

    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if (dist.is_available() and dist.is_initialized()) else 1

    def _minibatch(self, idx: torch.Tensor) -> None:
        import torch.distributed as dist
        B = self.B
        obs = self.OBS.reshape(-1, self.nx).index_select(0, idx)
        cold = (self.OK.reshape(-1).index_select(0, idx) == 0).to(torch.int32)     # no accepted roll-out solve: no iterate worth starting from
        self.sample_mpc.set_iterate_rows(*self.iters, index=idx)
        r = self.sample_mpc.solve(obs, sens_pi=True, cold_mask=cold)
        if self.nu > 1:
            self._call("mpcrl_ppo_surrogate_grad_nu", idx, B, self.T * self.E, self.ACT, self.LOGP, self.ADV, self.OK, r.u0, r.status, r.dpi_dp,
                       self.n_p, self.nu, self.log_std, self.lo_v, self.hi_v, self.clip_range, self.ent_coef, self.lr,
                       int(self.normalize_advantage), self._ws, self.msg)
        else:
            self._call("mpcrl_ppo_surrogate_grad", idx, B, self.T * self.E, self.ACT, self.LOGP, self.ADV, self.OK, r.u0, r.status, r.dpi_dp,
                       self.n_p, self.log_std, self.lo, self.hi, self.clip_range, self.ent_coef, self.lr, int(self.normalize_advantage),
                       self._ws, self.msg)
        world = self._world()
        if world > 1:
            dist.all_reduce(self.msg, op=dist.ReduceOp.SUM, group=self.group)      # the one collective of the policy step
        self._stat += self.msg[self.n_p + 1: self.n_p + MSG_EXTRA]
        self._stat_rows += B * world
        self._call("mpcrl_qlearning_apply", self.msg, self.n_p, self.learn_mask, self.theta, self.step_out)
        if self.nu > 1:
            self._call("mpcrl_ppo_log_std_apply_nu", self.msg, self.n_p, self.nu, self.log_std)
        else:
            self._call("mpcrl_ppo_log_std_apply", self.msg, self.n_p, self.log_std)
        for m in (self.rollout_mpc, self.sample_mpc):
            m.set_theta(self.theta)
        self._value_step(idx, obs, world)

    def _value_step(self, idx: torch.Tensor, obs: torch.Tensor, world: int) -> None:
        """The value network's step on the returns of the minibatch ``idx`` (``obs``: its observations, float64 [B, nx])."""
        import torch.distributed as dist
        B = self.B
        if self.value_kernels:
            self._call("mpcrl_value_mse_grad", self.OBS, self.RET, idx, B, self.T * self.E, self.ocp.nx, self.policy.value_flat, self.vf_coef,
                       1.0 / world, self._vws, self.vmsg)
            if world > 1:
                dist.all_reduce(self.vmsg, op=dist.ReduceOp.SUM, group=self.group)     # the one collective of the value step
            self.policy.value_grad_flat.copy_(self.vmsg[: self.n_value])
            self.policy.optimizer.step()
            return
        ret = self.RET.reshape(-1).index_select(0, idx).to(torch.float32)
        opt = self.policy.optimizer
        opt.zero_grad(set_to_none=False)
        loss = self.vf_coef * torch.nn.functional.mse_loss(self.policy.value_net(obs.to(torch.float32)).reshape(B), ret)
        loss.backward()
        self._vloss = loss.detach()
        if world > 1:
            for p in self.policy.value_net.parameters():
                dist.all_reduce(p.grad, op=dist.ReduceOp.SUM, group=self.group)
                p.grad /= world
        opt.step()

    def train(self) -> None:
        """n_epochs passes over the roll-out's T E samples in shuffled minibatches of batch_size."""
        self._stat.zero_()
        self._stat_rows = 0
        n = self.T * self.E
        for _ in range(self.n_epochs):
            perm = torch.randperm(n, generator=self.gen, device=self.device)
            for k in range(n // self.B):
                self._minibatch(perm[k * self.B:(k + 1) * self.B])

    def learn(self, n_iterations: int = 1) -> "BatchedPPO":
        for _ in range(n_iterations):
            self.collect()
            self.train()
            self.iterations += 1
        return self

    def last_stats(self) -> dict:
        """Statistics of the last train() (means over the valid rows of its minibatches) and of the last roll-out; ``value_loss`` is the
        MSE of the last minibatch's value step (its loss / vf_coef; NaN when vf_coef = 0).  Reads the device."""
        cnt, loss, kl, clipped, ratio, _, _ = self._stat.tolist()
        c = max(1.0, cnt)
        vl = float(self._vloss.item()) / (self._world() if self.value_kernels else 1)      # (the message's loss entry is summed over the ranks)
        return {"policy_loss": loss / c, "approx_kl": kl / c, "clip_fraction": clipped / c, "mean_ratio": ratio / c,
                "valid_fraction": cnt / max(1, self._stat_rows), "mean_reward": float(self.REW.mean().item()) / self.reward_scale,
                "log_std": float(self.log_std.mean().item()), "value_loss": vl / self.vf_coef if self.vf_coef != 0.0 else float("nan")}
