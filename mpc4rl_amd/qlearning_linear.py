"""Batched Q-learning of the linear-system MPC on the device: rlmpc/examples/linear_system_mpc_qlearning.py:153-205 for E environments.

``BatchedQLearning`` (qlearning.py) is the model-agnostic torch form of that loop; this is its device form for the plant the example is
written for, in the shape of ``CartpoleQLearning``.  Per time step the roll-out is ONE batched solve over the E environments (warm, an
episode's first solve cold per instance through the cold mask) and ONE launch of mpcrl_qlearning_linear_collect (the action, the
environment step, row t of the episode table, the next observation); the learning sweep is ONE batched Q solve over all E (T - 1)
samples (u0 fixed to the recorded actions, dQ/dp, cold), ONE V solve started from the Q solve's primal iterate and ONE launch of
mpcrl_qlearning_td_grad with a ``live`` table of ones, which gives exactly the T - 2 terms per environment of ``BatchedQLearning``'s
``td = C[:n-1] + gamma v[1:] - q[:-1]``.  With several ranks only the message is all-reduced; then mpcrl_qlearning_apply takes the mean and
steps theta (all 12 entries: A, B, b, V_0, f).  ``enable_graphs()`` captures the roll-out step and the sweep as two HIP graphs.

The Q solve does not keep its bound multipliers (``store_bounds=False``).  That is right for the linear handle: lq_solve_kernel honours
MPCRL_NO_BND_STORE and mpcrl_solve then marks the stored multipliers as placeholders, so the V solve starts from the Q solve's x, u, pi
with its interior point at the default point (MPCRL_COLD_DUAL) — the Q solve's pinned u0 bound makes its multipliers a poor interior-point
start for the free problem.  At short horizons, where the handle falls back to the one-stage kernel, the planes are stored and then
ignored by the same flag: the same start, one wasted store.

Differences from the example, on purpose: the mean of the step is over the valid terms of ALL environments (and ranks), a term whose Q or
V solve failed is left out (the reference raises); ``noise_scale`` > 0 adds clip(a + sigma eps, lbu, ubu) exploration with float32
standard normals (the example has none: the default is 0).  The environment's parameters are read when the learner is built.  There is no
CPU path: the solver has none.  ``linear_collect_terms`` states the roll-out kernel in torch float64 (what the tests hold it to).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .envs import BatchedLinearSystemEnv
from .qlearning import DeviceQLearning, EpisodeStats


def linear_env_par(env: BatchedLinearSystemEnv) -> list:
    """The 12 doubles mpcrl_env_linear_step takes: A (row-major), B, lb_noise, ub_noise, min_observation, max_observation."""
    return (env.A.reshape(-1).tolist() + env.B.reshape(-1).tolist() + [float(env.lb_noise), float(env.ub_noise)] + env.low.tolist()
            + env.high.tolist())


def linear_env_step_terms(par: Sequence[float], state: torch.Tensor, action: torch.Tensor, u01: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """linear_env_step of csrc/env_kernel.hpp in torch float64, one rounding per operation, in the kernel's grouping.  par: the 12
    doubles of ``linear_env_par``; state [E, 2], action [E], u01 [E].  Returns the new state [E, 2] and the cost [E].  (The kernel is
    compiled with floating-point contraction and the environment's CPU path goes through a matrix product, so the three agree bit for bit
    where the products are exact and to a few roundings otherwise.)"""
    A0, A1, A2, A3, B0, B1, lb, ub, l0, l1, h0, h1 = (float(v) for v in par)
    x0, x1 = state[:, 0], state[:, 1]
    a = action.reshape(-1)
    n0 = lb + (ub - lb) * u01.reshape(-1)
    s0 = (x0 * A0 + x1 * A1) + a * B0 + n0
    s1 = (x0 * A2 + x1 * A3) + a * B1
    hundred, zero = torch.full_like(s0, 1e2), torch.zeros_like(s0)
    lower = torch.where((l0 - s0 > 0.0) | (l1 - s1 > 0.0), hundred, zero)
    upper = torch.where((s0 - h0 > 0.0) | (s1 - h1 > 0.0), hundred, zero)
    cost = 0.5 * (s0 * s0 + s1 * s1) + 0.5 * (a * a) + lower + upper
    return torch.stack([s0, s1], 1), cost


def linear_collect_terms(par: Sequence[float], state: torch.Tensor, u0: torch.Tensor, status: torch.Tensor, eps: torch.Tensor,
                         u01: torch.Tensor, lo: float, hi: float, sigma: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One roll-out step in torch (what mpcrl_qlearning_linear_collect computes for an environment whose row lies inside the table).
    state [E, 2], u0 [E] (or [E, 1]), status [E], eps [E] float32 and u01 [E] float64 (the step's rows of the draws).
        act = status in {0, 2} and u0 finite ? u0 : 0;   sigma > 0: act = clip(act + (double)(float32(sigma) * eps), lo, hi)
    Returns act [E] (row t of A), the new state [E, 2] (the next row of S, the next observation) and the cost [E] (row t of C)."""
    u = u0.to(torch.float64).reshape(-1)
    good = ((status.reshape(-1) == 0) | (status.reshape(-1) == 2)) & torch.isfinite(u)
    act = torch.where(good, u, torch.zeros_like(u))
    if sigma > 0.0:
        n = torch.tensor(sigma, dtype=torch.float32, device=u.device) * eps.reshape(-1).to(torch.float32)
        act = torch.clamp(act + n.to(torch.float64), lo, hi)
    new_state, cost = linear_env_step_terms(par, state.to(torch.float64), act, u01.to(torch.float64))
    return act, new_state, cost


class LinearQLearning(DeviceQLearning):
    """Q-learning of the linear-system MPC's parameters with E parallel environments (``env.num_envs``) and episodes of
    ``episode_length`` = T steps.  ``rollout_mpc`` solves the E policies, ``sample_mpc`` the E (T - 1) samples of the learning sweep.
    ``gamma=None`` takes the OCP's discount factor (as ``BatchedQLearning``); both handles are set to it.  All of theta (A, B, b, V_0,
    f) is learned."""

    NX = 2

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-4, gamma: Optional[float] = None, noise_scale: float = 0.0, seed: int = 0,
                 device=None, group=None, method: str = "gradient", damping: float = 1e-3, trust_radius: Optional[float] = None,
                 theta_bounds=None, theta_scale=None):
        if getattr(ocp, "model", None) != _lib.MODEL_LINEAR or ocp.nu != 1 or ocp.nx != 2:
            raise ValueError("LinearQLearning needs the linear-system OCP (linear_system_ocp())")
        if not isinstance(env, BatchedLinearSystemEnv):
            raise TypeError("LinearQLearning needs a BatchedLinearSystemEnv")
        gamma = ocp.gamma if gamma is None else gamma
        super().__init__(ocp, env, episode_length, lr, gamma, noise_scale, seed, device, group, mpc_gamma=gamma, method=method,
                         damping=damping, trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale)
        self.par = linear_env_par(env)
        self._par_c = (ctypes.c_double * 12)(*self.par)
        self.u01 = torch.zeros(self.T, self.E, dtype=torch.float64, device=self.device)
        self.live = torch.ones(self.T, self.E, dtype=torch.uint8, device=self.device)    # the environment never terminates: every row is a sample

    def _start_episode(self, x0: Optional[torch.Tensor] = None) -> None:
        super()._start_episode(x0)
        torch.rand(self.T, self.E, generator=self.env.gen, dtype=torch.float64, device=self.device, out=self.u01)

    def _collect(self, r) -> None:
        self._call("mpcrl_qlearning_linear_collect", self._par_c, self.E, self.T, self.env.state, r.u0, r.status, self.eps, self.u01, self.lo,
                   self.hi, self.noise_scale, self.obs, self.row, self.cold, self.S, self.A, self.C)

    def _stats(self) -> EpisodeStats:
        nv = float(self.valid.sum().item())
        cand = float((self.T - 2) * self.E)
        return EpisodeStats(total_cost=float(self.C.sum().item()) / self.E, td_error_mean=float(self.td.sum().item()) / max(1.0, nv),
                            step=self.step_out.clone(), converged_fraction=nv / cand if cand > 0 else 1.0)
