"""Batched Q-learning of the cartpole MPC: scripts/cartpole_mpc_qlearning.py:200-263 of the reference for E environments, on the device.

Per episode the reference script
    rolls out until ``done`` (or MAX_EPISODE_LENGTH - 1 steps):  a = perturb_action(mpc.get_action(s)) = clip(a + 0.1 N(0, 1), -1, 1),
        env.step(a), replay_buffer.add(...)                                                             (223-234, 104-107)
    for every stored sample i < size - 1:  Q_i, dQ/dp_i = mpc.q_update(s_i, unscale_action(a_i));  V_i = mpc.update(s_i)   (240-249)
    td_i = cost_i + GAMMA V_{i+1} - Q_i  (i < size - 2);   p += mean_i(LR td_i dQ/dp_i)                 (255-269)
Here the roll-out is, per time step, ONE batched solve over the E environments and ONE launch of mpcrl_qlearning_cartpole_collect (the
action with its exploration noise, the environment step, row t of the episode table, the environments' liveness); the learning sweep is
ONE batched Q solve over all E (T - 1) samples (u0 fixed to the recorded unscaled actions, dQ/dp, cold), ONE V solve warm-started from the
Q solve's primal iterate (the reference's q_update -> update on one solver; the bound multipliers start cold, as the Q solve's pinned u0
bound makes its own a poor interior-point start), and ONE launch of mpcrl_qlearning_td_grad (TD errors, validity, and the message
[sum lr td dQ/dp, sum lr td, count] of distributed.mean_update).  With several ranks only that message is all-reduced; then
mpcrl_qlearning_apply takes the mean and steps theta.  ``enable_graphs()`` captures the roll-out step and the sweep as two HIP graphs.

Differences from the script, on purpose:
  * the script does ``obs = next_obs`` BEFORE ``replay_buffer.add(obs=obs, ...)`` (lines 229-231), so it stores s_{t+1} as the observation
    of (a_t, c_t).  The table here stores s_t, which is what the TD formula means;
  * an environment's episode ends when it is terminated, or truncated at the environment's max_episode_steps, or after T steps; the
    mean of the step is over the valid terms of ALL environments (and ranks); a term whose Q or V solve failed is left out (the reference
    raises instead, mpc.py:81-83,197-198);
  * the parameter vector is the engine's cartpole p: (M, m, l) are learned, the cost block is not (config/cartpole.yaml:75-78 keeps g
    fixed).  Learning g as well — the script's "unfix all" — needs a p layout with g in it and is NOT supported here;
  * the exploration draws are float32 standard normals (the TD3 loop's convention), from the learner's own generator;
  * rows of an environment that has ended are still solved (the batch shape is fixed): they hold the environment's final state and a zero
    action, and never reach the step.
The MPC keeps the OCP's own discount factor; ``gamma`` is the TD discount (the script's GAMMA).  There is no CPU path: the solver has
none.  ``qlearning_td_terms`` states the TD step in torch (the reference the tests hold the kernel to).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .envs import BatchedCartPoleSwingUpEnv
from .qlearning import DeviceQLearning, EpisodeStats


@dataclass
class CartpoleEpisodeStats(EpisodeStats):
    """EpisodeStats (total_cost = sum of the recorded costs / E; td_error_mean over the valid terms; converged_fraction = valid terms /
    terms of the episodes' samples) plus the rows every environment recorded."""
    episode_lengths: torch.Tensor = None     # [E] int64


def qlearning_td_terms(q: torch.Tensor, v: torch.Tensor, dq: torch.Tensor, status_q: torch.Tensor, status_v: torch.Tensor,
                       cost: torch.Tensor, live: torch.Tensor, gamma: float, lr: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The TD step of one episode in torch (what mpcrl_qlearning_td_grad computes).  q, v, status_q, status_v [T-1, E], dq [T-1, E, n_p]
    (the learning sweep over sample rows i < T - 1), cost, live [T, E] (the episode table).  With L_e = live[:, e].sum() the rows
    environment e recorded, term (i, e), i < T - 2, is valid when rows i and i + 1 are live, i + 1 < L_e - 1 (the script's size - 1
    samples and td[:-1]) and the Q and V solves of both rows returned 0.  Returns
        msg [n_p + 2] = [sum lr td dQ/dp, sum lr td, count] over the valid terms,  td [T-2, E] (0 where not valid),  valid [T-2, E] bool."""
    T = cost.shape[0]
    n_t = max(T - 2, 0)
    lv = live.to(torch.bool)
    L = lv.to(torch.int64).sum(0)
    i = torch.arange(n_t, device=cost.device)[:, None]
    ok = (status_q == 0) & (status_v == 0)
    valid = lv[:n_t] & lv[1:n_t + 1] & (i + 1 < L[None, :] - 1) & ok[:n_t] & ok[1:n_t + 1]
    td = cost[:n_t] + gamma * v[1:n_t + 1] - q[:n_t]
    td = torch.where(valid, td, torch.zeros_like(td))            # selected: Q / V of a failed solve may be NaN
    w = torch.where(valid, lr * td, torch.zeros_like(td))
    g = torch.where(valid[..., None], torch.nan_to_num(dq[:n_t]), torch.zeros_like(dq[:n_t]))
    msg = torch.cat([(w[..., None] * g).sum((0, 1)), w.sum().reshape(1), valid.sum().to(torch.float64).reshape(1)])
    return msg, td, valid


class CartpoleQLearning(DeviceQLearning):
    """Q-learning of the cartpole MPC's parameters with E parallel environments (``env.num_envs``) and episodes of at most
    ``episode_length`` = T steps.  ``rollout_mpc`` solves the E policies, ``sample_mpc`` the E (T - 1) samples of the learning sweep.
    Of theta, (M, m, l) are learned."""

    NX = 4

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-4, gamma: float = 0.99, noise_scale: float = 0.1, seed: int = 0,
                 device=None, group=None, method: str = "gradient", damping: float = 1e-3, trust_radius: Optional[float] = None,
                 theta_bounds=None, theta_scale=None):
        if getattr(ocp, "model", None) != _lib.MODEL_CARTPOLE or ocp.nu != 1 or ocp.nx != 4:
            raise ValueError("CartpoleQLearning needs the cartpole OCP (cartpole_ocp())")
        if not isinstance(env, BatchedCartPoleSwingUpEnv):
            raise TypeError("CartpoleQLearning needs a BatchedCartPoleSwingUpEnv")
        super().__init__(ocp, env, episode_length, lr, gamma, noise_scale, seed, device, group, method=method, damping=damping,
                         trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale)
        self.alive = torch.zeros(self.E, dtype=torch.uint8, device=self.device)
        self.live = torch.zeros(self.T, self.E, dtype=torch.uint8, device=self.device)

    def _start_episode(self, x0: Optional[torch.Tensor] = None) -> None:
        super()._start_episode(x0)
        self.alive.fill_(1)

    def _collect(self, r) -> None:
        env = self.env
        self._call("mpcrl_qlearning_cartpole_collect", env._par(), self.E, self.T, env.state, env.steps, r.u0, r.status, self.eps, self.lo,
                   self.hi, self.noise_scale, self.obs, self.alive, self.row, self.cold, self.S, self.A, self.C, self.live)

    def _env_carried(self):
        return [self.env.state, self.env.steps]

    def _stats(self) -> CartpoleEpisodeStats:
        L = self.live.to(torch.int64).sum(0)
        nv = float(self.valid.sum().item())
        cand = float(torch.clamp(L - 2, min=0).sum().item())
        return CartpoleEpisodeStats(total_cost=float(self.C.sum().item()) / self.E, td_error_mean=float(self.td.sum().item()) / max(1.0, nv),
                                    step=self.step_out.clone(), converged_fraction=nv / cand if cand > 0 else 1.0, episode_lengths=L)
