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

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .batch import MPCBatch, _ptr
from .envs import BatchedCartPoleSwingUpEnv
from .qlearning import EpisodeStats


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


class CartpoleQLearning:
    """Q-learning of the cartpole MPC's parameters with E parallel environments (``env.num_envs``) and episodes of at most
    ``episode_length`` = T steps.  ``rollout_mpc`` solves the E policies, ``sample_mpc`` the E (T - 1) samples of the learning sweep."""

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-4, gamma: float = 0.99, noise_scale: float = 0.1, seed: int = 0,
                 device=None, group=None):
        if getattr(ocp, "model", None) != _lib.MODEL_CARTPOLE or ocp.nu != 1 or ocp.nx != 4:
            raise ValueError("CartpoleQLearning needs the cartpole OCP (cartpole_ocp())")
        if not isinstance(env, BatchedCartPoleSwingUpEnv):
            raise TypeError("CartpoleQLearning needs a BatchedCartPoleSwingUpEnv")
        if isinstance(episode_length, bool) or not isinstance(episode_length, int) or episode_length < 2:
            raise ValueError("episode_length must be an int >= 2 (a TD term needs two samples)")
        if not math.isfinite(lr):
            raise ValueError("lr must be finite")
        if not (0.0 < gamma <= 1.0):
            raise ValueError("gamma must lie in (0, 1]")
        if not (math.isfinite(noise_scale) and noise_scale >= 0.0):
            raise ValueError("noise_scale must be finite and >= 0")
        dev = env.device if device is None else torch.device(device)
        if dev.type != "cuda" or env.device.type != "cuda":
            raise RuntimeError("CartpoleQLearning runs on a HIP device (the environment's state too); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if env.device.index is not None and env.device != dev:
            raise ValueError("the environment must live on the learner's device (its state is updated in place by the library)")
        self.ocp, self.env, self.T, self.lr, self.gamma, self.noise_scale = ocp, env, episode_length, float(lr), float(gamma), float(noise_scale)
        self.E, self.device, self.group = env.num_envs, dev, group
        T, E = self.T, self.E
        self.rollout_mpc = MPCBatch(ocp, E, dev)
        self.sample_mpc = MPCBatch(ocp, E * (T - 1), dev)
        self.n_p = ocp.n_p
        f64 = dict(dtype=torch.float64, device=dev)
        self.theta = torch.as_tensor(ocp.p0, **f64).clone()            # updated in place (the handles copy it after every step)
        self.learn_mask = torch.zeros_like(self.theta)
        self.learn_mask[: ocp.n_model_p] = 1.0                          # (M, m, l)
        self.lo, self.hi = float(ocp.lbu[0]), float(ocp.ubu[0])
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        # the episode's device state: every buffer keeps its address (captured graphs hold them)
        self.obs = torch.zeros(E, 4, **f64)
        self.alive = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.row = torch.zeros(E, dtype=torch.int32, device=dev)
        self.cold = torch.ones(E, dtype=torch.int32, device=dev)
        self.eps = torch.zeros(T, E, dtype=torch.float32, device=dev)
        self.S = torch.zeros(T, E, 4, **f64)
        self.A = torch.zeros(T, E, **f64)
        self.C = torch.zeros(T, E, **f64)
        self.live = torch.zeros(T, E, dtype=torch.uint8, device=dev)
        self.td = torch.zeros(T - 2, E, **f64)
        self.valid = torch.zeros(T - 2, E, dtype=torch.uint8, device=dev)
        self.msg = torch.zeros(self.n_p + 2, **f64)
        self.step_out = torch.zeros(self.n_p, **f64)
        self._lib = _lib.load()
        nb = int(self._lib.mpcrl_qlearning_td_workspace_bytes(T, E, self.n_p))
        if nb < 0:
            raise RuntimeError(f"mpcrl_qlearning_td_workspace_bytes failed with {nb}")
        self._td_ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
        # the roll-out handle holds an iterate from here on, so that the first solve of every episode (eager or replayed) is the
        # per-instance cold start of the cold mask, never the handle-wide one of a fresh handle
        self.rollout_mpc.solve(self.obs, cold=True)
        self._graphs = None
        self.last_sweep = None          # (Q solve, V solve) of the last episode's learning sweep
        self.episodes = 0

    # ------------------------------------------------------------------ pieces (the same launches eager and captured)
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _start_episode(self, x0: Optional[torch.Tensor] = None) -> None:
        self.env.reset()
        if x0 is not None:
            self.env.state.copy_(torch.as_tensor(x0, dtype=torch.float64, device=self.device).reshape(self.E, 4))
        self.obs.copy_(self.env.state)
        self.alive.fill_(1)
        self.row.zero_()
        self.cold.fill_(1)
        torch.randn(self.T, self.E, generator=self.gen, dtype=torch.float32, device=self.device, out=self.eps)

    def _rollout_step(self) -> None:
        r = self.rollout_mpc.solve(self.obs, cold_mask=self.cold)           # the policy of every environment (mpc.get_action), one launch
        env = self.env
        with torch.cuda.device(self.device):
            rc = self._lib.mpcrl_qlearning_cartpole_collect(
                env._par(), self.E, self.T, _ptr(env.state), _ptr(env.steps), _ptr(r.u0), _ptr(r.status), _ptr(self.eps), self.lo, self.hi,
                self.noise_scale, _ptr(self.obs), _ptr(self.alive), _ptr(self.row), _ptr(self.cold), _ptr(self.S), _ptr(self.A), _ptr(self.C),
                _ptr(self.live), self._stream())
        if rc != 0:
            raise RuntimeError(f"mpcrl_qlearning_cartpole_collect failed with {rc}")

    def _sweep(self):
        n = self.T - 1
        s = self.S[:n].reshape(n * self.E, 4)
        a = self.A[:n].reshape(n * self.E, 1)
        # q_update: Q(s_i, a_i), dQ/dp_i (240-246); its bound multipliers are not kept (store_bounds=False) ...
        rq = self.sample_mpc.solve(s, u0=a, sens_v=True, cold=True, store_bounds=False)
        # ... update: V(s_i) from the Q solve's primal iterate, interior point from its default point (248-249)
        rv = self.sample_mpc.solve(s)
        with torch.cuda.device(self.device):
            rc = self._lib.mpcrl_qlearning_td_grad(
                _ptr(rq.V), _ptr(rv.V), _ptr(rq.dV_dp), _ptr(rq.status), _ptr(rv.status), _ptr(self.C), _ptr(self.live), self.T, self.E, self.n_p,
                self.gamma, self.lr, _ptr(self._td_ws), _ptr(self.td), _ptr(self.valid), _ptr(self.msg), self._stream())
        if rc != 0:
            raise RuntimeError(f"mpcrl_qlearning_td_grad failed with {rc}")
        return rq, rv

    def _allreduce(self) -> None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and (self.group is not None or dist.get_world_size() > 1):
            dist.all_reduce(self.msg, op=dist.ReduceOp.SUM, group=self.group)

    def _apply(self) -> None:
        with torch.cuda.device(self.device):
            rc = self._lib.mpcrl_qlearning_apply(_ptr(self.msg), self.n_p, _ptr(self.learn_mask), _ptr(self.theta), _ptr(self.step_out),
                                                 self._stream())
        if rc != 0:
            raise RuntimeError(f"mpcrl_qlearning_apply failed with {rc}")
        for m in (self.rollout_mpc, self.sample_mpc):
            m.set_theta(self.theta)                                    # mpc.set_p (269)

    # ------------------------------------------------------------------ the episode
    def run_episode(self, x0: Optional[torch.Tensor] = None) -> CartpoleEpisodeStats:
        """One episode of all E environments, its learning sweep and the parameter step.  x0 [E, 4]: the initial states, instead of the
        environment's reset draw (which is taken all the same, so the environment's generator advances alike)."""
        self._start_episode(x0)
        if self._graphs is not None:
            for _ in range(self.T):
                self._graphs["rollout"].replay()
            self._graphs["sweep"].replay()
            self.last_sweep = self._graphs["sweep_out"]
        else:
            for _ in range(self.T):
                self._rollout_step()
            self.last_sweep = self._sweep()
        self._allreduce()                                               # the one collective of an episode (world > 1)
        self._apply()
        self.episodes += 1
        return self._stats()

    def _stats(self) -> CartpoleEpisodeStats:
        L = self.live.to(torch.int64).sum(0)
        nv = float(self.valid.sum().item())
        cand = float(torch.clamp(L - 2, min=0).sum().item())
        return CartpoleEpisodeStats(total_cost=float(self.C.sum().item()) / self.E, td_error_mean=float(self.td.sum().item()) / max(1.0, nv),
                                    step=self.step_out.clone(), converged_fraction=nv / cand if cand > 0 else 1.0, episode_lengths=L)

    # ------------------------------------------------------------------ HIP graphs
    def enable_graphs(self) -> None:
        """Captures one roll-out step (solve + collect; replayed T times per episode) and the learning sweep (Q solve, V solve, TD kernel)
        as two HIP graphs.  The episode start, the collective and the apply stay eager calls, so episodes are bit-identical to the eager
        ones.  A warm-up of both pieces runs first on the capture stream (lazy initialisation, the solves' launch shape); the
        environment's state is put back afterwards, and nothing else the learner carries from one episode to the next is touched by it."""
        if self._graphs is not None:
            return
        dev = self.device
        snap = (self.env.state.clone(), self.env.steps.clone())
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._rollout_step()
            self._sweep()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.env.state.copy_(snap[0]), self.env.steps.copy_(snap[1])
        torch.cuda.synchronize(dev)
        g_roll, g_sweep = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_roll, stream=side):
            self._rollout_step()
        with torch.cuda.graph(g_sweep, stream=side):
            out = self._sweep()
        torch.cuda.synchronize(dev)
        self._graphs = {"rollout": g_roll, "sweep": g_sweep, "sweep_out": out}
