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
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .batch import MPCBatch, _ptr
from .envs import BatchedLinearSystemEnv
from .qlearning import EpisodeStats


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


class LinearQLearning:
    """Q-learning of the linear-system MPC's parameters with E parallel environments (``env.num_envs``) and episodes of
    ``episode_length`` = T steps.  ``rollout_mpc`` solves the E policies, ``sample_mpc`` the E (T - 1) samples of the learning sweep.
    ``gamma=None`` takes the OCP's discount factor (as ``BatchedQLearning``); both handles are set to it."""

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-4, gamma: Optional[float] = None, noise_scale: float = 0.0, seed: int = 0,
                 device=None, group=None):
        if getattr(ocp, "model", None) != _lib.MODEL_LINEAR or ocp.nu != 1 or ocp.nx != 2:
            raise ValueError("LinearQLearning needs the linear-system OCP (linear_system_ocp())")
        if not isinstance(env, BatchedLinearSystemEnv):
            raise TypeError("LinearQLearning needs a BatchedLinearSystemEnv")
        if isinstance(episode_length, bool) or not isinstance(episode_length, int) or episode_length < 2:
            raise ValueError("episode_length must be an int >= 2 (a TD term needs two samples)")
        if not math.isfinite(lr):
            raise ValueError("lr must be finite")
        gamma = ocp.gamma if gamma is None else gamma
        if not (0.0 < gamma <= 1.0):
            raise ValueError("gamma must lie in (0, 1]")
        if not (math.isfinite(noise_scale) and noise_scale >= 0.0):
            raise ValueError("noise_scale must be finite and >= 0")
        dev = env.device if device is None else torch.device(device)
        if dev.type != "cuda" or env.device.type != "cuda":
            raise RuntimeError("LinearQLearning runs on a HIP device (the environment's state too); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if env.device.index is not None and env.device != dev:
            raise ValueError("the environment must live on the learner's device (its state is updated in place by the library)")
        self.ocp, self.env, self.T, self.lr, self.gamma, self.noise_scale = ocp, env, episode_length, float(lr), float(gamma), float(noise_scale)
        self.E, self.device, self.group = env.num_envs, dev, group
        T, E = self.T, self.E
        self.rollout_mpc = MPCBatch(ocp, E, dev)
        self.sample_mpc = MPCBatch(ocp, E * (T - 1), dev)
        for m in (self.rollout_mpc, self.sample_mpc):
            m.set_discount_factor(self.gamma)
        self.n_p = ocp.n_p
        f64 = dict(dtype=torch.float64, device=dev)
        self.theta = torch.as_tensor(ocp.p0, **f64).clone()            # updated in place (the handles copy it after every step)
        self.learn_mask = torch.zeros_like(self.theta)
        self.learn_mask[: ocp.n_model_p] = 1.0                          # all of A, B, b, V_0, f
        self.lo, self.hi = float(ocp.lbu[0]), float(ocp.ubu[0])
        self.par = linear_env_par(env)
        self._par_c = (ctypes.c_double * 12)(*self.par)
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        # the episode's device state: every buffer keeps its address (captured graphs hold them)
        self.obs = torch.zeros(E, 2, **f64)
        self.row = torch.zeros(E, dtype=torch.int32, device=dev)
        self.cold = torch.ones(E, dtype=torch.int32, device=dev)
        self.eps = torch.zeros(T, E, dtype=torch.float32, device=dev)
        self.u01 = torch.zeros(T, E, **f64)
        self.S = torch.zeros(T, E, 2, **f64)
        self.A = torch.zeros(T, E, **f64)
        self.C = torch.zeros(T, E, **f64)
        self.live = torch.ones(T, E, dtype=torch.uint8, device=dev)    # the environment never terminates: every row is a sample
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
        self.last = None                # the roll-out solves of the last eager episode, one SolveResult per step
        self.last_sweep = None          # (Q solve, V solve) of the last episode's learning sweep
        self.episodes = 0

    # ------------------------------------------------------------------ pieces (the same launches eager and captured)
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _start_episode(self, x0: Optional[torch.Tensor] = None) -> None:
        self.env.reset()
        if x0 is not None:
            self.env.state.copy_(torch.as_tensor(x0, dtype=torch.float64, device=self.device).reshape(self.E, 2))
        self.obs.copy_(self.env.state)
        self.row.zero_()
        self.cold.fill_(1)
        torch.randn(self.T, self.E, generator=self.gen, dtype=torch.float32, device=self.device, out=self.eps)
        torch.rand(self.T, self.E, generator=self.env.gen, dtype=torch.float64, device=self.device, out=self.u01)

    def _rollout_step(self):
        r = self.rollout_mpc.solve(self.obs, cold_mask=self.cold)           # the policy of every environment (mpc.get_action), one launch
        with torch.cuda.device(self.device):
            rc = self._lib.mpcrl_qlearning_linear_collect(
                self._par_c, self.E, self.T, _ptr(self.env.state), _ptr(r.u0), _ptr(r.status), _ptr(self.eps), _ptr(self.u01), self.lo, self.hi,
                self.noise_scale, _ptr(self.obs), _ptr(self.row), _ptr(self.cold), _ptr(self.S), _ptr(self.A), _ptr(self.C), self._stream())
        if rc != 0:
            raise RuntimeError(f"mpcrl_qlearning_linear_collect failed with {rc}")
        return r

    def _sweep(self):
        n = self.T - 1
        s = self.S[:n].reshape(n * self.E, 2)
        a = self.A[:n].reshape(n * self.E, 1)
        # q_update: Q(s_i, a_i), dQ/dp_i (181-187); its bound multipliers are not kept (the module docstring) ...
        rq = self.sample_mpc.solve(s, u0=a, sens_v=True, cold=True, store_bounds=False)
        # ... update: V(s_i) from the Q solve's primal iterate, interior point from its default point (189-190)
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
            m.set_theta(self.theta)                                    # mpc.set_parameter (204-205)

    # ------------------------------------------------------------------ the episode
    def run_episode(self, x0: Optional[torch.Tensor] = None) -> EpisodeStats:
        """One episode of all E environments, its learning sweep and the parameter step.  x0 [E, 2]: the initial states, instead of the
        environment's reset state."""
        self._start_episode(x0)
        if self._graphs is not None:
            for _ in range(self.T):
                self._graphs["rollout"].replay()
            self._graphs["sweep"].replay()
            self.last, self.last_sweep = None, self._graphs["sweep_out"]
        else:
            self.last = [self._rollout_step() for _ in range(self.T)]
            self.last_sweep = self._sweep()
        self._allreduce()                                               # the one collective of an episode (world > 1)
        self._apply()
        self.episodes += 1
        return self._stats()

    def _stats(self) -> EpisodeStats:
        nv = float(self.valid.sum().item())
        cand = float((self.T - 2) * self.E)
        return EpisodeStats(total_cost=float(self.C.sum().item()) / self.E, td_error_mean=float(self.td.sum().item()) / max(1.0, nv),
                            step=self.step_out.clone(), converged_fraction=nv / cand if cand > 0 else 1.0)

    # ------------------------------------------------------------------ HIP graphs
    def enable_graphs(self) -> None:
        """Captures one roll-out step (solve + collect; replayed T times per episode) and the learning sweep (Q solve, V solve, TD kernel)
        as two HIP graphs.  The episode start, the collective and the apply stay eager calls, so episodes are bit-identical to the eager
        ones.  A warm-up of both pieces runs first on the capture stream (lazy initialisation, the solves' launch shape); the
        environment's state is put back afterwards, and nothing else the learner carries from one episode to the next is touched by it."""
        if self._graphs is not None:
            return
        dev = self.device
        snap = self.env.state.clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._rollout_step()
            self._sweep()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.env.state.copy_(snap)
        torch.cuda.synchronize(dev)
        g_roll, g_sweep = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_roll, stream=side):
            self._rollout_step()
        with torch.cuda.graph(g_sweep, stream=side):
            out = self._sweep()
        torch.cuda.synchronize(dev)
        self._graphs = {"rollout": g_roll, "sweep": g_sweep, "sweep_out": out}
