"""Batched Q-learning of the chain-of-masses MPC on the device: the loop of rlmpc/examples/linear_system_mpc_qlearning.py:153-205 around
the reference's largest model (rlmpc/mpc/chain_mass/ocp_utils.py), for E environments.

The reference has no plant for the chain: ``BatchedChainMassEnv`` (envs.py) is the model's own map — RK4 on the chain ODE
(ocp_utils.py:76-130) — at the PLANT's parameter vector, with a Gaussian disturbance on the free masses' accelerations.  ``ChainQLearning``
is ``DeviceQLearning`` (qlearning.py) with that plant and three controls.  Per time step the roll-out is ONE batched solve over the E
environments (warm, an episode's first solve cold per instance through the cold mask) and ONE launch of mpcrl_qlearning_chain_collect (the
three controls, optionally explored; the environment step; row t of the episode table; the next observation); the learning sweep is ONE
batched Q solve over all E (T - 1) samples (u0 fixed to the recorded actions, dQ/dp, cold), ONE V solve started from the Q solve's primal
iterate and ONE launch of mpcrl_qlearning_td_grad with a ``live`` table of ones: the T - 2 terms per environment of ``BatchedQLearning``'s
``td = C[:n-1] + gamma v[1:] - q[:-1]``.  With several ranks only the message is all-reduced; then mpcrl_qlearning_apply takes the mean and
steps the entries of theta that ``learn`` names.  ``enable_graphs()`` captures the roll-out step and the sweep as two HIP graphs.

The recorded cost is l(s_t, a_t) of the state BEFORE the step with the plant's own Q and R (see ``BatchedChainMassEnv``), the quantity
Q(s, a) models.  A term whose Q or V solve failed is left out (the reference raises); ``noise_scale`` > 0 adds
clip(a + sigma eps, lbu, ubu) exploration per control with float32 standard normals.  The plant's parameters are read from ``env.p`` at
every step.  There is no CPU path of the learner: the solver has none.  ``chain_env_step_terms`` states the plant and
``chain_collect_terms`` the roll-out kernel in torch float64: the CPU path of the environment, and what the tests hold the kernels to.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .envs import BatchedChainMassEnv, _chain_dims
from .problems import chain_param_layout
from .qlearning import DeviceQLearning, EpisodeStats


def _chain_ode_terms(M: int, m, D, L, C, w, x: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """ChainDev::ode_p of csrc/models_dev.hpp for a batch, in its grouping: x [E, nx], u [E, 3]; m [.., nl], D, L, C [.., nl, 3], w [.., M, 3]."""
    E = x.shape[0]
    pos, vel = x[:, : 3 * (M + 1)].reshape(E, M + 1, 3), x[:, 3 * (M + 1):].reshape(E, M, 3)
    z3 = torch.zeros(E, 1, 3, dtype=x.dtype, device=x.device)
    dist = pos - torch.cat([z3, pos[:, :-1]], 1)                                            # ocp_utils.py:80-84
    inrm = 1.0 / torch.sqrt(dist[..., 0] * dist[..., 0] + dist[..., 1] * dist[..., 1] + dist[..., 2] * dist[..., 2])[..., None]
    Fs = (D * (1.0 / m)[..., None]) * ((1.0 - L * inrm) * dist)                             # ocp_utils.py:86-88
    dv = torch.cat([vel, u[:, None, :]], 1) - torch.cat([z3, vel], 1)                       # ocp_utils.py:99-105
    Ft = Fs + C * dv                                                                        # ocp_utils.py:107-109
    grav = torch.tensor([0.0, 0.0, -9.81], dtype=x.dtype, device=x.device)
    acc = ((w + grav) - Ft[:, :M]) + Ft[:, 1:]                                              # ocp_utils.py:76-77,91-96,111-125
    return torch.cat([vel.reshape(E, -1), u, acc.reshape(E, -1)], 1)                        # ocp_utils.py:130


def chain_env_step_terms(ocp_or_dims, p: torch.Tensor, x_ss: torch.Tensor, state: torch.Tensor, action: torch.Tensor,
                         wn: Optional[torch.Tensor], w_std: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """chain_env_step of csrc/chain_env_kernel.hpp (mpcrl_env_chain_step) in torch float64, one rounding per operation, in the kernel's
    grouping.  ocp_or_dims: a ``chain_mass_ocp(...)`` or (n_mass, Ts, rk_steps); p [n_p] or [E, n_p] in the OCP's layout; x_ss [nx];
    state [E, nx]; action [E, 3], used as given; wn [E, 3 M] standard normals (None: no disturbance).  ``rk_steps`` RK4 steps of
    ``Ts / rk_steps`` on the chain ODE at p, with ``w_std * wn`` added to the free masses' accelerations of every evaluation (the ODE is
    additive in w: this is p's w + w_std * wn).  Returns the new state [E, nx] and
        cost [E] = 1/2 (s - x_ss)' Q (s - x_ss) + 1/2 a' R a
    of the state BEFORE the step with p's own Q and R.  (The kernel is compiled with floating-point contraction, so the two agree to
    rounding, not bit for bit.)"""
    n_mass, Ts, rk_steps = ocp_or_dims if isinstance(ocp_or_dims, (tuple, list)) else _chain_dims(ocp_or_dims)
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    x = state.to(torch.float64).reshape(-1, nx)
    E = x.shape[0]
    a = action.to(torch.float64).reshape(E, 3)
    p = p.to(torch.float64)
    if p.shape[-1] != n_p or p.dim() > 2:
        raise ValueError(f"p must be [{n_p}] or [E, {n_p}]")
    blk = lambda key, *shape: p[..., off[key][0]: off[key][1]].reshape(*p.shape[:-1], *shape)
    m, D, L, C, w = blk("m", nl), blk("D", nl, 3), blk("L", nl, 3), blk("C", nl, 3), blk("w", M, 3)
    Q, R = blk("Q", nx, nx).transpose(-1, -2), blk("R", 3, 3).transpose(-1, -2)           # column-major (ocp_utils.py:267)
    e = x - x_ss.to(torch.float64)
    quad = lambda v, W: sum(sum(v[:, i: i + 1] * W[..., i, :] for i in range(v.shape[1]))[:, j] * v[:, j] for j in range(v.shape[1]))
    cost = 0.5 * (quad(e, Q) + quad(a, R))                                                  # v' W v column by column, in the kernel's order
    nz = None if wn is None or w_std == 0.0 else w_std * wn.to(torch.float64).reshape(E, 3 * M)

    def f(xc):
        k = _chain_ode_terms(M, m, D, L, C, w, xc, a)
        return k if nz is None else torch.cat([k[:, : 3 * (M + 1)], k[:, 3 * (M + 1):] + nz], 1)

    h = Ts / rk_steps
    for _ in range(rk_steps):                                                               # ocp_utils.py:42-56
        k = f(x)
        acc = k
        k = f(x + (0.5 * h) * k)
        acc = acc + 2.0 * k
        k = f(x + (0.5 * h) * k)
        acc = acc + 2.0 * k
        k = f(x + h * k)
        x = x + (h / 6.0) * (acc + k)
    return x, cost


def chain_collect_terms(ocp_or_dims, p: torch.Tensor, x_ss: torch.Tensor, state: torch.Tensor, u0: torch.Tensor, status: torch.Tensor,
                        eps: torch.Tensor, wn: Optional[torch.Tensor], w_std: float, lo: Sequence[float], hi: Sequence[float], sigma: float
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One roll-out step in torch (what mpcrl_qlearning_chain_collect computes for an environment whose row lies inside the table).
    state [E, nx], u0 [E, 3], status [E], eps [E, 3] float32 and wn [E, 3 M] float64 (the step's rows of the draws), lo, hi: 3 each.
        good = status in {0, 2} and all three u0 finite;  act_j = good ? u0_j : 0;
        sigma > 0: act_j = clip(act_j + (double)(float32(sigma) * eps_j), lo_j, hi_j)
    Returns act [E, 3] (row t of A), the new state [E, nx] (the next row of S, the next observation) and the cost [E] (row t of C)."""
    u = u0.to(torch.float64).reshape(-1, 3)
    st = status.reshape(-1)
    good = ((st == 0) | (st == 2)) & torch.isfinite(u).all(1)
    act = torch.where(good[:, None], u, torch.zeros_like(u))
    sig = torch.tensor(sigma, dtype=torch.float32, device=u.device)
    if float(sig) > 0.0:                                   # sigma as the kernel holds it: a positive double that rounds to 0.0f explores nothing
        n = sig * eps.reshape(-1, 3).to(torch.float32)
        lo_t, hi_t = (torch.tensor([float(v) for v in b], dtype=torch.float64, device=u.device) for b in (lo, hi))
        act = torch.minimum(torch.maximum(act + n.to(torch.float64), lo_t), hi_t)
    new_state, cost = chain_env_step_terms(ocp_or_dims, p, x_ss, state, act, wn, w_std)
    return act, new_state, cost


def chain_theta_bounds(ocp, rel: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """Physical bounds (lo, hi), [n_p] float64 each, for ``ChainQLearning(theta_bounds=...)``: the masses m and the spring constants D
    within [(1 - rel) p0, (1 + rel) p0], 0 <= rel < 1 (they stay positive), every other entry unbounded (-inf, +inf)."""
    if not (0.0 <= rel < 1.0):
        raise ValueError("rel must lie in [0, 1)")
    n_mass = _chain_dims(ocp)[0]
    off = chain_param_layout(n_mass)[4]
    p0 = torch.as_tensor(ocp.p0, dtype=torch.float64)
    lo, hi = torch.full_like(p0, -float("inf")), torch.full_like(p0, float("inf"))
    for key in ("m", "D"):
        sl = slice(off[key][0], off[key][1])
        a, b = (1.0 - rel) * p0[sl], (1.0 + rel) * p0[sl]
        lo[sl], hi[sl] = torch.minimum(a, b), torch.maximum(a, b)
    return lo, hi


class ChainQLearning(DeviceQLearning):
    """Q-learning of the chain-of-masses MPC's parameters with E parallel chains (``env.num_envs``) and episodes of ``episode_length`` = T
    steps.  ``rollout_mpc`` solves the E policies, ``sample_mpc`` the E (T - 1) samples of the learning sweep.  ``gamma=None`` takes the
    OCP's discount factor (as ``BatchedQLearning``); both handles are set to it.

    ``learn``: the blocks of theta that are learned, any of "m", "D", "L", "C", "Q", "R", "w" (``chain_param_layout``).  The default is
    the dynamics block only: an unconstrained gradient step on Q or R can leave the cone of positive semi-definite matrices, after which
    the OCP is no longer convex in the cost.  ``lr``: the default is 1e-6.  The gradient's scale grows quickly with the chain: with every
    entry learned, ``lr = 1e-4`` moved the dynamics block by 6e-5 at n_mass 3 but by 0.045 at n_mass 5, where m itself is 0.033.
    ``method="gauss_newton"`` (``DeviceQLearning``) takes the damped least-squares TD step instead, whose ``lr`` in (0, 1] does not depend
    on the parameters' units; it learns at most 64 entries (m, D, L, C are 20 at n_mass 3 and 40 at n_mass 5; Q alone is 81 or more).
    ``trust_radius``, ``theta_bounds`` and ``theta_scale`` (``DeviceQLearning``) keep that step inside bounds and a trust region;
    ``chain_theta_bounds(ocp)`` keeps the masses and spring constants positive.

    Sizing: ``sample_mpc`` holds E (T - 1) chain instances, each with its trajectories and factorisation workspace — about 2 MB each at
    n_mass 5, N 40, so E = 256, T = 5 (1024 instances, the benchmark's chain5 batch) is about 2 GB.  ``workspace_bytes()`` returns
    (roll-out handle, sweep handle) as the library reports them."""

    NU = 3
    BLOCKS = ("m", "D", "L", "C", "Q", "R", "w")

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-6, gamma: Optional[float] = None, noise_scale: float = 0.0, seed: int = 0,
                 device=None, group=None, learn: Sequence[str] = ("m", "D", "L", "C"), method: str = "gradient", damping: float = 1e-3,
                 trust_radius: Optional[float] = None, theta_bounds=None, theta_scale=None):
        if getattr(ocp, "model", None) != _lib.MODEL_CHAIN or ocp.nu != 3:
            raise ValueError("ChainQLearning needs the chain-of-masses OCP (chain_mass_ocp())")
        if not isinstance(env, BatchedChainMassEnv):
            raise TypeError("ChainQLearning needs a BatchedChainMassEnv")
        n_mass, Ts, rk_steps = _chain_dims(ocp)
        if (env.n_mass, env.Ts, env.rk_steps, env.nx) != (n_mass, Ts, rk_steps, ocp.nx):
            raise ValueError("the environment was built for another chain (n_mass, Ts, rk_steps)")
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        for key in learn:
            if key not in self.BLOCKS:
                raise ValueError(f"learn: unknown block {key!r} (one of {', '.join(self.BLOCKS)})")
        self.NX = ocp.nx                                                     # per instance: the chain's size sets the state's width
        gamma = ocp.gamma if gamma is None else gamma
        super().__init__(ocp, env, episode_length, lr, gamma, noise_scale, seed, device, group, mpc_gamma=gamma, method=method,
                         damping=damping, trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale)
        self.n_mass, self.Ts, self.rk_steps, self.M, self.learn = n_mass, Ts, rk_steps, n_mass - 2, learn
        off = chain_param_layout(n_mass)[4]
        self.learn_mask.zero_()
        for key in learn:
            self.learn_mask[off[key][0]: off[key][1]] = 1.0
        if method == "gauss_newton":
            self._gn_setup()                                                 # (refuses more than 64 learned entries here, not at the first sweep)
        self.wn = torch.zeros(self.T, self.E, 3 * self.M, dtype=torch.float64, device=self.device)
        self.live = torch.ones(self.T, self.E, dtype=torch.uint8, device=self.device)    # the plant never terminates: every row is a sample

    def _initial_obs(self):
        # the zero state is no state of a chain: its masses coincide there and the ODE divides by their distance
        return self.ocp.x0

    def workspace_bytes(self) -> Tuple[int, int]:
        """Bytes of device memory of the roll-out handle (E instances) and of the sweep handle (E (T - 1) instances)."""
        return self.rollout_mpc.workspace_bytes(), self.sample_mpc.workspace_bytes()

    def _start_episode(self, x0: Optional[torch.Tensor] = None) -> None:
        super()._start_episode(x0)
        torch.randn(*self.wn.shape, generator=self.env.gen, dtype=torch.float64, device=self.device, out=self.wn)

    def _collect(self, r) -> None:
        env = self.env
        self._call("mpcrl_qlearning_chain_collect", self.n_mass, self.Ts, self.rk_steps, env.p, 0 if env.p.dim() == 1 else self.n_p, env.x_ss,
                   env.w_std, self.E, self.T, env.state, r.u0, r.status, self.eps, self.wn, self.lo_v, self.hi_v, self.noise_scale, self.obs,
                   self.row, self.cold, self.S, self.A, self.C)

    def _stats(self) -> EpisodeStats:
        nv = float(self.valid.sum().item())
        cand = float((self.T - 2) * self.E)
        return EpisodeStats(total_cost=float(self.C.sum().item()) / self.E, td_error_mean=float(self.td.sum().item()) / max(1.0, nv),
                            step=self.step_out.clone(), converged_fraction=nv / cand if cand > 0 else 1.0)
