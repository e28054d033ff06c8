"""The deterministic policy gradient of the MPC's parameters with a compatible linear critic, from the roll-out's own du0*/dp.

The MPC is the policy, pi_theta(s) = u0*(s; theta).  The deterministic policy gradient theorem with the compatible critic
    A_w(s, a) = (a - pi(s))' dpi/dtheta(s)' w
gives
    grad_theta J = E[ dpi/dtheta(s) dpi/dtheta(s)' ] w,
and the natural gradient is w itself.  w is fitted by least squares to the one-step TD residual of a baseline.  Everything this needs
is computed while the episode is rolled out: pi(s_t) = u0* and dpi/dtheta = du0*/dp (the solver's ``sens_pi`` output) come from the
roll-out solve, V(s_t) of the same solve is the baseline, and a_t - pi(s_t) is the exploration that was applied.  So an episode needs
no learning sweep, no second handle of E (T - 1) instances and no network: T roll-out solves with ``sens_pi``, one reduction launch
(mpcrl_cdpg_terms) and one small solve (mpcrl_cdpg_apply).

What the critic is, and is not.  The baseline is the MPC's own V_theta, not a fitted value function of the policy.  delta_t = c_t +
gamma V_theta(s_{t+1}) - V_theta(s_t) is therefore the TD residual OF V_theta, and w is the policy-improvement direction WITH RESPECT
TO V_theta: it is biased as far as V_theta is from the closed loop's true cost-to-go (a perfect V_theta makes delta the advantage of
the explored action up to noise; a wrong one makes w chase the model's own error).  A fitted state-value baseline is not part of this
module.

``cdpg_terms`` and ``cdpg_step`` state the two kernels in torch float64 (what the tests hold them to); ``DevicePolicyGradient`` is
the learner's plant-independent part and ``CartpolePolicyGradient``, ``LinearPolicyGradient``, ``ChainPolicyGradient`` its three
plants, which reuse the Q-learners' collect launches, tables and statistics (qlearning*.py).  There is no CPU path of the learners:
the solver has none.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .qlearning import GN_KMAX, DeviceQLearning, _gn_chol_solve
from .qlearning_cartpole import CartpoleQLearning
from .qlearning_chain import ChainQLearning
from .qlearning_linear import LinearQLearning


def cdpg_msg_len(K: int) -> int:
    """The length of the message [G (K (K + 1) / 2) | b (K) | M (K (K + 1) / 2) | sum delta | count]."""
    return K * (K + 1) + K + 2


def cdpg_terms(v: torch.Tensor, u0: torch.Tensor, J: torch.Tensor, status: torch.Tensor, act: torch.Tensor, cost: torch.Tensor,
               live: torch.Tensor, gamma: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The terms of one episode in torch float64 (what mpcrl_cdpg_terms computes).  v, status, cost, live [T, E]; u0, act [T, E, nu]
    (nu = 1: [T, E] is taken too); J [T, E, nu, K], the learned columns of du0*/dp.  Term (i, e) exists for i < T - 2 and is valid when
    live[i] & live[i+1] & live[i+2] (the liveness rule of ``qlearning_td_terms``) and status[i] == 0 == status[i+1] (the roll-out
    solves').  With
        delta = (cost[i] + gamma v[i+1]) - v[i]   (three roundings, the Q-learning kernels' order),   d = act[i] - u0[i],
        psi_a = sum_c nan_to_num(J[i, e, c, a]) d_c   (c in order, one rounding per operation)
    over the valid terms (an invalid one is selected out, never multiplied by 0) returns
        msg = [G_ac = sum psi_a psi_c, a <= c, packed row-major | b_a = sum delta psi_a | M_ac = sum sum_c' J_c'a J_c'c, packed alike
               | sum delta | count],   delta [T-2, E] (0 where not valid),   valid [T-2, E] bool.
    The message is additive over environments and ranks."""
    T, E = cost.shape
    n_t = max(T - 2, 0)
    K = J.shape[-1]
    f64 = torch.float64
    u0, act = u0.to(f64).reshape(T, E, -1), act.to(f64).reshape(T, E, -1)
    nu = u0.shape[-1]
    J = J.to(f64).reshape(T, E, nu, K)
    v, cost = v.to(f64), cost.to(f64)
    lv = live.to(torch.bool)
    ok = status == 0
    valid = lv[:n_t] & lv[1:n_t + 1] & lv[2:n_t + 2] & ok[:n_t] & ok[1:n_t + 1]
    delta = cost[:n_t] + gamma * v[1:n_t + 1] - v[:n_t]
    delta = torch.where(valid, delta, torch.zeros_like(delta))              # selected: V of a failed solve may be NaN
    d = act[:n_t] - u0[:n_t]
    Jn = torch.nan_to_num(J[:n_t])
    psi = Jn[:, :, 0, :] * d[:, :, 0:1]
    for c in range(1, nu):
        psi = psi + Jn[:, :, c, :] * d[:, :, c:c + 1]
    psi = torch.where(valid[..., None], psi, torch.zeros_like(psi)).reshape(-1, K)
    Jn = torch.where(valid[..., None, None], Jn, torch.zeros_like(Jn))
    G = psi.t() @ psi
    b = psi.t() @ delta.reshape(-1)
    M = torch.zeros(K, K, dtype=f64, device=J.device)
    for c in range(nu):
        Jc = Jn[:, :, c, :].reshape(-1, K)
        M = M + Jc.t() @ Jc
    iu = torch.triu_indices(K, K, device=J.device)                          # row-major: (0, 0) .. (0, K-1), (1, 1) ..
    msg = torch.cat([G[iu[0], iu[1]], b, M[iu[0], iu[1]], delta.sum().reshape(1), valid.sum().to(f64).reshape(1)])
    return msg, delta, valid


def cdpg_step(msg: torch.Tensor, K: int, lr: float, damping: float, natural: bool, lo=None, hi=None, scale=None, radius: float = math.inf,
              theta_idx=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """The parameter step of a message in torch float64 on the CPU (what mpcrl_cdpg_apply computes before it scatters).
    n = max(1, count);  H = G/n + damping diag(G_aa/n > 0 ? G_aa/n : 1e-12 d_max), d_max = max_a G_aa/n (the rule of
    ``qlearning_gn_step``, with its codes -1 and a + 1);  w = H^-1 (b/n) by ``_gn_chol_solve``;
        step = -lr w (natural)   or   -lr (M/n) w.
    If any of ``lo``, ``hi``, ``scale`` [K] (the bounds on theta, the trust region's scales, AT THE LEARNED ENTRIES; None: -inf, +inf,
    1) or a finite ``radius`` is given, the step is clipped entrywise (a clip, not a QP) to
        [max(lo - theta_idx, -radius scale), min(hi - theta_idx, +radius scale)],   theta_idx [K]: theta at the learned entries.
    Returns (step [K], w [K], active [K] uint8: 0 inside, 1 clipped to the lower end, 2 to the upper, info): info = -1 (count 0, or d_max
    not finite or 0), -2 (an empty interval or a NaN bound, checked before the factorisation), a + 1 (pivot a is no finite number > 0),
    each with step = w = 0 and active = 0; else 0."""
    f64 = dict(dtype=torch.float64)
    msg = msg.to(torch.float64).cpu()
    if not radius > 0.0:
        raise ValueError("radius must be > 0 (inf: no trust region)")
    KK = K * (K + 1) // 2
    count = float(msg[2 * KK + K + 1])
    n = max(1.0, count)
    iu = torch.triu_indices(K, K)

    def unpack(tri):
        A = torch.zeros(K, K, **f64)
        A[iu[0], iu[1]] = tri / n
        return torch.triu(A, 1).t() + A

    H, Mb = unpack(msg[:KK]), unpack(msg[KK + K: 2 * KK + K])
    y = msg[KK: KK + K] / n
    zero, none = torch.zeros(K, **f64), torch.zeros(K, dtype=torch.uint8)
    dg = torch.diagonal(H).clone()
    d_max = float(dg.max())                                     # (torch.max propagates a NaN)
    if not count > 0.0 or not math.isfinite(d_max) or d_max == 0.0:
        return zero, zero.clone(), none, -1
    H = H + damping * torch.diag(torch.where(dg > 0.0, dg, torch.full_like(dg, 1e-12 * d_max)))
    l, u = torch.full((K,), -math.inf, **f64), torch.full((K,), math.inf, **f64)
    if lo is not None or hi is not None or scale is not None or radius < math.inf:
        vec = lambda t, fill: torch.full((K,), fill, **f64) if t is None else torch.as_tensor(t, **f64).reshape(-1).cpu()
        lo, hi, scale = vec(lo, -math.inf), vec(hi, math.inf), vec(scale, 1.0)
        th = vec(theta_idx, 0.0)
        if not (lo.numel() == hi.numel() == scale.numel() == th.numel() == K):
            raise ValueError(f"lo, hi, scale and theta_idx hold the {K} learned entries")
        t = radius * scale
        a, b = lo - th, hi - th
        l = torch.where((a > -t) | torch.isnan(a), a, -t)
        u = torch.where((b < t) | torch.isnan(b), b, t)
        if not bool((l <= u).all()):
            return zero, zero.clone(), none, -2
    fail = _gn_chol_solve(H, y)
    if fail >= 0:
        return zero, zero.clone(), none, fail + 1
    w = y
    s = w if natural else Mb @ w
    step = (-lr) * s
    active = torch.where(step < l, 1, torch.where(step > u, 2, 0)).to(torch.uint8)
    step = torch.where(active == 1, l, torch.where(active == 2, u, step))
    return step, w.clone(), active, 0


class DevicePolicyGradient(DeviceQLearning):
    """The plant-independent part of the device policy-gradient learners: the episode of ``DeviceQLearning`` without its learning
    sweep.  Per time step ONE batched roll-out solve with ``sens_pi`` over the E environments, ONE launch of mpcrl_cdpg_record (row t
    of the tables V, u0*, status and the learned columns of du0*/dp) and ONE launch of the plant's collect kernel; after T steps ONE
    launch of mpcrl_cdpg_terms (delta, validity, the message [G | b | M | sum delta | count]); with several ranks that message is
    all-reduced; then mpcrl_cdpg_apply solves for the critic's weights w and steps theta by -lr (M/n) w, or by -lr w with
    ``natural=True``.  No ``sample_mpc`` is built.

    The baseline of the TD residual is the MPC's own V_theta (the roll-out solve's), not a fitted value function: w improves the policy
    with respect to V_theta and is biased as far as V_theta is from the true cost-to-go (see the module's text).

    ``noise_scale`` must be > 0: without exploration a = pi(s), G = 0 and no step can be taken.  ``damping`` >= 0 is Marquardt's, as in
    the Q-learners' Gauss-Newton step.  At most 64 entries of theta are learned; they are read from ``learn_mask`` at the first roll-out
    step (or ``enable_graphs``) and then kept.  ``trust_radius``, ``theta_bounds`` = (lo, hi) and ``theta_scale`` ([n_p] each, defaults as
    in ``DeviceQLearning``) clip the step entrywise: theta stays in [lo, hi] and no entry moves by more than trust_radius * theta_scale_a
    per episode.  ``EpisodeStats.gn_info`` is the code of mpcrl_cdpg_apply (0 stepped, -1 no usable term, -2 an empty interval, a > 0
    pivot a failed), ``gn_active`` the clipped entries, ``td_error_mean`` the mean delta; ``w`` [K] holds the critic's weights.

    A plant's class lists this class before the plant's Q-learner: the plant's constructor, collect launch, tables and statistics are
    the Q-learner's.  (``method`` reads "gauss_newton" on these learners: the switch of ``DeviceQLearning`` for a step over
    ``learn_idx``; there is nothing to choose.)"""

    _SAMPLE = False

    def __init__(self, ocp, env, episode_length: int, lr: float, gamma, noise_scale: float, seed: int, device, group, damping: float = 1e-3,
                 natural: bool = False, learn_mask=None, trust_radius: Optional[float] = None, theta_bounds=None, theta_scale=None, **plant):
        if not isinstance(natural, bool):
            raise ValueError("natural must be a bool")
        if isinstance(noise_scale, bool) or not isinstance(noise_scale, (int, float)) or not (math.isfinite(noise_scale) and noise_scale > 0.0):
            raise ValueError("noise_scale must be finite and > 0 (without exploration G = 0 and no step can be taken)")
        if learn_mask is not None:
            learn_mask = torch.as_tensor(learn_mask).detach().to(dtype=torch.float64, device="cpu")
            if learn_mask.shape != (ocp.n_p,):
                raise ValueError(f"learn_mask must have shape [{ocp.n_p}]")
        self.natural = natural
        self.w = None                       # the critic's weights [K], from the first set-up on
        super().__init__(ocp, env, episode_length, lr=lr, gamma=gamma, noise_scale=noise_scale, seed=seed, device=device, group=group,
                         method="gauss_newton", damping=damping, trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale,
                         **plant)
        if learn_mask is not None:
            self.learn_mask.copy_((learn_mask != 0.0).to(torch.float64))

    def _gn_setup(self) -> None:
        """The learned entries, the roll-out tables and the buffers of the step, from ``learn_mask`` as it stands.  Runs once, before
        anything is captured; the buffers keep their addresses from then on."""
        if self.learn_idx is not None:
            return
        idx = torch.nonzero(self.learn_mask != 0.0).reshape(-1)
        K = int(idx.numel())
        if K < 1 or K > GN_KMAX:
            raise ValueError(f"{type(self).__name__} learns between 1 and {GN_KMAX} entries of theta; learn_mask marks {K}")
        T, E, NU, dev = self.T, self.E, self.NU, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.K = K
        self.msg = torch.zeros(cdpg_msg_len(K), **f64)
        self._ws = _lib.workspace("mpcrl_cdpg_workspace_bytes", T, E, K, device=dev)
        self.Vt = torch.zeros(T, E, **f64)
        self.U0 = torch.zeros(T, E, NU, **f64)
        self.St = torch.zeros(T, E, dtype=torch.int32, device=dev)
        self.Jt = torch.zeros(T, E, NU, K, **f64)
        self.w = torch.zeros(K, **f64)
        self.gn_active = torch.zeros(K, dtype=torch.uint8, device=dev)
        self.learn_idx = idx.to(torch.int32).contiguous()
        if self.box:
            self._box_setup(idx, K)

    @property
    def delta(self) -> torch.Tensor:
        """The TD residuals of the last episode [T - 2, E] (0 where the term is not valid)."""
        return self.td

    def _rollout_step(self):
        self._gn_setup()
        r = self.rollout_mpc.solve(self.obs, cold_mask=self.cold, sens_pi=True)     # the policy and its Jacobian, one launch
        self._call("mpcrl_cdpg_record", r.V, r.u0, r.dpi_dp, r.status, self.row, self.learn_idx, self.E, self.T, self.NU, self.n_p, self.K,
                   self.Vt, self.U0, self.St, self.Jt)
        self._collect(r)
        return r

    def _sweep(self):
        """No sweep: the terms of the episode's own roll-out solves, one launch."""
        self._gn_setup()
        self._call("mpcrl_cdpg_terms", self.Vt, self.U0, self.Jt, self.St, self.A, self.C, self.live, self.T, self.E, self.NU, self.K,
                   self.gamma, self._ws, self.td, self.valid, self.msg)
        return None

    def _apply(self) -> None:
        lo, hi, scale = (self.theta_lo, self.theta_hi, self.theta_scale) if self.box else (None, None, None)
        self._call("mpcrl_cdpg_apply", self.msg, self.K, self.learn_idx, self.n_p, self.lr, self.damping, int(self.natural), lo, hi, scale,
                   self.trust_radius, self.theta, self.step_out, self.w, self.gn_active, self.gn_info)
        self._set_theta()


class LinearPolicyGradient(DevicePolicyGradient, LinearQLearning):
    """``DevicePolicyGradient`` on the linear system (the plant, tables and statistics of ``LinearQLearning``).  ``gamma=None`` takes the
    OCP's discount factor; the handle is set to it.  All of theta is learned unless ``learn_mask`` [n_p] says otherwise."""

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-2, gamma: Optional[float] = None, noise_scale: float = 0.1, seed: int = 0,
                 device=None, group=None, damping: float = 1e-3, natural: bool = False, learn_mask=None, trust_radius: Optional[float] = None,
                 theta_bounds=None, theta_scale=None):
        super().__init__(ocp, env, episode_length, lr, gamma, noise_scale, seed, device, group, damping=damping, natural=natural,
                         learn_mask=learn_mask, trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale)


class CartpolePolicyGradient(DevicePolicyGradient, CartpoleQLearning):
    """``DevicePolicyGradient`` on the cartpole (the plant, tables, liveness and statistics of ``CartpoleQLearning``).  The MPC keeps the
    OCP's own discount factor; ``gamma`` is the TD discount.  (M, m, l) are learned unless ``learn_mask`` [n_p] says otherwise."""

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-2, gamma: float = 0.99, noise_scale: float = 0.1, seed: int = 0,
                 device=None, group=None, damping: float = 1e-3, natural: bool = False, learn_mask=None, trust_radius: Optional[float] = None,
                 theta_bounds=None, theta_scale=None):
        super().__init__(ocp, env, episode_length, lr, gamma, noise_scale, seed, device, group, damping=damping, natural=natural,
                         learn_mask=learn_mask, trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale)


class ChainPolicyGradient(DevicePolicyGradient, ChainQLearning):
    """``DevicePolicyGradient`` on the chain of masses (the plant, tables and statistics of ``ChainQLearning``), three controls.
    ``learn``: the blocks of theta that are learned (``ChainQLearning``; at most 64 entries: m, D, L, C are 20 at n_mass 3 and 40 at
    n_mass 5).  ``chain_theta_bounds(ocp)`` keeps the masses and spring constants positive."""

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-2, gamma: Optional[float] = None, noise_scale: float = 0.05, seed: int = 0,
                 device=None, group=None, damping: float = 1e-3, natural: bool = False, learn: Sequence[str] = ("m", "D", "L", "C"),
                 trust_radius: Optional[float] = None, theta_bounds=None, theta_scale=None):
        super().__init__(ocp, env, episode_length, lr, gamma, noise_scale, seed, device, group, damping=damping, natural=natural,
                         trust_radius=trust_radius, theta_bounds=theta_bounds, theta_scale=theta_scale, learn=learn)

    def workspace_bytes(self) -> Tuple[int, int]:
        """Bytes of device memory of the roll-out handle; there is no sweep handle (0)."""
        return self.rollout_mpc.workspace_bytes(), 0
