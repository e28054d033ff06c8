"""Batched MPC Q-learning: the reference's documented use of the hot path, with the per-sample loops turned into batches.

rlmpc/examples/linear_system_mpc_qlearning.py:153-205 per episode:
    roll out EPISODE_LENGTH steps with  a = mpc.get_action(s)                          (160-167)
    for every stored sample i:  mpc.q_update(s_i, a_i) -> Q_i, dQ/dp_i ;  mpc.update(s_i) -> V_i      (178-190)
    td_i = cost_i + gamma * V_{i+1} - Q_i                                               (193)
    p   += mean_i( LR * td_i * dQ/dp_i )                                                (203-205)
The samples of an episode are independent given p, and so are parallel environments: here the roll-out is ONE
``MPCBatch.solve`` per time step over E environments and the learning sweep is TWO batched solves over all E*T samples.
With several ranks every rank learns from its own environments and the parameter step is all-reduced
(mpc4rl_amd.distributed), so all ranks hold identical parameters.

``BatchedQLearning`` is that loop in torch for any model.  ``DeviceQLearning`` is the core of its device forms (``CartpoleQLearning``,
``LinearQLearning``, ``ChainQLearning``): everything of an episode but the plant's own roll-out kernel and tables.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

from . import _lib
from .batch import MPCBatch
from .distributed import mean_update


@dataclass
class EpisodeStats:
    total_cost: float
    td_error_mean: float
    step: torch.Tensor          # parameter step that was applied
    converged_fraction: float
    gn_info: int = 0            # method="gauss_newton": info of mpcrl_qlearning_gn_apply (0 stepped, -1 no usable term, a > 0 pivot a failed)
    gn_active: int = 0          # with bounds or a trust region: the entries of the step that sit on a bound ...
    gn_iterations: int = 0      # ... and the active-set iterations of mpcrl_qlearning_gn_apply_box (gn_info -2: empty box, -3: iteration cap)


GN_KMAX = 64                    # the cap on the learned entries of the Gauss-Newton step (GN_KMAX of csrc/qlearning_gn_kernel.hpp)
METHODS = ("gradient", "gauss_newton")


def gn_msg_len(K: int) -> int:
    """The length of the Gauss-Newton message [G (upper triangle, K (K + 1) / 2) | b (K) | sum td | count]."""
    return K * (K + 1) // 2 + K + 2


def qlearning_gn_terms(q: torch.Tensor, v: torch.Tensor, dq: torch.Tensor, status_q: torch.Tensor, status_v: torch.Tensor, cost: torch.Tensor,
                       live: torch.Tensor, gamma: float, idx) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The TD terms and Gauss-Newton sums of one episode in torch float64 (what mpcrl_qlearning_td_gn computes).  The arguments, the terms,
    ``td`` and ``valid`` are those of ``qlearning_td_terms``; ``idx`` [K]: the learned columns of dq, strictly increasing.  With
    g = nan_to_num(dq[..., idx]) over the valid terms (an invalid one is selected out) returns
        msg = [G_ac = sum g_a g_c, a <= c, packed row-major | b_a = sum td g_a | sum td | count],  td [T-2, E],  valid [T-2, E] bool."""
    from .qlearning_cartpole import qlearning_td_terms       # (that module imports this one)
    _, td, valid = qlearning_td_terms(q, v, dq, status_q, status_v, cost, live, gamma, 0.0)
    idx = torch.as_tensor(idx, dtype=torch.int64, device=dq.device).reshape(-1)
    K, n_t = idx.numel(), td.shape[0]
    g = torch.nan_to_num(dq[:n_t].to(torch.float64)[..., idx])
    g = torch.where(valid[..., None], g, torch.zeros_like(g)).reshape(-1, K)
    G = g.t() @ g
    b = g.t() @ td.reshape(-1).to(torch.float64)
    iu = torch.triu_indices(K, K, device=dq.device)            # row-major: (0, 0) .. (0, K-1), (1, 1) ..
    msg = torch.cat([G[iu[0], iu[1]], b, td.sum().reshape(1).to(torch.float64), valid.sum().to(torch.float64).reshape(1)])
    return msg, td, valid


def qlearning_gn_step(msg: torch.Tensor, K: int, lr: float, damping: float) -> Tuple[torch.Tensor, int]:
    """The damped Gauss-Newton step of a message in torch float64 (what mpcrl_qlearning_gn_apply computes before it scatters):
    n = max(1, count), Gb = G / n, bb = b / n, d_max = max_a Gb_aa;  H = Gb + damping diag(Gb_aa > 0 ? Gb_aa : 1e-12 d_max) (Marquardt's
    scaling: the step is covariant under a diagonal rescaling of the parameters for any damping; the floor is for an entry no term is
    sensitive to, whose step is 0 whatever it is);  delta = lr H^-1 bb by a Cholesky factorisation.
    Returns (delta [K], info): info = -1 (count 0, or d_max not finite or 0) or a + 1 (pivot a is no finite number > 0) with delta = 0,
    else 0."""
    msg = msg.to(torch.float64)
    KK = K * (K + 1) // 2
    count = float(msg[KK + K + 1])
    n = max(1.0, count)
    iu = torch.triu_indices(K, K, device=msg.device)
    H = torch.zeros(K, K, dtype=torch.float64, device=msg.device)
    H[iu[0], iu[1]] = msg[:KK] / n
    H = torch.triu(H, 1).t() + H
    y = msg[KK: KK + K] / n
    zero = torch.zeros(K, dtype=torch.float64, device=msg.device)
    d = torch.diagonal(H).clone()
    d_max = float(d.max())                                      # (torch.max propagates a NaN)
    if not count > 0.0 or not math.isfinite(d_max) or d_max == 0.0:
        return zero, -1
    H = H + damping * torch.diag(torch.where(d > 0.0, d, torch.full_like(d, 1e-12 * d_max)))
    fail = _gn_chol_solve(H, y)
    if fail >= 0:
        return zero, fail + 1
    return lr * y, 0


def _gn_chol_solve(H: torch.Tensor, y: torch.Tensor) -> int:
    """gn_chol_solve of csrc/qlearning_gn_kernel.hpp: the Cholesky factorisation H = L L' in place (right-looking, a column at a time,
    the kernel's order), then y <- H^-1 y.  Returns -1, or the index of the first pivot that is no finite number > 0 (H and y are then
    left half done)."""
    K = H.shape[0]
    for k in range(K):
        piv = float(H[k, k])
        if not (math.isfinite(piv) and piv > 0.0):
            return k
        l = math.sqrt(piv)
        H[k, k] = l
        H[k + 1:, k] = H[k + 1:, k] / l
        H[k + 1:, k + 1:] -= torch.outer(H[k + 1:, k], H[k + 1:, k])
    for k in range(K):
        y[k] = y[k] / H[k, k]
        y[k + 1:] -= H[k + 1:, k] * y[k]
    for k in range(K - 1, -1, -1):
        y[k] = y[k] / H[k, k]
        y[:k] -= H[k, :k] * y[k]
    return -1


def gn_box_iteration_cap(K: int) -> int:
    """The cap on the active-set iterations of the box-constrained Gauss-Newton step (gn_box_iteration_cap of
    csrc/qlearning_gn_kernel.hpp, where it is explained)."""
    return 8 * K + 16


def qlearning_gn_box_step(msg: torch.Tensor, K: int, lr: float, damping: float, lo: torch.Tensor, hi: torch.Tensor, scale: torch.Tensor,
                          radius: float, theta_idx: torch.Tensor, with_iterations: bool = False):
    """The Gauss-Newton step of a message inside a box and a per-entry trust region, in torch float64 on the CPU (what
    mpcrl_qlearning_gn_apply_box computes before it scatters; the only CPU path).  With H and bb of ``qlearning_gn_step``,
        delta = argmin 1/2 d' H d - lr bb' d   subject to  l <= d <= u,
        l_a = max(lo_a - theta_a, -radius scale_a),  u_a = min(hi_a - theta_a, +radius scale_a)
    where ``lo``, ``hi``, ``scale`` and ``theta_idx`` [K] are the bounds, the trust region's scales and theta AT THE LEARNED ENTRIES
    (``lo[idx]`` ...); lo, hi may be -+inf, radius +inf.  A strictly convex box QP, solved exactly by a primal active-set method:
      x = clamp(0, l, u), the entries that start on a bound are active (1 at l, 2 at u); H is factored whole first (its pivot codes);
      every iteration solves the free block, H_FF z = lr bb_F - H_FB x_B, by ``_gn_chol_solve``;
      if some z_a leaves [l_a, u_a], x moves towards z up to the first blocking bound (lowest entry on a tie), which it takes exactly
      and which becomes active;
      else x_F = z, and with the multipliers r = H x - lr bb the active entry with l_a < u_a whose r_a has the wrong sign by more than
      tol_a / 2, tol_a = 4 (3 K + 1) eps (sum_c sqrt(H_aa H_cc) |x_c| + lr |bb_a|) (the backward error of the solve: a multiplier
      below it is rounding), and the largest such r_a / sqrt(H_aa) (covariant under a rescaling of the parameters) is released; none: done.
    An entry with l_a = u_a is reported at 1 or 2 by the sign of its multiplier.
    Returns (delta [K], active [K] uint8, info): info = -1 (no usable term), -2 (l_a > u_a, or a bound that is NaN, for some a), -3 (the
    iteration cap), a + 1 (a pivot of entry a is no finite number > 0), each with delta = 0 and active = 0; else 0.
    ``with_iterations``: also returns the number of free-block solves."""
    def out(delta, active, info, it):
        return (delta, active, info, it) if with_iterations else (delta, active, info)

    msg = msg.to(torch.float64).cpu()
    f64 = dict(dtype=torch.float64)
    lo, hi, scale, th = (torch.as_tensor(t, **f64).reshape(-1).cpu() for t in (lo, hi, scale, theta_idx))
    if not (lo.numel() == hi.numel() == scale.numel() == th.numel() == K):
        raise ValueError(f"lo, hi, scale and theta_idx hold the {K} learned entries")
    if not radius > 0.0:
        raise ValueError("radius must be > 0 (inf: no trust region)")
    KK = K * (K + 1) // 2
    count = float(msg[KK + K + 1])
    n = max(1.0, count)
    iu = torch.triu_indices(K, K)
    H = torch.zeros(K, K, **f64)
    H[iu[0], iu[1]] = msg[:KK] / n
    H = torch.triu(H, 1).t() + H
    g = lr * (msg[KK: KK + K] / n)
    zero, none = torch.zeros(K, **f64), torch.zeros(K, dtype=torch.uint8)
    d = torch.diagonal(H).clone()
    d_max = float(d.max())
    if not count > 0.0 or not math.isfinite(d_max) or d_max == 0.0:
        return out(zero, none, -1, 0)
    H = H + damping * torch.diag(torch.where(d > 0.0, d, torch.full_like(d, 1e-12 * d_max)))
    t = radius * scale
    a, b = lo - th, hi - th
    l = torch.where((a > -t) | torch.isnan(a), a, -t)
    u = torch.where((b < t) | torch.isnan(b), b, t)
    if not bool((l <= u).all()):
        return out(zero, none, -2, 0)
    x = torch.where(l > 0.0, l, torch.where(u < 0.0, u, zero))
    st = torch.where(x == l, 1, torch.where(x == u, 2, 0))
    x = torch.where(st == 1, l, torch.where(st == 2, u, x))
    L, z = H.clone(), g.clone()
    fail = _gn_chol_solve(L, z)                                     # the whole of H first: its pivots' codes
    if fail >= 0:
        return out(zero, none, fail + 1, 0)
    hd = torch.diagonal(H)
    root = torch.sqrt(hd)
    it, cap, first = 0, gn_box_iteration_cap(K), True
    while True:
        F = torch.nonzero(st == 0).reshape(-1)
        B = torch.nonzero(st != 0).reshape(-1)
        if it == cap:
            return out(zero, none, -3, it)
        it += 1
        if not (first and F.numel() == K):                          # (else the factorisation above is this iteration's)
            z = g[F] - H[F][:, B] @ x[B]
            L = H[F][:, F].clone()
            fail = _gn_chol_solve(L, z)
            if fail >= 0:
                return out(zero, none, int(F[fail]) + 1, it)
        first = False
        xf, lf, uf = x[F], l[F], u[F]
        inf = torch.full_like(z, math.inf)
        alpha = torch.where(z > uf, (uf - xf) / (z - xf), torch.where(z < lf, (lf - xf) / (z - xf), inf))
        if F.numel() > 0 and float(alpha.min()) < math.inf:
            p = int(torch.argmax((alpha == alpha.min()).to(torch.int8)))    # the lowest entry on a tie
            al = float(alpha[p])
            xn = torch.minimum(torch.maximum(xf + al * (z - xf), lf), uf)
            side = 2 if float(z[p]) > float(uf[p]) else 1
            xn[p] = uf[p] if side == 2 else lf[p]
            x[F] = xn
            st[F[p]] = side
            continue
        x[F] = z
        r = H @ x - g
        tol = 4.0 * (3 * K + 1) * 2.0 ** -53 * (root * (root @ x.abs()) + g.abs())
        v = torch.where(st == 1, -r, r)
        cand = (st != 0) & (l < u) & (v > 0.5 * tol)
        if not bool(cand.any()):
            break
        score = torch.where(cand, v / root, torch.full_like(v, -math.inf))
        st[int(torch.argmax((score == score.max()).to(torch.int8)))] = 0
    st = torch.where(l == u, torch.where(r >= 0.0, 1, 2), st)
    return out(x, st.to(torch.uint8), 0, it)


class BatchedQLearning:
    """Q-learning of the MPC parameters with E parallel environments and episodes of T steps.

    ``rollout_mpc`` solves E instances (policy), ``sample_mpc`` solves E*(T-1) instances (Q and V of every transition)."""

    def __init__(self, ocp, env, episode_length: int, lr: float = 1e-4, gamma: Optional[float] = None,
                 scale_action: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 unscale_action: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, device=None, group=None):
        self.ocp, self.env, self.T, self.lr = ocp, env, episode_length, lr
        self.gamma = ocp.gamma if gamma is None else gamma
        self.E = env.num_envs
        self.rollout_mpc = MPCBatch(ocp, self.E, device)
        self.sample_mpc = MPCBatch(ocp, self.E * (episode_length - 1), device)
        for m in (self.rollout_mpc, self.sample_mpc):
            m.set_discount_factor(self.gamma)
        self.theta = torch.as_tensor(ocp.p0, dtype=torch.float64, device=self.rollout_mpc.device).clone()
        self.scale_action = scale_action or (lambda u: u)
        self.unscale_action = unscale_action or (lambda a: a)
        self.group = group
        self.last_episode = None

    def run_episode(self) -> EpisodeStats:
        dev = self.rollout_mpc.device
        obs = self.env.reset().to(dev)
        self.rollout_mpc.reset()
        S, A, C = [], [], []
        for _ in range(self.T):
            u = self.rollout_mpc.get_action(obs)                  # [E, nu], one launch (mpc.get_action, 160-161)
            a = self.scale_action(u)
            nxt, cost, _, _ = self.env.step(a.to(self.env.device))
            S.append(obs), A.append(u), C.append(cost.to(dev))
            obs = nxt.to(dev)
        S, A, C = torch.stack(S), torch.stack(A), torch.stack(C)      # [T, E, .]
        self.last_episode = (S, A, C)                                 # the replay buffer of the reference loop (168-172)
        n = self.T - 1                                                # replay_buffer.size() - 1 samples (172)
        s = S[:n].reshape(n * self.E, -1)
        a = A[:n].reshape(n * self.E, -1)
        self.sample_mpc.reset()
        rq = self.sample_mpc.solve(s, u0=a, sens_v=True, cold=True)   # Q(s_i, a_i), dQ/dp_i   (q_update, 181-187)
        rv = self.sample_mpc.solve(s, cold=True)                      # V(s_i)               (update, 189-190)
        ok = ((rq.status == 0) & (rv.status == 0)).reshape(n, self.E)
        q, v = rq.V.reshape(n, self.E), rv.V.reshape(n, self.E)
        dq = rq.dV_dp.reshape(n, self.E, -1)
        td = C[: n - 1] + self.gamma * v[1:] - q[:-1]                 # (193)
        okb = ok[:-1] & ok[1:]
        valid = okb.to(td.dtype)
        # failed samples are SELECTED out (their V / Q may be NaN, and NaN * 0 = NaN)
        w = (self.lr * torch.where(okb, td, torch.zeros_like(td))).reshape(-1)
        g = dq[: n - 1].reshape(-1, dq.shape[-1])
        g = torch.where(okb.reshape(-1, 1), torch.nan_to_num(g), torch.zeros_like(g))
        step = mean_update(g, w, self.group, valid=valid.reshape(-1))   # mean_i(LR * td_i * dQ/dp_i) over the valid samples of all ranks (203)
        self.theta = self.theta + step
        for m in (self.rollout_mpc, self.sample_mpc):
            m.set_theta(self.theta)                                   # mpc.set_parameter (204-205)
        return EpisodeStats(float(C.sum().item()) / self.E, float(torch.where(okb, td, torch.zeros_like(td)).sum().item() / max(1.0, float(valid.sum().item()))), step, float(valid.mean().item()))


class DeviceQLearning:
    """The plant-independent part of the device Q-learners.  Per time step the roll-out is ONE batched solve over the E environments
    (warm, an episode's first solve cold per instance through the cold mask) and ONE launch of the plant's collect kernel; the learning
    sweep is ONE batched Q solve over all E (T - 1) samples (u0 fixed to the recorded actions, dQ/dp, cold), ONE V solve started from
    the Q solve's primal iterate and ONE launch of mpcrl_qlearning_td_grad (TD errors, validity, and the message [sum lr td dQ/dp,
    sum lr td, count] of distributed.mean_update).  With several ranks only that message is all-reduced; then mpcrl_qlearning_apply
    takes the mean and steps theta.

    ``method="gauss_newton"`` replaces that first-order step by the least-squares TD step over the entries ``learn_mask`` marks,
    delta = lr (G/n + damping diag(G/n))^-1 (b/n) with G = sum g g', b = sum td g, g = dQ/dp on those entries: mpcrl_qlearning_td_gn in
    the sweep (the message [G | b | sum td | count], additive: still one collective) and mpcrl_qlearning_gn_apply after it.  The step is
    covariant under a rescaling of the parameters, so ``lr`` in (0, 1] means the same on every model; ``damping`` >= 0 is Marquardt's.  At
    most 64 entries can be learned that way (the factorisation is one workgroup's, in LDS).  The entries are read from ``learn_mask`` at
    the first sweep (or ``enable_graphs``) and kept.  ``EpisodeStats.gn_info`` reports a step that was not taken.

    ``trust_radius``, ``theta_bounds`` = (lo, hi) and ``theta_scale`` (each [n_p]; gauss_newton only) make that step the box QP of
    ``qlearning_gn_box_step``: theta stays in [lo, hi] (-+inf: no bound) and no entry moves by more than trust_radius * theta_scale_a in
    one episode, solved exactly by mpcrl_qlearning_gn_apply_box in one launch.  ``theta_scale`` defaults to |p0_a|, where that is 0 to the
    largest |p0_c| over the learned entries, and to 1 if those are all 0.  With all three None the plain step runs, bit for bit as before.
    ``EpisodeStats.gn_active`` counts the entries on a bound, ``gn_iterations`` the active-set iterations.

    A plant's class sets ``NX`` and, with more than one control, ``NU``, checks its OCP and environment, allocates
    ``live`` [T, E] (and what else its collect kernel needs) after this constructor, and defines ``_collect(r)`` (the collect launch
    after the roll-out solve r, through ``self._call``), ``_stats()``, where the environment carries more than its state from step to step
    ``_env_carried()``, and, where the zero state is no state of the plant, ``_initial_obs()``.

    ``NU`` = 1: ``A`` and ``eps`` are [T, E] and the control bounds the floats ``lo``, ``hi``.  ``NU`` > 1: ``A`` and ``eps`` are
    [T, E, NU] and the bounds the host arrays ``lo_v``, ``hi_v`` (ctypes doubles, what a collect export takes)."""

    NX: int = 0             # the state's width
    NU: int = 1             # the number of controls
    _SAMPLE: bool = True    # False: a learner without a learning sweep (policy_gradient.py) builds no ``sample_mpc`` and no TD workspace

    def __init__(self, ocp, env, episode_length: int, lr: float, gamma: float, noise_scale: float, seed: int, device, group,
                 mpc_gamma: Optional[float] = None, method: str = "gradient", damping: float = 1e-3, trust_radius: Optional[float] = None,
                 theta_bounds: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, theta_scale: Optional[torch.Tensor] = None):
        name = type(self).__name__
        if method not in METHODS:
            raise ValueError(f"method: unknown {method!r} (one of {', '.join(METHODS)})")
        if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not (math.isfinite(damping) and damping >= 0.0):
            raise ValueError("damping must be finite and >= 0")
        box = trust_radius is not None or theta_bounds is not None or theta_scale is not None
        if box and method != "gauss_newton":
            raise ValueError("trust_radius, theta_bounds and theta_scale belong to method='gauss_newton' (no projected first-order step)")
        if trust_radius is not None and (isinstance(trust_radius, bool) or not isinstance(trust_radius, (int, float)) or not trust_radius > 0.0):
            raise ValueError("trust_radius must be > 0 (None or inf: no trust region)")
        f64c = dict(dtype=torch.float64, device="cpu")
        if theta_bounds is not None:
            if not isinstance(theta_bounds, (tuple, list)) or len(theta_bounds) != 2:
                raise ValueError("theta_bounds is a pair (lo, hi)")
            theta_bounds = tuple(torch.as_tensor(t).detach().to(**f64c) for t in theta_bounds)
            if any(t.shape != (ocp.n_p,) for t in theta_bounds):
                raise ValueError(f"theta_bounds: lo and hi must have shape [{ocp.n_p}]")
            if not bool((theta_bounds[0] <= theta_bounds[1]).all()):
                raise ValueError("theta_bounds: lo <= hi must hold for every entry (and neither may be NaN)")
        if theta_scale is not None:
            theta_scale = torch.as_tensor(theta_scale).detach().to(**f64c)
            if theta_scale.shape != (ocp.n_p,):
                raise ValueError(f"theta_scale must have shape [{ocp.n_p}]")
            if not bool((torch.isfinite(theta_scale) & (theta_scale > 0.0)).all()):
                raise ValueError("theta_scale must be finite and > 0")
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
            raise RuntimeError(f"{name} runs on a HIP device (the environment's state too); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if env.device.index is not None and env.device != dev:
            raise ValueError("the environment must live on the learner's device (its state is updated in place by the library)")
        self.ocp, self.env, self.T, self.lr, self.gamma, self.noise_scale = ocp, env, episode_length, float(lr), float(gamma), float(noise_scale)
        self.E, self.device, self.group = env.num_envs, dev, group
        self.method, self.damping = method, float(damping)
        self.learn_idx = None               # gauss_newton: the learned entries [K] int32, built from learn_mask at the first sweep
        self.gn_info = torch.zeros(2, dtype=torch.int32, device=dev)      # [code, iterations of the box step]
        self.box = box
        self.trust_radius = math.inf if trust_radius is None else float(trust_radius)
        self._box_args = (theta_bounds, theta_scale)                        # as given (CPU), until _gn_setup puts them on the device
        T, E, NX, NU = self.T, self.E, self.NX, self.NU
        if ocp.nu != NU:
            raise ValueError(f"{name} is written for {NU} control(s), the OCP has {ocp.nu}")
        wide = () if NU == 1 else (NU,)      # one control: the tables keep no control axis
        self.rollout_mpc = MPCBatch(ocp, E, dev)
        if self._SAMPLE:
            self.sample_mpc = MPCBatch(ocp, E * (T - 1), dev)
        if mpc_gamma is not None:           # the handles' own discount factor (else the OCP's)
            for m in self._handles():
                m.set_discount_factor(mpc_gamma)
        self.n_p = ocp.n_p
        f64 = dict(dtype=torch.float64, device=dev)
        self.theta = torch.as_tensor(ocp.p0, **f64).clone()            # updated in place (the handles copy it after every step)
        self.learn_mask = torch.zeros_like(self.theta)
        self.learn_mask[: ocp.n_model_p] = 1.0                          # the model's parameters
        if NU == 1:
            self.lo, self.hi = float(ocp.lbu[0]), float(ocp.ubu[0])
        else:
            import ctypes
            self.lo_v, self.hi_v = (ctypes.c_double * NU)(*map(float, ocp.lbu)), (ctypes.c_double * NU)(*map(float, ocp.ubu))
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        # the episode's device state: every buffer keeps its address (captured graphs hold them)
        self.obs = torch.zeros(E, NX, **f64)
        self.row = torch.zeros(E, dtype=torch.int32, device=dev)
        self.cold = torch.ones(E, dtype=torch.int32, device=dev)
        self.eps = torch.zeros(T, E, *wide, dtype=torch.float32, device=dev)
        self.S = torch.zeros(T, E, NX, **f64)
        self.A = torch.zeros(T, E, *wide, **f64)
        self.C = torch.zeros(T, E, **f64)
        self.td = torch.zeros(T - 2, E, **f64)
        self.valid = torch.zeros(T - 2, E, dtype=torch.uint8, device=dev)
        self.msg = torch.zeros(self.n_p + 2, **f64)
        self.step_out = torch.zeros(self.n_p, **f64)
        if self._SAMPLE:
            self._td_ws = _lib.workspace("mpcrl_qlearning_td_workspace_bytes", T, E, self.n_p, device=dev)
        # the roll-out handle holds an iterate from here on, so that the first solve of every episode (eager or replayed) is the
        # per-instance cold start of the cold mask, never the handle-wide one of a fresh handle
        x_init = self._initial_obs()
        if x_init is not None:              # else the zero state, as the buffers are allocated
            x_init = torch.as_tensor(x_init, **f64)
            self.obs.copy_(x_init.expand_as(self.obs))
            self.S.copy_(x_init.expand_as(self.S))
        self.rollout_mpc.solve(self.obs, cold=True)
        self._graphs = None
        self.last = None                # the roll-out solves of the last eager episode, one SolveResult per step
        self.last_sweep = None          # (Q solve, V solve) of the last episode's learning sweep
        self.episodes = 0

    # ------------------------------------------------------------------ pieces (the same launches eager and captured)
    def _call(self, name: str, *args) -> int:
        return _lib.call(name, *args, device=self.device)

    def _handles(self):
        return (self.rollout_mpc, self.sample_mpc) if self._SAMPLE else (self.rollout_mpc,)

    def _start_episode(self, x0: Optional[torch.Tensor] = None) -> None:
        self.env.reset()
        if x0 is not None:
            self.env.state.copy_(torch.as_tensor(x0, dtype=torch.float64, device=self.device).reshape(self.E, self.NX))
        self.obs.copy_(self.env.state)
        self.row.zero_()
        self.cold.fill_(1)
        torch.randn(*self.eps.shape, generator=self.gen, dtype=torch.float32, device=self.device, out=self.eps)

    def _rollout_step(self):
        r = self.rollout_mpc.solve(self.obs, cold_mask=self.cold)           # the policy of every environment (mpc.get_action), one launch
        self._collect(r)
        return r

    def _gn_setup(self) -> None:
        """The learned entries and the buffers of the Gauss-Newton step, from ``learn_mask`` as it stands (a plant's class sets it after
        this constructor).  Runs once, before anything is captured; the buffers keep their addresses from then on."""
        if self.learn_idx is not None:
            return
        idx = torch.nonzero(self.learn_mask != 0.0).reshape(-1)
        K = int(idx.numel())
        if K < 1 or K > GN_KMAX:
            raise ValueError(f"method='gauss_newton' learns between 1 and {GN_KMAX} entries of theta; learn_mask marks {K}")
        self.K = K
        self.msg = torch.zeros(gn_msg_len(K), dtype=torch.float64, device=self.device)
        self._gn_ws = _lib.workspace("mpcrl_qlearning_gn_workspace_bytes", self.T, self.E, K, device=self.device)
        self.learn_idx = idx.to(torch.int32).contiguous()
        if self.box:
            self._box_setup(idx, K)

    def _box_setup(self, idx: torch.Tensor, K: int) -> None:
        """The bounds and the trust region's scales on the device, from the constructor's arguments and their defaults."""
        f64 = dict(dtype=torch.float64, device=self.device)
        bounds, scale = self._box_args
        if bounds is None:
            bounds = (torch.full((self.n_p,), -math.inf), torch.full((self.n_p,), math.inf))
        if scale is None:       # |p0_a|; where that is 0 the largest |p0_c| of the learned entries; 1 if those are all 0
            p0 = torch.as_tensor(self.ocp.p0, dtype=torch.float64).abs()
            top = float(p0[idx.cpu()].max())
            scale = torch.where(p0 != 0.0, p0, torch.full_like(p0, top if top > 0.0 else 1.0))
        self.theta_lo, self.theta_hi, self.theta_scale = bounds[0].to(**f64), bounds[1].to(**f64), scale.to(**f64)
        self.gn_active = torch.zeros(K, dtype=torch.uint8, device=self.device)

    def _sweep(self):
        if self.method == "gauss_newton":
            self._gn_setup()
        n = self.T - 1
        s = self.S[:n].reshape(n * self.E, self.NX)
        a = self.A[:n].reshape(n * self.E, self.NU)
        # q_update: Q(s_i, a_i), dQ/dp_i; its bound multipliers are not kept (store_bounds=False) ...
        rq = self.sample_mpc.solve(s, u0=a, sens_v=True, cold=True, store_bounds=False)
        # ... update: V(s_i) from the Q solve's primal iterate, interior point from its default point
        rv = self.sample_mpc.solve(s)
        if self.method == "gauss_newton":
            self._call("mpcrl_qlearning_td_gn", rq.V, rv.V, rq.dV_dp, rq.status, rv.status, self.C, self.live, self.T, self.E, self.n_p,
                       self.gamma, self.learn_idx, self.K, self._gn_ws, self.td, self.valid, self.msg)
        else:
            self._call("mpcrl_qlearning_td_grad", rq.V, rv.V, rq.dV_dp, rq.status, rv.status, self.C, self.live, self.T, self.E, self.n_p,
                       self.gamma, self.lr, self._td_ws, self.td, self.valid, self.msg)
        return rq, rv

    def _allreduce(self) -> None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and (self.group is not None or dist.get_world_size() > 1):
            dist.all_reduce(self.msg, op=dist.ReduceOp.SUM, group=self.group)

    def _apply(self) -> None:
        if self.method == "gauss_newton" and self.box:
            self._call("mpcrl_qlearning_gn_apply_box", self.msg, self.K, self.learn_idx, self.n_p, self.lr, self.damping, self.theta_lo,
                       self.theta_hi, self.theta_scale, self.trust_radius, self.theta, self.step_out, self.gn_active, self.gn_info)
        elif self.method == "gauss_newton":
            self._call("mpcrl_qlearning_gn_apply", self.msg, self.K, self.learn_idx, self.n_p, self.lr, self.damping, self.theta,
                       self.step_out, self.gn_info)
        else:
            self._call("mpcrl_qlearning_apply", self.msg, self.n_p, self.learn_mask, self.theta, self.step_out)
        self._set_theta()

    def _set_theta(self) -> None:
        for m in self._handles():
            m.set_theta(self.theta)                                    # mpc.set_parameter

    def _initial_obs(self):
        """The state [NX] that ``obs`` and the rows of ``S`` hold before the first episode: what the constructor's priming solve and the
        warm-up of enable_graphs solve on.  None: zeros."""
        return None

    def _env_carried(self):
        """The environment's tensors that a roll-out step changes (put back after the warm-up of enable_graphs)."""
        return [self.env.state]

    # ------------------------------------------------------------------ the episode
    def run_episode(self, x0: Optional[torch.Tensor] = None) -> EpisodeStats:
        """One episode of all E environments, its learning sweep and the parameter step.  x0 [E, NX]: the initial states, instead of
        what the environment's reset gives (which is taken all the same, so the environment's generator advances alike)."""
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
        stats = self._stats()
        if self.method == "gauss_newton":
            info = self.gn_info.tolist()
            stats.gn_info = info[0]
            if self.box:
                stats.gn_iterations, stats.gn_active = info[1], int((self.gn_active != 0).sum().item())
        return stats

    # ------------------------------------------------------------------ HIP graphs
    def enable_graphs(self) -> None:
        """Captures one roll-out step (solve + collect; replayed T times per episode) and the learning sweep (Q solve, V solve, TD kernel)
        as two HIP graphs.  The episode start, the collective and the apply stay eager calls, so episodes are bit-identical to the eager
        ones.  A warm-up of both pieces runs first on the capture stream (lazy initialisation, the solves' launch shape); the
        environment's state is put back afterwards, and nothing else the learner carries from one episode to the next is touched by it."""
        if self._graphs is not None:
            return
        if self.method == "gauss_newton":
            self._gn_setup()
        dev = self.device
        snap = [t.clone() for t in self._env_carried()]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._rollout_step()
            self._sweep()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        for t, s in zip(self._env_carried(), snap):
            t.copy_(s)
        torch.cuda.synchronize(dev)
        g_roll, g_sweep = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_roll, stream=side):
            self._rollout_step()
        with torch.cuda.graph(g_sweep, stream=side):
            out = self._sweep()
        torch.cuda.synchronize(dev)
        self._graphs = {"rollout": g_roll, "sweep": g_sweep, "sweep_out": out}
