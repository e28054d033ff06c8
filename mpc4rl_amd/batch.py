"""MPCBatch — the batched extension of the reference's MPC surface: B OCP instances per call.

``rlmpc.td3.policies.Actor.forward`` loops ``mpc.get_action`` over the observation batch in Python
(rlmpc/td3/policies.py:186-197) and the Q-learning example loops ``q_update``/``update`` over replay samples
(rlmpc/examples/linear_system_mpc_qlearning.py:178-190).  Here each of those loops is ONE call that issues one
kernel launch through the C ABI (include/mpcrl.h); inputs and outputs are torch tensors on the GPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr      # noqa: F401  (tests and profiles/microbench call the library directly with it)
from .problems import OcpDescription, chain_param_layout


@dataclass
class SolveResult:
    u0: torch.Tensor                 # [B, nu]   u_0*
    V: torch.Tensor                  # [B]       optimal cost (V, or Q when u0 was fixed)
    status: torch.Tensor             # [B] int32 0 success, 1 NaN, 2 max-iter, 4 QP failure
    iters: torch.Tensor              # [B, 2] int32  SQP iterations, interior-point iterations
    dV_dp: Optional[torch.Tensor]    # [B, n_p]
    dpi_dp: Optional[torch.Tensor]   # [B, nu, n_p]


@dataclass
class StateSens:
    dV_dx0: Optional[torch.Tensor]    # [B, nx]      dV/dx0, or dQ/dx0 when the solve had u0 fixed
    dQ_du0: Optional[torch.Tensor]    # [B, nu]      Q mode only
    dpi_dx0: Optional[torch.Tensor]   # [B, nu, nx]  du0*/dx0 (zeros in Q mode)


class BoxBounds(NamedTuple):
    """The box bounds of an OCP as tensors, the three groups of ``MPCBatch.set_bounds`` (shared by the batch, as the handle's bounds
    are): stage-0 controls, stages 1 .. N-1 in stage-vector order v = [u; x], terminal states.  |bound| >= 1e29 = absent."""
    lb0: torch.Tensor     # [nu]
    ub0: torch.Tensor     # [nu]
    lb: torch.Tensor      # [nu + nx]
    ub: torch.Tensor      # [nu + nx]
    lbe: torch.Tensor     # [nx]
    ube: torch.Tensor     # [nx]


class TrajectoryJacobian(NamedTuple):
    """``MPCBatch.trajectory_jacobian``: the Jacobian of the planned trajectory with respect to the initial state and the
    parameters.  The columns of the parameter blocks at entries the sensitivity pass does not differentiate are zeros."""
    dX_dx0: torch.Tensor       # [B, N + 1, nx, nx]
    dU_dx0: torch.Tensor       # [B, N, nu, nx]
    dX_dtheta: torch.Tensor    # [B, N + 1, nx, n_p]
    dU_dtheta: torch.Tensor    # [B, N, nu, n_p]


class ChainTrajectoryJacobian(NamedTuple):
    """``MPCBatch.chain_trajectory_jacobian``: columns of the Jacobian of the chain's planned trajectory with respect to the initial
    state and to the entries ``entries`` of the parameters.  The parameter blocks are compact: one column per entry asked for."""
    dX_dx0: torch.Tensor       # [B, N + 1, nx, nx]
    dU_dx0: torch.Tensor       # [B, N, nu, nx]
    dX_dtheta: torch.Tensor    # [B, N + 1, nx, len(entries)]
    dU_dtheta: torch.Tensor    # [B, N, nu, len(entries)]
    entries: torch.Tensor      # [len(entries)] int64: the index into p of each column


def chain_jacobian_entries(n_mass: int, entries=None) -> np.ndarray:
    """The index array into the chain's p that ``MPCBatch.chain_trajectory_jacobian(entries)`` differentiates: ``entries`` is an index
    array (checked against n_p and returned as int64), or a block name or tuple of block names of ``chain_param_layout`` — the blocks
    in the order given, each whole; None is the dynamics block ("m", "D", "L", "C")."""
    off, n_p = chain_param_layout(n_mass)[4:]
    if entries is None:
        entries = ("m", "D", "L", "C")
    if isinstance(entries, str):
        entries = (entries,)
    if len(entries) > 0 and all(isinstance(e, str) for e in entries):
        unknown = [e for e in entries if e not in off]
        if unknown:
            raise ValueError(f"the chain's parameter blocks are {', '.join(off)}; got {', '.join(unknown)}")
        return np.concatenate([np.arange(*off[e], dtype=np.int64) for e in entries])
    idx = np.asarray(entries.cpu() if isinstance(entries, torch.Tensor) else entries)
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
        raise ValueError("entries is a one-dimensional integer index array into p, or a tuple of block names")
    idx = idx.astype(np.int64)
    if idx.min() < 0 or idx.max() >= n_p:
        raise ValueError(f"entries index p, which has {n_p} entries at n_mass {n_mass}")
    return idx


class CartpoleCost(NamedTuple):
    """The cost block of the cartpole's parameter vector (entries 3 .. 82 of p) as tensors: l = 1/2 r' W r, r = y - yref, y = [x; u]
    on stages 0 .. N-1 (W_0, yref_0 on stage 0; W, yref on stages 1 .. N-1) and y = x on stage N (W_e, yref_e).  Leading batch
    dimensions are allowed on every member."""
    W_0: torch.Tensor       # [..., 5, 5]
    W: torch.Tensor         # [..., 5, 5]
    W_e: torch.Tensor       # [..., 4, 4]
    yref_0: torch.Tensor    # [..., 5]
    yref: torch.Tensor      # [..., 5]
    yref_e: torch.Tensor    # [..., 4]


_CARTPOLE_NP, _CARTPOLE_NDYN = 83, 3
_CARTPOLE_COST_FIELDS = ((3, 5, True), (28, 5, True), (53, 4, True), (69, 5, False), (74, 5, False), (79, 4, False))   # (offset, side, matrix)


def cartpole_cost_of(theta: torch.Tensor) -> CartpoleCost:
    """``theta[..., 3:]`` of a cartpole parameter vector [..., 83] as the six tensors of a CartpoleCost (each matrix is stored
    column-major in p).  Differentiable: views of ``theta``."""
    if theta.shape[-1] != _CARTPOLE_NP:
        raise ValueError(f"a cartpole parameter vector has {_CARTPOLE_NP} entries, got {theta.shape[-1]}")
    lead = theta.shape[:-1]
    return CartpoleCost(*(theta[..., o:o + n * n].reshape(lead + (n, n)).transpose(-1, -2) if mat else theta[..., o:o + n]
                          for o, n, mat in _CARTPOLE_COST_FIELDS))


def cartpole_theta(dyn: torch.Tensor, cost: CartpoleCost) -> torch.Tensor:
    """The inverse of ``cartpole_cost_of``: the dynamics block ``dyn`` [..., 3] and a CartpoleCost to a parameter vector [..., 83].
    Differentiable."""
    cost = CartpoleCost(*cost)
    if dyn.shape[-1] != _CARTPOLE_NDYN:
        raise ValueError(f"the cartpole's dynamics block has {_CARTPOLE_NDYN} entries, got {dyn.shape[-1]}")
    parts = [dyn]
    for t, (o, n, mat) in zip(cost, _CARTPOLE_COST_FIELDS):
        if (t.shape[-2:] != (n, n)) if mat else (t.shape[-1] != n):
            raise ValueError(f"CartpoleCost.{CartpoleCost._fields[len(parts) - 1]} has the shape {tuple(t.shape)}")
        parts.append(t.transpose(-1, -2).reshape(t.shape[:-2] + (n * n,)) if mat else t)
    lead = torch.broadcast_shapes(*(p.shape[:-1] for p in parts))
    return torch.cat([p.expand(lead + p.shape[-1:]) for p in parts], dim=-1)


class MPCBatch:
    """B independent instances of one OCP on one GPU.  The handle keeps the warm-start iterate of every
    instance (like the reference's solver object keeps its single iterate)."""

    def __init__(self, ocp: OcpDescription, batch: int, device: Optional[torch.device] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("mpc4rl_amd.MPCBatch needs a HIP device; there is no CPU fallback.")
        self.ocp = ocp
        self.B = int(batch)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:      # "cuda" = the current device, not GPU 0
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.nx, self.nu, self.N, self.n_p = ocp.nx, ocp.nu, ocp.N, ocp.n_p
        spec, keep = ocp.c_spec()
        h = C.c_void_p()
        _lib.call("mpcrl_create", C.byref(spec), self.B, self.device.index, C.byref(h))
        del keep
        self._h = h
        self._theta = None
        self.has_iterate = False       # a stored iterate exists (after a solve / set_iterate; cleared by reset)
        self.duals_valid = False       # ... and its bound multipliers / slacks come from a solve (not the cold placeholders)
        self._solve_status = None      # status tensor of the solve that stored the iterate (None: the iterate was set, not solved)
        self._solve_q_mode = False     # ... and whether that solve had u0 fixed
        self._is_chain = ocp.name.startswith("chain")
        # chain: the handle's workspace still describes the last solve (include/mpcrl_chain_ext.h; the library keeps the same flag)
        self._chain_ws_current = False
        self.set_theta(torch.as_tensor(ocp.p0, dtype=torch.float64))
        self.gamma = ocp.gamma

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.mpcrl_destroy(h)      # (not through _lib.call: at interpreter exit the module may be gone before the handle)

    @property
    def chain_workspace_current(self) -> bool:
        """Chain of masses: the handle's workspace still describes the last solve, which is what ``state_sens(policy=True)`` reads
        there (include/mpcrl_chain_ext.h).  False on the other models, before a solve and after anything else touched the handle."""
        return self._chain_ws_current

    # ------------------------------------------------------------------ helpers
    def _call(self, name: str, *args) -> int:
        return _lib.call(name, self._h, *args, device=self.device)

    # _stream and _check: for direct calls of self.lib (tests, profiles/microbench); the package's own calls go through _call
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, shape) -> torch.Tensor:
        t = torch.as_tensor(t, dtype=torch.float64, device=self.device).reshape(shape).contiguous()
        return t

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed with {rc}")

    # ------------------------------------------------------------------ parameters / options
    def set_theta(self, theta) -> None:
        """theta: [n_p] (shared) or [B, n_p] (per instance).  Mirrors MPC.set_p / set_parameter (mpc.py:137-154,233-257)."""
        t = torch.as_tensor(theta, dtype=torch.float64, device=self.device).contiguous()
        per = int(t.dim() == 2)
        if t.shape[-1] != self.n_p or (per and t.shape[0] != self.B):
            raise ValueError(f"theta must be [{self.n_p}] or [{self.B}, {self.n_p}]")
        self._theta = t
        self._call("mpcrl_set_theta", t, self.n_p, per)
        self._chain_ws_current = False

    def get_theta(self) -> torch.Tensor:
        return self._theta

    def set_discount_factor(self, gamma: float) -> None:
        """MPC.set_discount_factor (mpc.py:259-285)."""
        self.gamma = float(gamma)
        self._call("mpcrl_set_gamma", float(gamma))
        self._chain_ws_current = False

    def set_options(self, tol: float = -1.0, max_iter: int = -1) -> None:
        self._call("mpcrl_set_options", float(tol), int(max_iter))

    def set_exit_rule(self, window: int = 10, factor: float = 0.1) -> None:
        """Opt-in divergence exit (include/mpcrl.h mpcrl_set_exit_rule): every ``window`` SQP iterations the best NLP residual of an
        instance must have dropped below ``factor`` x its value at the previous check, else it ends with status 2.  window = 0: off
        (the reference's behaviour: full-step SQP to max_iter)."""
        self._call("mpcrl_set_exit_rule", int(window), float(factor))

    def set_launch_mode(self, mode: int = 0) -> None:
        """0 = the library times the time-sliced and the plain launch of the solve kernel against each other on this handle's own
        solves and uses the faster (default), 1 = time-sliced whenever legal, -1 = never (include/mpcrl.h mpcrl_set_launch_mode)."""
        self._call("mpcrl_set_launch_mode", int(mode))

    def launch_times(self, warm: bool = False):
        """(time-sliced ms, plain ms, preferred shape) of the launch tuner's last probes on cold (default) or warm calls; -1 = not
        measured yet."""
        a, b = C.c_double(-1.0), C.c_double(-1.0)
        rc = self._call("mpcrl_get_launch_times", int(warm), C.byref(a), C.byref(b))
        return a.value, b.value, ("plain" if rc == 1 else "time-sliced")

    def set_bounds(self, which: int, lb, ub) -> None:
        """ocp_solver.constraints_set (mpc.py:72-73,87-88): which = _lib.BOUNDS_U0 (stage-0 controls, nu values), BOUNDS_STAGE
        (stages 1..N-1, v = [u; x], nu + nx values), BOUNDS_TERMINAL (stage N, nx values); |bound| >= 1e29 = absent."""
        lb = np.ascontiguousarray(np.asarray(lb, float).reshape(-1))
        ub = np.ascontiguousarray(np.asarray(ub, float).reshape(-1))
        n = {_lib.BOUNDS_U0: self.nu, _lib.BOUNDS_STAGE: self.nu + self.nx, _lib.BOUNDS_TERMINAL: self.nx}[which]
        if lb.shape[0] != n or ub.shape[0] != n:
            raise ValueError(f"bounds of kind {which} have {n} entries")
        self._call("mpcrl_set_bounds", int(which), lb.ctypes.data, ub.ctypes.data)     # (host arrays of float64)
        self._chain_ws_current = False

    def reset(self, x0=None) -> None:
        """MPC.reset (mpc.py:204-210): the next solve starts from x_k = x0, u = 0, multipliers 0.  With x0 ([B, nx]) the stored
        iterate is set to that cold iterate as well (what get_iterate returns until the next solve)."""
        x0t = None if x0 is None else self._dev(x0, (self.B, self.nx))
        self._call("mpcrl_reset", x0t)
        self.has_iterate = self.duals_valid = False
        self._solve_status = None
        self._chain_ws_current = False

    def set_order(self, perm) -> None:
        """mpcrl_set_order: perm [B], a permutation of 0..B-1 (validity is the caller's contract) — slot i of the next launches works
        on instance perm[i]; None = identity.  A scheduling hint: no effect on results."""
        p = None if perm is None else torch.as_tensor(perm, device=self.device).to(torch.int32).reshape(self.B).contiguous()
        self._call("mpcrl_set_order", p)

    def get_order(self):
        """(perm [B] int32 or None = identity, state [3] = {spread, minimum, coordinate} of the last from-scratch auto order): what the
        next solve would read (mpcrl_debug_get_order, a test probe)."""
        perm = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        state = torch.empty((3,), dtype=torch.float64, device=self.device)
        rc = self._call("mpcrl_debug_get_order", perm, state)
        return (perm if rc == 1 else None), state

    # ------------------------------------------------------------------ the hot path
    def _pack_order(self, x0: torch.Tensor) -> None:
        """Scheduling hint: instances that share a wavefront run in lock-step for the maximum of their iteration counts, so
        neighbours should be similar problems.  Order the batch along the coordinate of x0 with the largest spread."""
        if self.B < 128:
            return
        if 64 // (self.N + 1) < 2:   # one instance per wavefront (the library also skips the chain at any horizon): no lock step to pack for
            self._call("mpcrl_set_order", None)
            return
        if self.B <= 8192:   # one small kernel inside the library (csrc/order_kernel.hpp)
            self._call("mpcrl_auto_order", x0)
            return
        dim = torch.argmax(x0.max(0).values - x0.min(0).values).reshape(1)     # stays on the device: no host sync
        perm = torch.argsort(torch.index_select(x0, 1, dim).reshape(-1)).to(torch.int32)
        self._call("mpcrl_set_order", perm)

    def solve(self, x0, u0=None, sens_v: bool = False, sens_pi: bool = False, rti: bool = False, cold: bool = False,
              reorder: bool = True, cold_mask: Optional[torch.Tensor] = None, store_bounds: bool = True,
              exact_qp: bool = False) -> SolveResult:
        """cold_mask [B] (bool / int): these instances ignore their stored iterate (per-environment ``mpc.reset`` at an episode end).
        store_bounds = False (MPCRL_NO_BND_STORE): the bound multipliers / slacks of the solution are not written back to the stored
        iterate — for callers that start every solve cold; the next solve then starts its interior point from the default point.
        exact_qp (MPCRL_EXACT_QP, test-only, cartpole): every QP solved to the tight tolerance, the reference's acados / HPIPM setting."""
        x0 = self._dev(x0, (self.B, self.nx))
        if cold_mask is not None:
            cm = cold_mask.to(device=self.device, dtype=torch.int32).reshape(self.B).contiguous()
            self._call("mpcrl_set_cold_mask", cm)
        u0f = None if u0 is None else self._dev(u0, (self.B, self.nu))
        flags = (_lib.SENS_V if sens_v else 0) | (_lib.SENS_PI if sens_pi else 0) | (_lib.RTI if rti else 0) | \
            (_lib.COLD if cold else 0) | (0 if store_bounds else _lib.NO_BND_STORE) | (_lib.EXACT_QP if exact_qp else 0)
        if reorder:
            if self._call("mpcrl_query_time_sliced", flags) == 1:
                # the time-sliced launch deals the batch out in quarters: no packing order needed (and none left over from before)
                self._call("mpcrl_set_order", None)
            else:
                self._pack_order(x0)
        kw = dict(dtype=torch.float64, device=self.device)
        u0_out = torch.empty((self.B, self.nu), **kw)
        V = torch.empty((self.B,), **kw)
        dV = torch.empty((self.B, self.n_p), **kw) if sens_v else None
        dpi = torch.empty((self.B, self.nu, self.n_p), **kw) if sens_pi else None
        status = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        iters = torch.empty((self.B, 2), dtype=torch.int32, device=self.device)
        self._call("mpcrl_solve", x0, u0f, flags, u0_out, V, dV, dpi, status, iters)
        self.has_iterate, self.duals_valid = True, bool(store_bounds)
        self._solve_status = status
        self._solve_q_mode = u0f is not None
        self._chain_ws_current = self._is_chain
        return SolveResult(u0_out, V, status, iters, dV, dpi)

    def state_sens(self, q_mode: bool = False, value: bool = True, policy: bool = True) -> StateSens:
        """Derivatives of the last solve with respect to its initial state and, in Q mode, its pinned first control
        (include/mpcrl_ext.h mpcrl_state_sens), from the iterate the handle stores.  q_mode: that solve had u0 fixed.  value:
        dV/dx0 (dQ/dx0 and dQ/du0 in Q mode).  policy: du0*/dx0 (zeros in Q mode).  On the chain of masses the policy part comes
        from the workspace of the last solve (include/mpcrl_chain_ext.h mpcrl_chain_policy_state_sens: one launch after a solve with
        sens_pi, four otherwise) and needs that solve to be the last thing that touched the handle: a set_theta, set_bounds,
        set_discount_factor, reset or set_iterate in between raises.  Rows of instances whose status is neither 0 nor 2 are zeros."""
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("state_sens needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        kw = dict(dtype=torch.float64, device=self.device)
        dV = torch.empty((self.B, self.nx), **kw) if value else None
        dQ = torch.empty((self.B, self.nu), **kw) if value and q_mode else None
        dpi = torch.empty((self.B, self.nu, self.nx), **kw) if policy else None
        flags = _lib.STATE_Q_MODE if q_mode else 0
        if self._is_chain and policy:
            if not self._chain_ws_current or self._solve_status is None:
                raise RuntimeError("state_sens(policy=True) on the chain of masses reads the workspace of the last solve, and the handle "
                                   "was changed since (set_theta, set_bounds, set_discount_factor, reset or set_iterate): solve again first")
            if value:
                self._call("mpcrl_state_sens", flags, dV, dQ, None)
            self._call("mpcrl_chain_policy_state_sens", flags, self._solve_status, dpi)
        else:
            self._call("mpcrl_state_sens", flags, dV, dQ, dpi)
        st = self._solve_status
        if st is not None:      # the library sees the stored iterate, not the status word: a failed QP (4) is selected out here
            good = (st == 0) | (st == 2)
            dV, dQ, dpi = (None if t is None else torch.where(good.reshape((self.B,) + (1,) * (t.dim() - 1)), t, torch.zeros_like(t))
                           for t in (dV, dQ, dpi))
        return StateSens(dV, dQ, dpi)

    def trajectory_vjp(self, gX=None, gU=None, x0: bool = True, theta: bool = True):
        """(g_x0 [B, nx] or None, g_theta [B, n_p] or None): the cotangents gX [B, N+1, nx] on X* and gU [B, N, nu] on U* of the last
        solve (None = zeros, not both) pulled back to its initial state and its parameters by one adjoint solve per instance
        (include/mpcrl_traj_ext.h mpcrl_traj_vjp), from the iterate the handle stores.  g_theta is zero at the entries of theta the
        sensitivity pass does not differentiate (the cartpole's cost block).  Rows of instances whose status is not 0 are zeros.
        Cartpole and linear system, after a solve without u0."""
        if self._is_chain:
            raise RuntimeError("trajectory_vjp is not available for the chain of masses")
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("trajectory_vjp needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        if self._solve_status is not None and self._solve_q_mode:
            raise RuntimeError("trajectory_vjp after a solve with u0 fixed (Q mode) is not available")
        if gX is None and gU is None:
            raise ValueError("trajectory_vjp needs a cotangent: gX, gU or both")
        if not (x0 or theta):
            raise ValueError("trajectory_vjp needs an output: x0, theta or both")
        gX = None if gX is None else self._dev(gX, (self.B, self.N + 1, self.nx))
        gU = None if gU is None else self._dev(gU, (self.B, self.N, self.nu))
        kw = dict(dtype=torch.float64, device=self.device)
        g_x0 = torch.empty((self.B, self.nx), **kw) if x0 else None
        g_th = torch.empty((self.B, self.n_p), **kw) if theta else None
        self._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th)
        st = self._solve_status
        if st is not None:      # as in state_sens: the library sees the stored iterate, not the status word
            good = (st == 0).reshape(self.B, 1)
            g_x0, g_th = (None if t is None else torch.where(good, t, torch.zeros_like(t)) for t in (g_x0, g_th))
        return g_x0, g_th

    def n_diff(self) -> int:
        """Number of leading entries of p the sensitivity pass differentiates on the cartpole and the linear system: the dynamics
        block m, M, l of the cartpole (its cost block is not), all twelve of the linear system."""
        if self._is_chain:
            raise RuntimeError("n_diff and the trajectory Jacobian are not available for the chain of masses")
        return _CARTPOLE_NDYN if self.n_p == _CARTPOLE_NP else self.n_p

    def trajectory_jvp(self, dx0=None, dtheta=None, X: bool = True, U: bool = True):
        """(dX [B, N+1, nx] or None, dU [B, N, nu] or None): how X* and U* of the last solve move when its initial state moves along
        dx0 [B, nx] and its parameters along dtheta [B, n_p] or [n_p] (None = zeros, not both) — the forward mode of
        ``trajectory_vjp``, one solve of the same linearised KKT system per instance and direction (include/mpcrl_traj_jvp_ext.h
        mpcrl_traj_jvp), from the iterate the handle stores.  With R directions per instance, dx0 [B, R, nx] and dtheta [B, R, n_p],
        the outputs are [B, R, N+1, nx] and [B, R, N, nu], from one launch.  dX[..., 0, :] is dx0.  Of dtheta only the entries the
        sensitivity pass differentiates are read (the first ``n_diff()``); the cartpole's cost block is ignored.  Rows of instances
        whose status is not 0 are zeros.  Cartpole and linear system, after a solve without u0."""
        if self._is_chain:
            raise RuntimeError("trajectory_jvp is not available for the chain of masses")
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("trajectory_jvp needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        if self._solve_status is not None and self._solve_q_mode:
            raise RuntimeError("trajectory_jvp after a solve with u0 fixed (Q mode) is not available")
        if dx0 is None and dtheta is None:
            raise ValueError("trajectory_jvp needs a direction: dx0, dtheta or both")
        if not (X or U):
            raise ValueError("trajectory_jvp needs an output: X, U or both")
        kw = dict(dtype=torch.float64, device=self.device)
        dx0 = None if dx0 is None else torch.as_tensor(dx0, **kw)
        dtheta = None if dtheta is None else torch.as_tensor(dtheta, **kw)
        if dtheta is not None and dtheta.dim() == 1:      # one direction in theta for the whole batch
            lead = (self.B,) if dx0 is None or dx0.dim() == 2 else (self.B, dx0.shape[1])
            dtheta = dtheta.reshape((1,) * len(lead) + (self.n_p,)).expand(lead + (self.n_p,))
        ranks = {t.dim() for t in (dx0, dtheta) if t is not None}
        if ranks not in ({2}, {3}):
            raise ValueError("trajectory_jvp takes dx0 [B, nx] / dtheta [B, n_p] or dx0 [B, R, nx] / dtheta [B, R, n_p]")
        single = ranks == {2}
        R = 1 if single else (dx0 if dx0 is not None else dtheta).shape[1]
        if R < 1:
            raise ValueError("trajectory_jvp needs at least one direction")
        dx0 = None if dx0 is None else self._dev(dx0, (self.B, R, self.nx))
        dtheta = None if dtheta is None else self._dev(dtheta, (self.B, R, self.n_p))
        dX = torch.empty((self.B, R, self.N + 1, self.nx), **kw) if X else None
        dU = torch.empty((self.B, R, self.N, self.nu), **kw) if U else None
        self._call("mpcrl_traj_jvp", 0, R, dx0, dtheta, dX, dU)
        st = self._solve_status
        if st is not None:      # as in trajectory_vjp: the library sees the stored iterate, not the status word
            good = (st == 0).reshape(self.B, 1, 1, 1)
            dX, dU = (None if t is None else torch.where(good, t, torch.zeros_like(t)) for t in (dX, dU))
        if single:
            dX, dU = (None if t is None else t[:, 0] for t in (dX, dU))
        return dX, dU

    def trajectory_jacobian(self) -> TrajectoryJacobian:
        """The full Jacobian of the last solve's plan, d(X*, U*) / d(x0, theta), from one ``trajectory_jvp`` with the
        nx + ``n_diff()`` unit directions.  The columns of the theta blocks past ``n_diff()`` are exact zeros."""
        nd, nx = self.n_diff(), self.nx      # (raises on the chain)
        kw = dict(dtype=torch.float64, device=self.device)
        dx0 = torch.zeros((self.B, nx + nd, nx), **kw)
        dth = torch.zeros((self.B, nx + nd, self.n_p), **kw)
        dx0[:, :nx] = torch.eye(nx, **kw)
        dth[:, nx:, :nd] = torch.eye(nd, **kw)
        dX, dU = self.trajectory_jvp(dx0, dth)
        dX, dU = dX.permute(0, 2, 3, 1), dU.permute(0, 2, 3, 1)      # [B, N + 1, nx, R], [B, N, nu, R]
        dX_dth = torch.zeros((self.B, self.N + 1, nx, self.n_p), **kw)
        dU_dth = torch.zeros((self.B, self.N, self.nu, self.n_p), **kw)
        dX_dth[..., :nd], dU_dth[..., :nd] = dX[..., nx:], dU[..., nx:]
        return TrajectoryJacobian(dX[..., :nx].contiguous(), dU[..., :nx].contiguous(), dX_dth, dU_dth)

    def chain_trajectory_vjp(self, gX=None, gU=None, x0: bool = True, theta: bool = True):
        """``trajectory_vjp`` for the chain of masses (include/mpcrl_chain_traj_ext.h mpcrl_chain_traj_vjp): (g_x0 [B, nx] or None,
        g_theta [B, n_p] or None) for the cotangents gX [B, N+1, nx] on X* and gU [B, N, nu] on U* of the last solve (None = zeros, not
        both), by one adjoint Riccati solve per instance on the workspace of that solve — three launches after a solve with sens_pi,
        five otherwise.  Like ``state_sens(policy=True)`` it needs that solve to be the last thing that touched the handle: a
        set_theta, set_bounds, set_discount_factor, reset or set_iterate in between raises.  After a solve without u0.  Rows of
        instances whose status is neither 0 nor 2 are zeros."""
        if not self._is_chain:
            raise RuntimeError("chain_trajectory_vjp is for the chain of masses; the cartpole and the linear system have trajectory_vjp")
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("chain_trajectory_vjp needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        if self._solve_status is not None and self._solve_q_mode:
            raise RuntimeError("chain_trajectory_vjp after a solve with u0 fixed (Q mode) is not available")
        if not self._chain_ws_current or self._solve_status is None:
            raise RuntimeError("chain_trajectory_vjp reads the workspace of the last solve, and the handle was changed since (set_theta, "
                               "set_bounds, set_discount_factor, reset or set_iterate): solve again first")
        if gX is None and gU is None:
            raise ValueError("chain_trajectory_vjp needs a cotangent: gX, gU or both")
        if not (x0 or theta):
            raise ValueError("chain_trajectory_vjp needs an output: x0, theta or both")
        gX = None if gX is None else self._dev(gX, (self.B, self.N + 1, self.nx))
        gU = None if gU is None else self._dev(gU, (self.B, self.N, self.nu))
        kw = dict(dtype=torch.float64, device=self.device)
        g_x0 = torch.empty((self.B, self.nx), **kw) if x0 else None
        g_th = torch.empty((self.B, self.n_p), **kw) if theta else None
        self._call("mpcrl_chain_traj_vjp", 0, self._solve_status, gX, gU, g_x0, g_th)
        return g_x0, g_th

    def chain_trajectory_jvp(self, dx0=None, dtheta=None, X: bool = True, U: bool = True):
        """``trajectory_jvp`` for the chain of masses (include/mpcrl_chain_traj_jvp_ext.h mpcrl_chain_traj_jvp): (dX [B, N+1, nx] or
        None, dU [B, N, nu] or None), how X* and U* of the last solve move when its initial state moves along dx0 [B, nx] and its
        parameters along dtheta [B, n_p] or [n_p] (None = zeros, not both) — the forward mode of ``chain_trajectory_vjp``, one primal
        Riccati solve per instance and direction on the workspace of that solve.  With R directions per instance, dx0 [B, R, nx] and
        dtheta [B, R, n_p], the outputs are [B, R, N+1, nx] and [B, R, N, nu]; a result does not depend on R or on the place of its
        direction.  dX[..., 0, :] is dx0.  Every entry of dtheta is read (m, D, L, C, Q, R, w).  The conditions are those of
        ``chain_trajectory_vjp``: the solve is the last thing that touched the handle, and it ran without u0.  Rows of instances whose
        status is neither 0 nor 2 are zeros."""
        if not self._is_chain:
            raise RuntimeError("chain_trajectory_jvp is for the chain of masses; the cartpole and the linear system have trajectory_jvp")
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("chain_trajectory_jvp needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        if self._solve_status is not None and self._solve_q_mode:
            raise RuntimeError("chain_trajectory_jvp after a solve with u0 fixed (Q mode) is not available")
        if not self._chain_ws_current or self._solve_status is None:
            raise RuntimeError("chain_trajectory_jvp reads the workspace of the last solve, and the handle was changed since (set_theta, "
                               "set_bounds, set_discount_factor, reset or set_iterate): solve again first")
        if dx0 is None and dtheta is None:
            raise ValueError("chain_trajectory_jvp needs a direction: dx0, dtheta or both")
        if not (X or U):
            raise ValueError("chain_trajectory_jvp needs an output: X, U or both")
        kw = dict(dtype=torch.float64, device=self.device)
        dx0 = None if dx0 is None else torch.as_tensor(dx0, **kw)
        dtheta = None if dtheta is None else torch.as_tensor(dtheta, **kw)
        if dtheta is not None and dtheta.dim() == 1:      # one direction in theta for the whole batch
            lead = (self.B,) if dx0 is None or dx0.dim() == 2 else (self.B, dx0.shape[1])
            dtheta = dtheta.reshape((1,) * len(lead) + (self.n_p,)).expand(lead + (self.n_p,))
        ranks = {t.dim() for t in (dx0, dtheta) if t is not None}
        if ranks not in ({2}, {3}):
            raise ValueError("chain_trajectory_jvp takes dx0 [B, nx] / dtheta [B, n_p] or dx0 [B, R, nx] / dtheta [B, R, n_p]")
        single = ranks == {2}
        R = 1 if single else (dx0 if dx0 is not None else dtheta).shape[1]
        if R < 1:
            raise ValueError("chain_trajectory_jvp needs at least one direction")
        dx0 = None if dx0 is None else self._dev(dx0, (self.B, R, self.nx))
        dtheta = None if dtheta is None else self._dev(dtheta, (self.B, R, self.n_p))
        dX = torch.empty((self.B, R, self.N + 1, self.nx), **kw) if X else None
        dU = torch.empty((self.B, R, self.N, self.nu), **kw) if U else None
        self._call("mpcrl_chain_traj_jvp", 0, self._solve_status, R, dx0, dtheta, dX, dU)
        if single:
            dX, dU = (None if t is None else t[:, 0] for t in (dX, dU))
        return dX, dU

    def chain_trajectory_jacobian(self, entries=None) -> ChainTrajectoryJacobian:
        """Columns of the Jacobian of the last chain solve's plan, d(X*, U*) / d(x0, theta[entries]), from ONE
        ``chain_trajectory_jvp`` with nx + len(entries) unit directions.  ``entries``: an index array into p, or a tuple of block names
        of ``chain_param_layout`` ("m", "D", "L", "C", "Q", "R", "w"); the default is the dynamics block ("m", "D", "L", "C").  The theta
        blocks are compact, [B, N+1, nx, len(entries)] and [B, N, nu, len(entries)]: a block n_p wide is 12.7 MB per instance at
        n_mass 7, N 40."""
        if not self._is_chain:
            raise RuntimeError("chain_trajectory_jacobian is for the chain of masses; the cartpole and the linear system have trajectory_jacobian")
        idx = chain_jacobian_entries((self.nx // 3 - 1) // 2 + 2, entries)
        ne, nx = len(idx), self.nx
        kw = dict(dtype=torch.float64, device=self.device)
        dx0 = torch.zeros((self.B, nx + ne, nx), **kw)
        dth = torch.zeros((self.B, nx + ne, self.n_p), **kw)
        dx0[:, :nx] = torch.eye(nx, **kw)
        dth[:, nx + torch.arange(ne, device=self.device), torch.as_tensor(idx, device=self.device)] = 1.0
        dX, dU = self.chain_trajectory_jvp(dx0, dth)
        dX, dU = dX.permute(0, 2, 3, 1), dU.permute(0, 2, 3, 1)      # [B, N + 1, nx, R], [B, N, nu, R]
        return ChainTrajectoryJacobian(dX[..., :nx].contiguous(), dU[..., :nx].contiguous(), dX[..., nx:].contiguous(),
                                       dU[..., nx:].contiguous(), torch.as_tensor(idx, device=self.device))

    def bound_value_grad(self, q_mode: bool = False):
        """(dV_dlb, dV_dub), each [B, N+1, nu+nx] in stage-vector order v = [u; x] (the layout of one plane of ``get_iterate``'s bnd):
        the derivative of the last solve's value (of Q after a solve with u0 fixed: q_mode) with respect to the lower / upper bound of
        every stage and coordinate, lam_l and -lam_u (include/mpcrl_bound_ext.h mpcrl_bound_value_grad).  One entry per stage: sum
        them onto the groups of ``set_bounds`` with ``fold_bound_grad``.  Exactly zero where no bound row exists (absent bounds,
        stage-0 states, terminal controls, in Q mode the stage-0 controls).  Every model.  Rows of instances whose status is neither
        0 nor 2 are zeros."""
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("bound_value_grad needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        kw = dict(dtype=torch.float64, device=self.device)
        shape = (self.B, self.N + 1, self.nu + self.nx)
        dlb, dub = torch.empty(shape, **kw), torch.empty(shape, **kw)
        self._call("mpcrl_bound_value_grad", _lib.STATE_Q_MODE if q_mode else 0, dlb, dub)
        st = self._solve_status
        if st is not None:      # as in state_sens: the library sees the stored iterate, not the status word
            good = ((st == 0) | (st == 2)).reshape(self.B, 1, 1)
            dlb, dub = (torch.where(good, t, torch.zeros_like(t)) for t in (dlb, dub))
        return dlb, dub

    def bound_vjp(self, gX=None, gU=None, x0: bool = True, theta: bool = True, bounds: bool = True):
        """(g_x0 [B, nx], g_theta [B, n_p], g_lb, g_ub [B, N+1, nu+nx]; None where not asked for): ``trajectory_vjp`` /
        ``chain_trajectory_vjp`` — whichever the model has — with the cotangents also pulled back to the box bounds, every stage and
        coordinate of v = [u; x] on its own (include/mpcrl_bound_ext.h mpcrl_bound_vjp / mpcrl_chain_bound_vjp): the same ONE adjoint
        solve per instance serves all four.  g_lb / g_ub are exactly zero where no bound row exists; ``fold_bound_grad`` sums them
        onto the groups of ``set_bounds``.  The conditions and the rows that are zeros are those of the model's trajectory VJP."""
        name = "chain_trajectory_vjp" if self._is_chain else "trajectory_vjp"
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError(f"{name} needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        if self._solve_status is not None and self._solve_q_mode:
            raise RuntimeError(f"{name} after a solve with u0 fixed (Q mode) is not available")
        if self._is_chain and (not self._chain_ws_current or self._solve_status is None):
            raise RuntimeError("chain_trajectory_vjp reads the workspace of the last solve, and the handle was changed since (set_theta, "
                               "set_bounds, set_discount_factor, reset or set_iterate): solve again first")
        if gX is None and gU is None:
            raise ValueError(f"{name} needs a cotangent: gX, gU or both")
        if not (x0 or theta or bounds):
            raise ValueError("bound_vjp needs an output: x0, theta, bounds or any of them")
        gX = None if gX is None else self._dev(gX, (self.B, self.N + 1, self.nx))
        gU = None if gU is None else self._dev(gU, (self.B, self.N, self.nu))
        kw = dict(dtype=torch.float64, device=self.device)
        g_x0 = torch.empty((self.B, self.nx), **kw) if x0 else None
        g_th = torch.empty((self.B, self.n_p), **kw) if theta else None
        g_lb = torch.empty((self.B, self.N + 1, self.nu + self.nx), **kw) if bounds else None
        g_ub = torch.empty((self.B, self.N + 1, self.nu + self.nx), **kw) if bounds else None
        if self._is_chain:
            self._call("mpcrl_chain_bound_vjp", 0, self._solve_status, gX, gU, g_x0, g_th, g_lb, g_ub)
            return g_x0, g_th, g_lb, g_ub
        self._call("mpcrl_bound_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub)
        st = self._solve_status
        if st is not None:      # as in trajectory_vjp: the library sees the stored iterate, not the status word
            good = st == 0
            g_x0, g_th, g_lb, g_ub = (None if t is None else torch.where(good.reshape((self.B,) + (1,) * (t.dim() - 1)), t, torch.zeros_like(t))
                                      for t in (g_x0, g_th, g_lb, g_ub))
        return g_x0, g_th, g_lb, g_ub

    def cost_value_grad(self) -> torch.Tensor:
        """dV/dcost [B, n_p] of the last solve (dQ/dcost after a solve with u0 fixed), cartpole only: the derivative of the value with
        respect to every entry of the cost block of p, each an independent variable (include/mpcrl_cost_ext.h mpcrl_cost_value_grad;
        ``cartpole_cost_of`` splits a row into W_0, W, W_e, yref_0, yref, yref_e).  Entries 0 .. 2 are exactly zero — the dynamics
        block is ``SolveResult.dV_dp``'s, whose own cost block stays zero.  Rows of instances whose status is neither 0 nor 2 are
        zeros."""
        if self.ocp.name != "cartpole":
            raise RuntimeError("cost_value_grad is for the cartpole: the linear system keeps its weights in consts, the chain has Q, R in dV_dp")
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("cost_value_grad needs the iterate of a solve (solve with store_bounds=True first)")
        dV = torch.empty((self.B, self.n_p), dtype=torch.float64, device=self.device)
        self._call("mpcrl_cost_value_grad", 0, dV)
        st = self._solve_status
        if st is not None:      # as in state_sens: the library sees the stored iterate, not the status word
            dV = torch.where(((st == 0) | (st == 2)).reshape(self.B, 1), dV, torch.zeros_like(dV))
        return dV

    def cost_vjp(self, gX=None, gU=None, x0: bool = True, theta: bool = True, bounds: bool = False, cost: bool = True):
        """(g_x0 [B, nx], g_theta [B, n_p], g_lb, g_ub [B, N+1, nu+nx], g_cost [B, n_p]; None where not asked for): ``bound_vjp`` with
        the cotangents also pulled back to the cartpole's cost block (include/mpcrl_cost_ext.h mpcrl_cost_vjp): the same ONE launch
        and ONE adjoint solve per instance serve all five.  g_cost is in the layout of p with exact zeros on entries 0 .. 2, and
        g_theta keeps its zero cost block, so the gradient with respect to the whole of p is ``g_theta + g_cost``.  Cartpole only;
        the conditions and the rows that are zeros are those of ``trajectory_vjp``."""
        if self.ocp.name != "cartpole":
            raise RuntimeError("cost_vjp is for the cartpole: the linear system keeps its weights in consts, the chain has Q, R in g_theta")
        if not (self.has_iterate and self.duals_valid):
            raise RuntimeError("cost_vjp needs the iterate of a solve with its bound multipliers (solve with store_bounds=True first)")
        if self._solve_status is not None and self._solve_q_mode:
            raise RuntimeError("cost_vjp after a solve with u0 fixed (Q mode) is not available")
        if gX is None and gU is None:
            raise ValueError("cost_vjp needs a cotangent: gX, gU or both")
        if not (x0 or theta or bounds or cost):
            raise ValueError("cost_vjp needs an output: x0, theta, bounds, cost or any of them")
        gX = None if gX is None else self._dev(gX, (self.B, self.N + 1, self.nx))
        gU = None if gU is None else self._dev(gU, (self.B, self.N, self.nu))
        kw = dict(dtype=torch.float64, device=self.device)
        g_x0 = torch.empty((self.B, self.nx), **kw) if x0 else None
        g_th = torch.empty((self.B, self.n_p), **kw) if theta else None
        g_lb = torch.empty((self.B, self.N + 1, self.nu + self.nx), **kw) if bounds else None
        g_ub = torch.empty((self.B, self.N + 1, self.nu + self.nx), **kw) if bounds else None
        g_c = torch.empty((self.B, self.n_p), **kw) if cost else None
        self._call("mpcrl_cost_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub, g_c)
        st = self._solve_status
        if st is not None:      # as in trajectory_vjp: the library sees the stored iterate, not the status word
            good = st == 0
            g_x0, g_th, g_lb, g_ub, g_c = (None if t is None else torch.where(good.reshape((self.B,) + (1,) * (t.dim() - 1)), t, torch.zeros_like(t))
                                           for t in (g_x0, g_th, g_lb, g_ub, g_c))
        return g_x0, g_th, g_lb, g_ub, g_c

    def fold_bound_grad(self, g: torch.Tensor):
        """A per-stage bound gradient g [B, N+1, nu+nx] (``bound_vjp``, ``bound_value_grad``) summed onto the three groups of
        ``set_bounds``: (U0 [B, nu]: the controls of stage 0, STAGE [B, nu+nx]: stages 1 .. N-1, TERMINAL [B, nx]: the states of
        stage N).  Tensors only: runs on any device."""
        if g.dim() != 3 or g.shape[1] != self.N + 1 or g.shape[2] != self.nu + self.nx:
            raise ValueError(f"a bound gradient is [B, {self.N + 1}, {self.nu + self.nx}]")
        return g[:, 0, :self.nu], g[:, 1:self.N].sum(1), g[:, self.N, self.nu:]

    def get_action(self, x0) -> torch.Tensor:
        """Batched MPC.get_action (mpc.py:27-50)."""
        return self.solve(x0).u0

    # ------------------------------------------------------------------ iterate access
    def get_iterate(self):
        """x [B,N+1,nx], u [B,N,nu], pi [B,N,nx], bnd [B,10,N+1,nu+nx], res [B,4] (layouts of include/mpcrl.h)."""
        kw = dict(dtype=torch.float64, device=self.device)
        nw = self.nx + self.nu
        x = torch.empty((self.B, self.N + 1, self.nx), **kw)
        u = torch.empty((self.B, self.N, self.nu), **kw)
        pi = torch.empty((self.B, self.N, self.nx), **kw)
        bnd = torch.empty((self.B, 10, self.N + 1, nw), **kw)
        res = torch.empty((self.B, 4), **kw)
        self._call("mpcrl_get_iterate", x, u, pi, bnd, res)
        return x, u, pi, bnd, res

    def set_iterate(self, x, u, pi, bnd=None) -> None:
        """bnd = None: the bound multipliers / slacks are reset to the cold state and the next solve starts its interior point from
        the default point (MPCRL_COLD_DUAL) — an initial guess for x, u, pi, not a warm start."""
        nw = self.nx + self.nu
        x = self._dev(x, (self.B, self.N + 1, self.nx))
        u = self._dev(u, (self.B, self.N, self.nu))
        pi = self._dev(pi, (self.B, self.N, self.nx))
        bnd = None if bnd is None else self._dev(bnd, (self.B, 10, self.N + 1, nw))
        self._call("mpcrl_set_iterate", x, u, pi, bnd)
        self.has_iterate, self.duals_valid = True, bnd is not None
        self._solve_status = None
        self._chain_ws_current = False

    def _row_tables(self, x, u, pi, bnd, index):
        nw = self.nx + self.nu
        lens = ((self.N + 1) * self.nx, self.N * self.nu, self.N * self.nx, 10 * (self.N + 1) * nw)
        for t, n in zip((x, u, pi, bnd), lens):
            if t is not None and not (t.dtype == torch.float64 and t.is_contiguous() and t.device == self.device and t.numel() % n == 0):
                raise ValueError("iterate tables are contiguous float64 tensors on the handle's device with whole rows")
        if index is not None and not (index.dtype == torch.int64 and index.is_contiguous() and index.numel() == self.B and index.device == self.device):
            raise ValueError("index: contiguous int64 [B] on the handle's device")

    def get_iterate_rows(self, x, u, pi, bnd, index: Optional[torch.Tensor] = None) -> None:
        """Table row index[i] := stored iterate of instance i (mpcrl_get_iterate_rows; the tables are the caller's, any number of rows,
        rows laid out as get_iterate's; None = skip that array)."""
        self._row_tables(x, u, pi, bnd, index)
        self._call("mpcrl_get_iterate_rows", x, u, pi, bnd, index)

    def set_iterate_rows(self, x, u, pi, bnd, index: Optional[torch.Tensor] = None) -> None:
        """Stored iterate of instance i := table row index[i] (mpcrl_set_iterate_rows); bnd = None as in set_iterate."""
        self._row_tables(x, u, pi, bnd, index)
        self._call("mpcrl_set_iterate_rows", x, u, pi, bnd, index)
        self.has_iterate, self.duals_valid = True, bnd is not None
        self._solve_status = None
        self._chain_ws_current = False

    def get_lagrangian(self) -> torch.Tensor:
        """[B] Lagrangian of the mirror NLP at the iterate of the last solve (nlp.L, nlp.py:1180,1390)."""
        L = torch.empty((self.B,), dtype=torch.float64, device=self.device)
        self._call("mpcrl_get_lagrangian", L)
        return L

    def workspace_bytes(self) -> int:
        return self._call("mpcrl_workspace_bytes")
