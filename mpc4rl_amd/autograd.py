"""The MPC as a differentiable torch layer: ``u0, V = layer(x0, theta)`` and ``Q = layer.q(x0, u0, theta)`` inside a torch graph.

The forward pass is one solve of the ``MPCBatch`` the layer is built around — with the parameter sensitivities ``theta.requires_grad``
calls for — and, when ``x0`` (or the pinned ``u0``) needs a gradient, one ``mpcrl_state_sens`` (include/mpcrl_ext.h).  The backward
pass is plain torch contractions of the stored Jacobians with the incoming gradients (``mpc_backward_terms``):

    g_x0    = g_u' du0*/dx0 + g_V dV/dx0
    g_theta = g_u' du0*/dp  + g_V dV/dp          summed over the batch for a shared theta [n_p], per instance for theta [B, n_p]
    g_u0    = g_Q dQ/du0                         (``layer.q``)

Instances whose solve did not end with status 0 contribute zero gradient; ``layer.last_status`` keeps the statuses.  On the chain of
masses du0*/dx0 is opt-in (``MPCLayer(..., policy_jacobian=True)``; include/mpcrl_chain_ext.h): the layer computes the state
sensitivities in ``forward``, before it knows whether ``g_u`` will arrive, and there that is three more launches per forward pass
whenever the solve itself did not run the du0*/dp pass.  Without it a loss that depends on ``u0`` cannot be back-propagated to ``x0``
on a chain, and asking for it raises.

``X, U = layer.trajectory(x0, theta)`` returns the whole plan X* [B, N+1, nx], U* [B, N, nu] (every model).  Its forward
pass is one plain solve — no sensitivity pass — and its backward pass one ``mpcrl_traj_vjp`` (include/mpcrl_traj_ext.h; on the chain of
masses ``mpcrl_chain_traj_vjp``, include/mpcrl_chain_traj_ext.h, through ``MPCBatch.chain_trajectory_vjp``: no opt-in) with the incoming
(g_X, g_U): one adjoint solve per instance whatever the horizon.  That call reads the iterate the handle stores, so the iterate must
still be that forward pass's: every ``forward``, ``q`` and ``trajectory`` of a layer increments the layer's pass counter, and
``backward`` raises a RuntimeError when the counter is no longer the one its forward pass recorded ("one backward per forward, before
the layer runs again").  Setters called on the batch directly (``set_theta``, ``set_iterate``, ``reset``, ``solve`` ...) between the
forward and the backward pass are the caller's responsibility: the layer does not see them.

``layer(x0, theta, bounds)`` and ``layer.trajectory(x0, theta, bounds)`` with ``bounds`` a ``BoxBounds`` of six tensors (the three
groups of ``MPCBatch.set_bounds``, shared by the batch) also differentiate with respect to the box bounds (include/mpcrl_bound_ext.h):
learned constraint back-offs.  The forward pass copies the six tensors to the host and calls ``set_bounds`` for the three groups — a
HOST SYNCHRONISATION per forward pass, and the bounds stay set on the batch afterwards — then solves as above.  The backward pass of
``trajectory`` is ONE ``MPCBatch.bound_vjp`` for everything that requires a gradient (x0, theta and the bounds: the same adjoint solve
serves them all), the per-stage rows folded onto the groups (``fold_bound_grad``) and summed over the batch; that of ``forward`` adds,
for the bounds, one ``bound_vjp`` with g_u as the cotangent on stage 0 of U* plus g_V dV/db (``bound_value_grad``: lam_l, -lam_u).
Members of ``bounds`` that do not require a gradient get none; instances excluded from the theta gradient (status != 0) contribute
zero; both backward passes read the stored iterate, so the pass-counter rule above covers them.  With ``bounds=None`` nothing changes:
the layer makes the calls it made before.  ``layer.q`` takes no bounds.

``MPCLayer(batch, cost_gradient=True)`` (cartpole only; off by default) also differentiates with respect to the tracking cost, the 80
entries W_0, W, W_e, yref_0, yref, yref_e of theta (include/mpcrl_cost_ext.h; ``cartpole_cost_of`` / ``cartpole_theta`` split and join
them): ``theta.grad`` then carries the cost block, which is exactly zero without the opt-in (dV/dp, du0*/dp and g_theta keep the
convention of the reference's mirror, whose cost is not parameterised).  The backward pass of ``trajectory`` is ONE
``MPCBatch.cost_vjp`` for x0, theta, the cost block and the bounds; ``forward`` adds g_V dV/dcost (``cost_value_grad``, computed in the
forward pass when theta requires a gradient) plus, when g_u arrives, one ``cost_vjp`` with g_u as the cotangent on stage 0 of U* — the
call that serves the bounds as well when they need a gradient; ``q`` adds g_Q dQ/dcost.  Instances with a status other than 0 are
selected out, and the pass-counter rule covers the ``cost_vjp`` calls.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .batch import BoxBounds, MPCBatch


def mpc_backward_terms(g_u: Optional[torch.Tensor], g_V: Optional[torch.Tensor], status: torch.Tensor,
                       du_dx0: Optional[torch.Tensor], dV_dx0: Optional[torch.Tensor],
                       du_dp: Optional[torch.Tensor], dV_dp: Optional[torch.Tensor],
                       shared_theta: bool) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(g_x0 [B, nx] or None, g_theta [n_p] / [B, n_p] or None) from the incoming gradients g_u [B, nu], g_V [B] (None = the loss does
    not depend on that output) and the Jacobians du_dx0 [B, nu, nx], dV_dx0 [B, nx], du_dp [B, nu, n_p], dV_dp [B, n_p] (None = that
    side is not wanted).  Rows of instances with status != 0 are selected out of every Jacobian before it is contracted, so whatever
    they hold (NaN included) never reaches a gradient.  Tensors only: runs on any device."""
    good = status == 0

    def rows(J):      # a select, not a product with a mask: 0 * NaN would be NaN
        return torch.where(good.reshape((-1,) + (1,) * (J.dim() - 1)), J, torch.zeros_like(J))

    def contract(du, dV):
        g = None
        if g_u is not None and du is not None:
            g = torch.einsum("bi,bij->bj", g_u, rows(du))
        if g_V is not None and dV is not None:
            t = g_V.reshape(-1, 1) * rows(dV)
            g = t if g is None else g + t
        return g

    g_x0 = contract(du_dx0, dV_dx0)
    g_th = contract(du_dp, dV_dp)
    if g_th is not None and shared_theta:
        g_th = g_th.sum(0)
    return g_x0, g_th


class MPCFunction(torch.autograd.Function):
    """(x0 [B, nx], theta [n_p] | [B, n_p]) -> (u0 [B, nu], V [B]) through ``layer.batch``."""

    @staticmethod
    def forward(ctx, x0, theta, layer):
        mpc: MPCBatch = layer.batch
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), sens_v=need_p, sens_pi=need_p, **layer.solve_args)
        s = mpc.state_sens(q_mode=False, value=True, policy=layer.has_policy_jacobian) if need_x else None
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.shared = theta.dim() == 1
        ctx.dtypes = (x0.dtype, theta.dtype)
        ctx.policy, ctx.chain = layer.has_policy_jacobian, layer.batch.ocp.name.startswith("chain")
        ctx.jac = (r.status, None if s is None else s.dpi_dx0, None if s is None else s.dV_dx0, r.dpi_dp, r.dV_dp)
        return r.u0.to(x0.dtype), r.V.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_u, g_V):
        status, du_dx0, dV_dx0, du_dp, dV_dp = ctx.jac
        if g_u is not None and ctx.needs_input_grad[0] and not ctx.policy:
            if not ctx.chain:
                raise RuntimeError("MPCLayer: the loss depends on u0 and x0 requires a gradient, but the layer was built with "
                                   "policy_jacobian=False; detach x0 or keep u0 out of the loss.")
            raise RuntimeError("MPCLayer: the loss depends on u0 and x0 requires a gradient, but du0*/dx0 is not available for the chain "
                               "of masses (dV/dx0, dQ/dx0 and dQ/du0 are) unless the layer is built with policy_jacobian=True; detach "
                               "x0 or keep u0 out of the loss.")
        f64 = [None if g is None else g.to(torch.float64) for g in (g_u, g_V)]
        g_x0, g_th = mpc_backward_terms(f64[0], f64[1], status, du_dx0, dV_dx0, du_dp, dV_dp, ctx.shared)
        return (None if g_x0 is None or not ctx.needs_input_grad[0] else g_x0.to(ctx.dtypes[0]),
                None if g_th is None or not ctx.needs_input_grad[1] else g_th.to(ctx.dtypes[1]), None)


class MPCQFunction(torch.autograd.Function):
    """(x0 [B, nx], u0 [B, nu], theta) -> Q [B]: the solve with u_0 pinned."""

    @staticmethod
    def forward(ctx, x0, u0, theta, layer):
        mpc: MPCBatch = layer.batch
        need_s, need_p = ctx.needs_input_grad[0] or ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), u0.detach().to(torch.float64), sens_v=need_p, **layer.solve_args)
        s = mpc.state_sens(q_mode=True, value=True, policy=False) if need_s else None
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.shared = theta.dim() == 1
        ctx.dtypes = (x0.dtype, u0.dtype, theta.dtype)
        ctx.jac = (r.status, None if s is None else s.dV_dx0, None if s is None else s.dQ_du0, r.dV_dp)
        ctx.dQ_dc = mpc.cost_value_grad() if need_p and layer.cost_gradient else None
        return r.V.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_Q):
        status, dQ_dx0, dQ_du0, dQ_dp = ctx.jac
        if g_Q is None:
            return None, None, None, None
        g_Q = g_Q.to(torch.float64)
        g_x0, g_th = mpc_backward_terms(None, g_Q, status, None, dQ_dx0, None, dQ_dp, ctx.shared)
        g_u0, _ = mpc_backward_terms(None, g_Q, status, None, dQ_du0, None, None, ctx.shared)
        if ctx.dQ_dc is not None:
            g_th = g_th + _cost_term(g_Q.reshape(-1, 1) * ctx.dQ_dc, status == 0, ctx.shared)
        return tuple(g.to(dt) if need and g is not None else None
                     for g, need, dt in zip((g_x0, g_u0, g_th), ctx.needs_input_grad[:3], ctx.dtypes)) + (None,)


class MPCTrajectoryFunction(torch.autograd.Function):
    """(x0 [B, nx], theta [n_p] | [B, n_p]) -> (X [B, N+1, nx], U [B, N, nu]) through ``layer.batch``; ``backward`` is one
    ``MPCBatch.trajectory_vjp`` (``chain_trajectory_vjp`` when the batch's OCP is a chain of masses) on the iterate that forward pass
    left in the handle (the layer's pass counter guards it)."""

    @staticmethod
    def forward(ctx, x0, theta, layer):
        mpc = layer.batch
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), **layer.solve_args)
        X, U = mpc.get_iterate()[:2]
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.layer, ctx.pass_id = layer, layer.pass_counter
        ctx.shared = theta.dim() == 1
        ctx.dtypes = (x0.dtype, theta.dtype)
        return X.to(x0.dtype), U.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_X, g_U):
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_X is None and g_U is None) or not (need_x or need_p):
            return None, None, None
        if ctx.layer.pass_counter != ctx.pass_id:
            raise RuntimeError("MPCLayer.trajectory: the backward pass reads the iterate its forward pass stored in the handle, and the "
                               "layer has run another forward, q or trajectory since (pass counter "
                               f"{ctx.layer.pass_counter}, recorded {ctx.pass_id}): one backward per forward, before the layer runs again.")
        batch = ctx.layer.batch
        vjp = batch.chain_trajectory_vjp if batch.ocp.name.startswith("chain") else batch.trajectory_vjp
        g_x0, g_th = vjp(None if g_X is None else g_X.to(torch.float64), None if g_U is None else g_U.to(torch.float64),
                         x0=need_x, theta=need_p)
        if g_th is not None and ctx.shared:
            g_th = g_th.sum(0)
        return (None if g_x0 is None else g_x0.to(ctx.dtypes[0]), None if g_th is None else g_th.to(ctx.dtypes[1]), None)


def _apply_bounds(mpc, bounds) -> None:
    """The six tensors of a BoxBounds to the host and into the handle (three ``set_bounds``): a host synchronisation."""
    host = [b.detach().to(torch.float64).cpu().numpy() for b in bounds]
    mpc.set_bounds(_lib.BOUNDS_U0, host[0], host[1])
    mpc.set_bounds(_lib.BOUNDS_STAGE, host[2], host[3])
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, host[4], host[5])


def _bound_grads(mpc, g_lb, g_ub, good, needs, like):
    """Per-stage bound gradients g_lb, g_ub [B, N+1, nu+nx] -> the six gradients of a BoxBounds (None where not needed): rows of
    instances outside ``good`` selected out, folded onto the groups of ``set_bounds`` and summed over the batch; ``like``: the
    (device, dtype) of each member (the bounds may live on the host)."""
    out = []
    for g in (g_lb, g_ub):
        g = torch.where(good.reshape(-1, 1, 1), g, torch.zeros_like(g))
        out.append([t.sum(0) for t in mpc.fold_bound_grad(g)])
    six = (out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2])      # lb0, ub0, lb, ub, lbe, ube
    return tuple(g.to(device=dev, dtype=dt) if need else None for g, need, (dev, dt) in zip(six, needs, like))


def _stale(ctx, what: str):
    if ctx.layer.pass_counter != ctx.pass_id:
        raise RuntimeError(f"MPCLayer.{what}: the backward pass reads the iterate its forward pass stored in the handle, and the "
                           "layer has run another forward, q or trajectory since (pass counter "
                           f"{ctx.layer.pass_counter}, recorded {ctx.pass_id}): one backward per forward, before the layer runs again.")


class MPCBoundedFunction(torch.autograd.Function):
    """``MPCFunction`` with the box bounds as inputs: (x0, theta, lb0, ub0, lb, ub, lbe, ube) -> (u0, V).  The x0 and theta sides
    are ``MPCFunction``'s; the bounds' gradient is one ``MPCBatch.bound_vjp`` (g_u on stage 0 of U*) plus g_V dV/db."""

    @staticmethod
    def forward(ctx, x0, theta, lb0, ub0, lb, ub, lbe, ube, layer):
        mpc: MPCBatch = layer.batch
        need_x, need_p, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2:8]
        _apply_bounds(mpc, (lb0, ub0, lb, ub, lbe, ube))
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), sens_v=need_p, sens_pi=need_p, **layer.solve_args)
        s = mpc.state_sens(q_mode=False, value=True, policy=layer.has_policy_jacobian) if need_x else None
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.layer, ctx.pass_id = layer, layer.pass_counter
        ctx.shared = theta.dim() == 1
        ctx.dtypes, ctx.like = (x0.dtype, theta.dtype), tuple((b.device, b.dtype) for b in (lb0, ub0, lb, ub, lbe, ube))
        ctx.policy, ctx.chain = layer.has_policy_jacobian, layer.batch.ocp.name.startswith("chain")
        ctx.jac = (r.status, None if s is None else s.dpi_dx0, None if s is None else s.dV_dx0, r.dpi_dp, r.dV_dp)
        ctx.dV_db = mpc.bound_value_grad(q_mode=False) if any(need_b) else None
        return r.u0.to(x0.dtype), r.V.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_u, g_V):
        status, du_dx0, dV_dx0, du_dp, dV_dp = ctx.jac
        need_b = ctx.needs_input_grad[2:8]
        if g_u is not None and ctx.needs_input_grad[0] and not ctx.policy:
            raise RuntimeError("MPCLayer: the loss depends on u0 and x0 requires a gradient, but du0*/dx0 is not available: build the layer "
                               "with policy_jacobian=True, detach x0 or keep u0 out of the loss.")
        f64 = [None if g is None else g.to(torch.float64) for g in (g_u, g_V)]
        g_x0, g_th = mpc_backward_terms(f64[0], f64[1], status, du_dx0, dV_dx0, du_dp, dV_dp, ctx.shared)
        g_b = (None,) * 6
        if any(need_b) and (g_u is not None or g_V is not None):
            mpc = ctx.layer.batch
            g_lb = g_ub = None
            if g_u is not None:
                _stale(ctx, "forward")
                gU = torch.zeros((mpc.B, mpc.N, mpc.nu), dtype=torch.float64, device=f64[0].device)
                gU[:, 0] = f64[0]
                g_lb, g_ub = mpc.bound_vjp(None, gU, x0=False, theta=False, bounds=True)[2:]
            if g_V is not None:
                dlb, dub = (f64[1].reshape(-1, 1, 1) * d for d in ctx.dV_db)
                g_lb, g_ub = (dlb, dub) if g_lb is None else (g_lb + dlb, g_ub + dub)
            g_b = _bound_grads(mpc, g_lb, g_ub, status == 0, need_b, ctx.like)
        return (None if g_x0 is None or not ctx.needs_input_grad[0] else g_x0.to(ctx.dtypes[0]),
                None if g_th is None or not ctx.needs_input_grad[1] else g_th.to(ctx.dtypes[1])) + g_b + (None,)


class MPCBoundedTrajectoryFunction(torch.autograd.Function):
    """``MPCTrajectoryFunction`` with the box bounds as inputs: (x0, theta, lb0, ub0, lb, ub, lbe, ube) -> (X, U); ``backward`` is one
    ``MPCBatch.bound_vjp`` for everything that requires a gradient."""

    @staticmethod
    def forward(ctx, x0, theta, lb0, ub0, lb, ub, lbe, ube, layer):
        mpc = layer.batch
        _apply_bounds(mpc, (lb0, ub0, lb, ub, lbe, ube))
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), **layer.solve_args)
        X, U = mpc.get_iterate()[:2]
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.layer, ctx.pass_id, ctx.status = layer, layer.pass_counter, r.status
        ctx.shared = theta.dim() == 1
        ctx.dtypes, ctx.like = (x0.dtype, theta.dtype), tuple((b.device, b.dtype) for b in (lb0, ub0, lb, ub, lbe, ube))
        return X.to(x0.dtype), U.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_X, g_U):
        need_x, need_p, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2:8]
        if (g_X is None and g_U is None) or not (need_x or need_p or any(need_b)):
            return (None,) * 9
        _stale(ctx, "trajectory")
        mpc = ctx.layer.batch
        g_x0, g_th, g_lb, g_ub = mpc.bound_vjp(None if g_X is None else g_X.to(torch.float64), None if g_U is None else g_U.to(torch.float64),
                                               x0=need_x, theta=need_p, bounds=any(need_b))
        if g_th is not None and ctx.shared:
            g_th = g_th.sum(0)
        # the rows bound_vjp keeps are those its model's trajectory VJP keeps (the chain: statuses 0 and 2): the bounds take the same
        g_b = _bound_grads(mpc, g_lb, g_ub, torch.ones_like(ctx.status, dtype=torch.bool), need_b, ctx.like) if any(need_b) else (None,) * 6
        return (None if g_x0 is None else g_x0.to(ctx.dtypes[0]), None if g_th is None else g_th.to(ctx.dtypes[1])) + g_b + (None,)


def _cost_term(g: torch.Tensor, good: torch.Tensor, shared: bool) -> torch.Tensor:
    """A per-instance cost gradient g [B, n_p] as a term of theta's gradient: rows outside ``good`` selected out (not multiplied),
    summed over the batch for a shared theta."""
    g = torch.where(good.reshape(-1, 1), g, torch.zeros_like(g))
    return g.sum(0) if shared else g


class MPCCostFunction(torch.autograd.Function):
    """``MPCFunction`` / ``MPCBoundedFunction`` of a layer with ``cost_gradient=True``: (x0, theta, layer[, lb0, ub0, lb, ub, lbe, ube])
    -> (u0, V).  theta's gradient gets, on the cost block, g_V dV/dcost (``MPCBatch.cost_value_grad``) plus one ``MPCBatch.cost_vjp``
    with g_u as the cotangent on stage 0 of U*; when bounds need a gradient that same call serves them."""

    @staticmethod
    def forward(ctx, x0, theta, layer, *bounds):
        mpc: MPCBatch = layer.batch
        need_x, need_p, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3:9]
        if bounds:
            _apply_bounds(mpc, bounds)
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), sens_v=need_p, sens_pi=need_p, **layer.solve_args)
        s = mpc.state_sens(q_mode=False, value=True, policy=layer.has_policy_jacobian) if need_x else None
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.layer, ctx.pass_id = layer, layer.pass_counter
        ctx.shared = theta.dim() == 1
        ctx.dtypes, ctx.like = (x0.dtype, theta.dtype), tuple((b.device, b.dtype) for b in bounds)
        ctx.policy = layer.has_policy_jacobian
        ctx.jac = (r.status, None if s is None else s.dpi_dx0, None if s is None else s.dV_dx0, r.dpi_dp, r.dV_dp)
        ctx.dV_db = mpc.bound_value_grad(q_mode=False) if any(need_b) else None
        ctx.dV_dc = mpc.cost_value_grad() if need_p else None
        return r.u0.to(x0.dtype), r.V.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_u, g_V):
        status, du_dx0, dV_dx0, du_dp, dV_dp = ctx.jac
        need_p, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[3:9]
        if g_u is not None and ctx.needs_input_grad[0] and not ctx.policy:
            raise RuntimeError("MPCLayer: the loss depends on u0 and x0 requires a gradient, but du0*/dx0 is not available: build the layer "
                               "with policy_jacobian=True, detach x0 or keep u0 out of the loss.")
        f64 = [None if g is None else g.to(torch.float64) for g in (g_u, g_V)]
        g_x0, g_th = mpc_backward_terms(f64[0], f64[1], status, du_dx0, dV_dx0, du_dp, dV_dp, ctx.shared)
        g_b = (None,) * len(need_b)
        if (need_p or any(need_b)) and (g_u is not None or g_V is not None):
            mpc = ctx.layer.batch
            g_lb = g_ub = g_c = None
            if g_u is not None:
                _stale(ctx, "forward")
                gU = torch.zeros((mpc.B, mpc.N, mpc.nu), dtype=torch.float64, device=f64[0].device)
                gU[:, 0] = f64[0]
                g_lb, g_ub, g_c = mpc.cost_vjp(None, gU, x0=False, theta=False, bounds=any(need_b), cost=need_p)[2:]
            if g_V is not None:
                if any(need_b):
                    dlb, dub = (f64[1].reshape(-1, 1, 1) * d for d in ctx.dV_db)
                    g_lb, g_ub = (dlb, dub) if g_lb is None else (g_lb + dlb, g_ub + dub)
                if need_p:
                    dc = f64[1].reshape(-1, 1) * ctx.dV_dc
                    g_c = dc if g_c is None else g_c + dc
            if any(need_b):
                g_b = _bound_grads(mpc, g_lb, g_ub, status == 0, need_b, ctx.like)
            if need_p:
                g_th = g_th + _cost_term(g_c, status == 0, ctx.shared)
        return (None if g_x0 is None or not ctx.needs_input_grad[0] else g_x0.to(ctx.dtypes[0]),
                None if g_th is None or not need_p else g_th.to(ctx.dtypes[1]), None) + g_b


class MPCCostTrajectoryFunction(torch.autograd.Function):
    """``MPCTrajectoryFunction`` / ``MPCBoundedTrajectoryFunction`` of a layer with ``cost_gradient=True``: (x0, theta, layer[, lb0, ub0,
    lb, ub, lbe, ube]) -> (X, U); ``backward`` is ONE ``MPCBatch.cost_vjp`` for everything that requires a gradient, and theta's
    gradient is g_theta + g_cost."""

    @staticmethod
    def forward(ctx, x0, theta, layer, *bounds):
        mpc = layer.batch
        if bounds:
            _apply_bounds(mpc, bounds)
        mpc.set_theta(theta.detach().to(torch.float64))
        r = mpc.solve(x0.detach().to(torch.float64), **layer.solve_args)
        X, U = mpc.get_iterate()[:2]
        layer.last_status = r.status
        ctx.set_materialize_grads(False)
        ctx.layer, ctx.pass_id, ctx.status = layer, layer.pass_counter, r.status
        ctx.shared = theta.dim() == 1
        ctx.dtypes, ctx.like = (x0.dtype, theta.dtype), tuple((b.device, b.dtype) for b in bounds)
        return X.to(x0.dtype), U.to(x0.dtype)

    @staticmethod
    def backward(ctx, g_X, g_U):
        need_x, need_p, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3:9]
        if (g_X is None and g_U is None) or not (need_x or need_p or any(need_b)):
            return (None,) * (3 + len(need_b))
        _stale(ctx, "trajectory")
        mpc = ctx.layer.batch
        g_x0, g_th, g_lb, g_ub, g_c = mpc.cost_vjp(None if g_X is None else g_X.to(torch.float64), None if g_U is None else g_U.to(torch.float64),
                                                   x0=need_x, theta=need_p, bounds=any(need_b), cost=need_p)
        if g_th is not None:      # (cost_vjp has selected the rows of instances with a status other than 0 out of both)
            g_th = g_th + g_c
            if ctx.shared:
                g_th = g_th.sum(0)
        g_b = _bound_grads(mpc, g_lb, g_ub, torch.ones_like(ctx.status, dtype=torch.bool), need_b, ctx.like) if any(need_b) else (None,) * len(need_b)
        return (None if g_x0 is None else g_x0.to(ctx.dtypes[0]), None if g_th is None else g_th.to(ctx.dtypes[1]), None) + g_b


class MPCLayer(torch.nn.Module):
    """``layer(x0, theta) -> (u0, V)``, ``layer.q(x0, u0, theta) -> Q`` and ``layer.trajectory(x0, theta) -> (X, U)`` around one
    ``MPCBatch`` (its batch size is the layer's).  ``pass_counter``: incremented by each of the three (the staleness rule of
    ``trajectory``'s backward pass, see the module's docstring).
    ``policy_jacobian``: whether ``forward`` computes du0*/dx0 when ``x0`` needs a gradient — None = on for the cartpole and the linear
    system, off for the chain of masses (where it costs up to three more launches per forward pass); True / False = on / off on any
    model.  ``solve_args`` go to every ``MPCBatch.solve`` of the layer (e.g. ``cold=True``).  ``last_status`` [B] int32: the statuses
    of the last forward pass.
    ``cost_gradient`` (cartpole only, ValueError otherwise; off by default): ``theta.grad`` also carries the cost block, entries
    3 .. 82 of p, each an independent variable (include/mpcrl_cost_ext.h, see the module's docstring)."""

    def __init__(self, batch: MPCBatch, policy_jacobian: Optional[bool] = None, cost_gradient: bool = False, **solve_args):
        super().__init__()
        if cost_gradient and batch.ocp.name != "cartpole":
            raise ValueError("MPCLayer: cost_gradient=True is for the cartpole (the linear system keeps its weights in consts, the chain "
                             f"has Q, R in its parameter gradient already), not for {batch.ocp.name!r}")
        self.cost_gradient = bool(cost_gradient)
        self.batch = batch
        self.solve_args = solve_args
        self.has_policy_jacobian = (not batch.ocp.name.startswith("chain")) if policy_jacobian is None else bool(policy_jacobian)
        self.last_status = None
        self.pass_counter = 0

    def forward(self, x0: torch.Tensor, theta: torch.Tensor, bounds: Optional[BoxBounds] = None):
        """``bounds``: a BoxBounds whose members may require a gradient (a host synchronisation per call, see the module's docstring);
        None = the bounds the batch has, as constants."""
        self.pass_counter += 1
        if self.cost_gradient:
            return MPCCostFunction.apply(x0, theta, self, *(() if bounds is None else BoxBounds(*bounds)))
        if bounds is None:
            return MPCFunction.apply(x0, theta, self)
        return MPCBoundedFunction.apply(x0, theta, *BoxBounds(*bounds), self)

    def q(self, x0: torch.Tensor, u0: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
        self.pass_counter += 1
        return MPCQFunction.apply(x0, u0, theta, self)

    def trajectory(self, x0: torch.Tensor, theta: torch.Tensor, bounds: Optional[BoxBounds] = None):
        """``bounds``: as in ``forward``."""
        self.pass_counter += 1
        if self.cost_gradient:
            return MPCCostTrajectoryFunction.apply(x0, theta, self, *(() if bounds is None else BoxBounds(*bounds)))
        if bounds is None:
            return MPCTrajectoryFunction.apply(x0, theta, self)
        return MPCBoundedTrajectoryFunction.apply(x0, theta, *BoxBounds(*bounds), self)
