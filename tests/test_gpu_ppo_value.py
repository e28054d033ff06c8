"""GPU tests of PPO's value function as library kernels (csrc/value_kernel.hpp, BatchedPPO(value_kernels=True)).

The yardstick everywhere is the float64 evaluation of the same network (copy.deepcopy(net).double()) on the inputs the kernels see
(the float64 tables rounded to float32): the kernels must be as close to it as torch's own float32 path is.  With err_k and err_t the
max-abs errors of kernel and torch-float32 against float64, divided by the largest float64 entry, the bound is
    err_k <= max(4 err_t, 2**-22)
— the rule of test_critic_td_grad_and_dq_da_vs_autograd with a floor of two float32 ulps of the largest entry, so that a lucky err_t
cannot fail a correct kernel.  Both errors are printed."""
import copy
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
FLOOR = 2.0 ** -22
E_ARG = -1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def _net(nx, seed):
    """the network MPCActorCriticPolicy builds by default, its parameters views of one flat buffer"""
    from mpc4rl_amd.td3 import flatten_parameters
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(nx, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(DEV)
    flat, _ = flatten_parameters(net)
    assert flat.numel() == 64 * nx + 4289
    return net, flat


def _errs(got, ref32, ref64):
    scale = float(ref64.abs().max())
    return float((got.double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale


def _within(err_k, err_t):
    return err_k <= max(4.0 * err_t, FLOOR)


# ---------------------------------------------------------------------- forward
@pytest.mark.parametrize("n,nx", [(1, 4), (63, 4), (64, 4), (65, 4), (1000, 4), (65, 1), (65, 16)])
def test_value_forward_vs_float64(n, nx):
    lib = _lib()
    net, flat = _net(nx, 7 * n + nx)
    obs = 2.0 * torch.randn(n, nx, **F64)
    out = torch.full((n + 3,), -7.0, **F64)
    assert lib.mpcrl_value_forward(_p(obs), n, nx, _p(flat), _p(out), _stream()) == 0
    with torch.no_grad():
        y64 = copy.deepcopy(net).double()(obs.float().double()).reshape(n)
        y32 = net(obs.float()).reshape(n)
    err_k, err_t = _errs(out[:n], y32, y64)
    print(f"forward n {n} nx {nx}: against float64 — kernel {err_k:.2e}, torch float32 {err_t:.2e}")
    assert _within(err_k, err_t)
    assert bool((out[n:] == -7.0).all())
    # the same call again: the same bits
    out2 = torch.zeros_like(out)
    assert lib.mpcrl_value_forward(_p(obs), n, nx, _p(flat), _p(out2), _stream()) == 0
    assert torch.equal(out2[:n], out[:n])
    # one row of NaN: a non-finite value in that row only
    r = n // 2
    bad = obs.clone()
    bad[r] = float("nan")
    out3 = torch.zeros_like(out)
    assert lib.mpcrl_value_forward(_p(bad), n, nx, _p(flat), _p(out3), _stream()) == 0
    keep = torch.arange(n, device=DEV) != r
    assert not math.isfinite(float(out3[r])) and torch.equal(out3[:n][keep], out[:n][keep])


def test_value_forward_argument_checks():
    lib = _lib()
    _, flat = _net(16, 0)
    obs, out = torch.zeros(8, 17, **F64), torch.zeros(8, **F64)
    for nx in (0, 17):
        assert lib.mpcrl_value_forward(_p(obs), 8, nx, _p(flat), _p(out), _stream()) == E_ARG
    assert lib.mpcrl_value_forward(None, 8, 4, _p(flat), _p(out), _stream()) == E_ARG
    assert lib.mpcrl_value_forward(_p(obs), -1, 4, _p(flat), _p(out), _stream()) == E_ARG
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ---------------------------------------------------------------------- gradient
def _grad_case(M, nx):
    """Tables of 3 M + 5 rows, idx drawn with repeats; with M > 4 a NaN OBS entry on one sampled row, an inf RET on another, one index
    -1 and one index n_rows."""
    g = torch.Generator(device=DEV).manual_seed(1000 * nx + M)
    n_rows = 3 * M + 5
    OBS = 1.5 * torch.randn(n_rows, nx, generator=g, **F64)
    RET = 3.0 * torch.randn(n_rows, generator=g, **F64) - 5.0
    idx = torch.randint(0, n_rows, (M,), generator=g, device=DEV)
    if M > 4:
        idx[M - 1] = idx[M - 2]                                        # a repeat, whatever the draw
        idx[0], idx[1] = -1, n_rows
        OBS[idx[2], nx - 1] = float("nan")
        RET[idx[3]] = float("inf")
    return OBS, RET, idx, n_rows


def _mse_grad(lib, OBS, RET, idx, n_rows, nx, flat, vf, scale, ws, out):
    return lib.mpcrl_value_mse_grad(_p(OBS), _p(RET), _p(idx), idx.numel(), n_rows, nx, _p(flat), vf, scale, _p(ws), _p(out), _stream())


@pytest.mark.parametrize("M,nx", [(1, 4), (15, 4), (16, 4), (17, 4), (257, 4), (4096, 4), (50, 1), (50, 16)])
def test_value_mse_grad_vs_float64(M, nx):
    from mpc4rl_amd import ppo_value_terms
    lib = _lib()
    net, flat = _net(nx, M + nx)
    n_p, vf = flat.numel(), 0.5
    OBS, RET, idx, n_rows = _grad_case(M, nx)
    nb = int(lib.mpcrl_value_workspace_bytes(M, nx))
    assert nb == ((M + 15) // 16) * (n_p + 2) * 8
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((n_p + 2 + 5,), -1.0, **F64)
    assert _mse_grad(lib, OBS, RET, idx, n_rows, nx, flat, vf, 0.5, ws, out) == 0
    l64, n64, g64 = ppo_value_terms(OBS, RET, idx, copy.deepcopy(net).double(), vf)
    l32, n32, g32 = ppo_value_terms(OBS, RET, idx, net, vf)
    # (M > 4: at least the four poisoned positions are out; a poisoned row that was drawn twice takes its twin along)
    assert int(n64) == int(n32) and (int(n64) == M if M <= 4 else 0 < int(n64) <= M - 4)
    assert float(out[n_p + 1]) == float(n64)
    err_k, err_t = _errs(2.0 * out[:n_p], g32, g64)
    lerr_k, lerr_t = _errs(out[n_p:n_p + 1], l32.reshape(1), l64.reshape(1))
    print(f"M {M} nx {nx}: gradient against float64 — kernels {err_k:.2e}, torch float32 {err_t:.2e}; loss — kernels {lerr_k:.2e}, torch float32 {lerr_t:.2e}; "
          f"count {int(n64)}")
    assert _within(lerr_k, lerr_t)
    assert _within(err_k, err_t)
    assert bool((out[n_p + 2:] == -1.0).all())
    # the same call again, the workspace full of 0xFF bytes beforehand: the same bits
    ws.fill_(0xFF)
    out2 = torch.zeros_like(out)
    assert _mse_grad(lib, OBS, RET, idx, n_rows, nx, flat, vf, 0.5, ws, out2) == 0
    assert torch.equal(out2[:n_p + 2], out[:n_p + 2])
    # every row invalid: zero gradient, zero loss, count 0
    ws.fill_(0xFF)
    out3 = torch.full_like(out, -1.0)
    assert _mse_grad(lib, torch.full_like(OBS, float("nan")), RET, idx, n_rows, nx, flat, vf, 0.5, ws, out3) == 0
    assert float(out3[:n_p + 2].abs().max()) == 0.0 and bool((out3[n_p + 2:] == -1.0).all())


def test_value_mse_grad_argument_checks():
    lib = _lib()
    nx, M = 4, 16
    _, flat = _net(nx, 0)
    OBS, RET, idx, n_rows = _grad_case(M, nx)
    ws = torch.zeros(int(lib.mpcrl_value_workspace_bytes(M, nx)), dtype=torch.uint8, device=DEV)
    out = torch.zeros(flat.numel() + 2, **F64)
    ptrs = [OBS, RET, idx, flat, ws, out]
    for k in range(len(ptrs)):                                             # a NULL pointer, each in turn
        a = [None if i == k else t for i, t in enumerate(ptrs)]
        assert lib.mpcrl_value_mse_grad(_p(a[0]), _p(a[1]), _p(a[2]), M, n_rows, nx, _p(a[3]), 0.5, 1.0, _p(a[4]), _p(a[5]), _stream()) == E_ARG
    call = lambda M_, rows_, nx_: lib.mpcrl_value_mse_grad(_p(OBS), _p(RET), _p(idx), M_, rows_, nx_, _p(flat), 0.5, 1.0, _p(ws), _p(out), _stream())  # noqa: E731
    assert call(0, n_rows, nx) == E_ARG and call(-3, n_rows, nx) == E_ARG and call(M, -1, nx) == E_ARG
    assert call(M, n_rows, 0) == E_ARG and call(M, n_rows, 17) == E_ARG
    assert lib.mpcrl_value_workspace_bytes(0, nx) == E_ARG and lib.mpcrl_value_workspace_bytes(M, 17) == E_ARG
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    # an empty table is no misuse: every index is outside it
    assert call(M, 0, nx) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def test_value_mse_grad_in_a_captured_graph():
    """The gradient call captured on one stream and replayed twice: the eager call's bits."""
    lib = _lib()
    M, nx = 257, 4
    _, flat = _net(nx, 5)
    OBS, RET, idx, n_rows = _grad_case(M, nx)
    ws = torch.zeros(int(lib.mpcrl_value_workspace_bytes(M, nx)), dtype=torch.uint8, device=DEV)
    eager, out = torch.zeros(flat.numel() + 2, **F64), torch.zeros(flat.numel() + 2, **F64)
    assert _mse_grad(lib, OBS, RET, idx, n_rows, nx, flat, 0.5, 1.0, ws, eager) == 0
    torch.cuda.synchronize()
    side, g = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = _mse_grad(lib, OBS, RET, idx, n_rows, nx, flat, 0.5, 1.0, ws, out)
    assert rc == 0
    for _ in range(2):
        out.zero_()
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and float(eager[:-2].abs().max()) > 0.0


# ---------------------------------------------------------------------- the loop
def _learner(value_kernels):
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedPPO, cartpole_ocp
    env = BatchedCartPoleSwingUpEnv(128, device=DEV, seed=3)
    return BatchedPPO(cartpole_ocp(), env, n_steps=4, batch_size=256, n_epochs=2, lr=1e-4, ent_coef=0.01, log_std_init=-1.0, seed=11,
                      value_kernels=value_kernels)


def _flat_of(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def _is_view_of(t, flat):
    return t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and t.dtype == flat.dtype


def test_loop_with_value_kernels_against_the_framework_path():
    """Two learners, the same seeds, value_kernels on / off: the roll-out does not see the value function, VAL / VNEXT agree with the
    float64 evaluation as well as torch's float32 path does, and the first Adam step moves the value parameters alike:
    max |p_on - p_off| <= 2 lr_value dg / eps_adam + 2**-22 with dg the largest difference of the two flat gradients (the first
    bias-corrected Adam step is lr g / (|g| + eps), whose slope in g is at most 1 / eps; the 2 covers float32 rounding of the update)."""
    on, off = _learner(True), _learner(False)
    pol = on.policy
    assert torch.equal(pol.value_flat, _flat_of(off.policy.value_net))
    assert all(_is_view_of(p.data, pol.value_flat) and _is_view_of(p.grad, pol.value_grad_flat) for p in pol.value_net.parameters())
    v = pol.predict_values(on.obs)
    assert v.shape == (128, 1) and v.dtype == torch.float64 and not v.requires_grad
    on.collect(), off.collect()
    torch.cuda.synchronize()
    for name in ("OBS", "ACT", "LOGP", "REW", "NEXT", "TERM", "DONE", "OK"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    net64 = copy.deepcopy(off.policy.value_net).double()
    for name, src in (("VAL", "OBS"), ("VNEXT", "NEXT")):
        with torch.no_grad():
            y64 = net64(getattr(off, src).reshape(-1, 4).float().double()).reshape(4, 128)
        err_k, err_t = _errs(getattr(on, name), getattr(off, name), y64)
        print(f"{name}: against float64 — kernel {err_k:.2e}, torch float32 {err_t:.2e}")
        assert _within(err_k, err_t), name
    idx = torch.randperm(4 * 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))[:256].contiguous()
    on._minibatch(idx), off._minibatch(idx)
    torch.cuda.synchronize()
    g_on = pol.value_grad_flat
    g_off = torch.cat([p.grad.reshape(-1) for p in off.policy.value_net.parameters()])
    p_off = _flat_of(off.policy.value_net)
    dg = float((g_on - g_off).abs().max())
    dp = float((pol.value_flat - p_off).abs().max())
    lr_value, eps_adam = off.policy.optimizer.param_groups[0]["lr"], off.policy.optimizer.param_groups[0]["eps"]
    print(f"first value step: largest gradient difference {dg:.2e} (largest entry {float(g_off.abs().max()):.2e}), largest parameter difference {dp:.2e}, "
          f"bound {2.0 * float(lr_value) * dg / eps_adam + FLOOR:.2e}")
    assert float(g_off.abs().max()) > 0.0 and float((pol.value_flat - _flat_of(net64).float()).abs().max()) > 0.0      # a step was taken
    assert dp <= 2.0 * float(lr_value) * dg / eps_adam + FLOOR
    s_on, s_off = on.last_stats(), off.last_stats()
    # value_loss is the same quantity on both paths (the last minibatch's loss / vf_coef) from float32 values that differ in their last
    # bits: a check of the definition, not of precision
    assert math.isfinite(s_on["value_loss"]) and math.isclose(s_on["value_loss"], s_off["value_loss"], rel_tol=1e-3)


def test_two_learn_iterations_with_value_kernels_are_finite_and_reproducible():
    outs = []
    for _ in range(2):
        ppo = _learner(True)
        th0, v0 = ppo.theta.clone(), ppo.policy.value_flat.clone()
        ppo.learn(2)
        st = ppo.last_stats()
        torch.cuda.synchronize()
        pol = ppo.policy
        outs.append((ppo.theta.clone(), ppo.log_std.clone(), pol.value_flat.clone(), st))
        assert torch.isfinite(ppo.theta).all() and torch.isfinite(ppo.log_std).all() and all(math.isfinite(x) for x in st.values())
        assert "value_loss" in st and st["value_loss"] > 0.0
        assert torch.isfinite(ppo.ADV).all() and torch.isfinite(ppo.RET).all() and torch.isfinite(pol.value_flat).all()
        assert float((ppo.theta - th0)[:3].abs().max()) > 0.0 and torch.equal(ppo.theta[3:], th0[3:]) and float(ppo.log_std) != -1.0
        assert float((pol.value_flat - v0).abs().max()) > 0.0
        assert all(_is_view_of(p.data, pol.value_flat) and _is_view_of(p.grad, pol.value_grad_flat) for p in pol.value_net.parameters())
        assert ppo.iterations == 2
    print("PPO statistics after two iterations, value kernels:", outs[0][3])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3]
