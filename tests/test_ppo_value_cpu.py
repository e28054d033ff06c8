"""CPU checks of PPO's value function as library kernels (csrc/value_kernel.hpp, mpc4rl_amd/ppo.py): the C ABI's three new symbols, the
torch statement of the gradient kernel against torch autograd of vf_coef x mse_loss and its rule for the rows that are left out, and
the policy's argument checks for value_kernels=True."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcrl_value_forward", "mpcrl_value_workspace_bytes", "mpcrl_value_mse_grad"]


def test_new_symbols_in_header_binding_and_library_abi_still_132():
    """The three value-function symbols are declared, bound and exported; they are additions, so header and binding still say 132."""
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.EXPORTS, name
    assert int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 132
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    lib.mpcrl_version.restype = ctypes.c_int
    assert lib.mpcrl_version() == 132
    # argument checks that need no device: the workspace size and its refusals
    lib.mpcrl_value_workspace_bytes.restype = ctypes.c_int64
    lib.mpcrl_value_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    assert lib.mpcrl_value_workspace_bytes(17, 4) == 2 * (64 * 4 + 4289 + 2) * 8          # two workgroups of 16 rows, double partials
    assert lib.mpcrl_value_workspace_bytes(4096, 16) == 256 * (64 * 16 + 4289 + 2) * 8
    for M, nx in ((0, 4), (-1, 4), (16, 0), (16, 17)):
        assert lib.mpcrl_value_workspace_bytes(M, nx) < 0


def _net(nx, seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(nx, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).double()


def _tables(n_rows, nx, seed):
    """float64 tables whose entries are float32 numbers (the kernel rounds its inputs to float32 on load; here that changes nothing)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n_rows, nx, generator=g).double(), (3.0 * torch.randn(n_rows, generator=g) - 5.0).double())


def test_value_terms_match_autograd_of_mse_loss():
    from mpc4rl_amd import ppo_value_terms
    nx, n_rows, M, vf = 4, 40, 24, 0.5
    net = _net(nx, 0)
    OBS, RET = _tables(n_rows, nx, 1)
    idx = torch.randint(0, n_rows, (M,), generator=torch.Generator().manual_seed(2))
    assert idx.unique().numel() < M                                    # drawn with repeats
    loss, count, grad = ppo_value_terms(OBS.reshape(5, 8, nx), RET.reshape(5, 8), idx, net, vf)      # [T, E] tables are flattened
    ref_loss = vf * torch.nn.functional.mse_loss(net(OBS[idx]).reshape(M), RET[idx])
    ref = torch.cat([g.reshape(-1) for g in torch.autograd.grad(ref_loss, list(net.parameters()))])
    assert int(count) == M and grad.shape == (64 * nx + 4289,)
    assert float((grad - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert abs(float(loss) - float(ref_loss.detach())) <= 1e-12 * float(ref_loss.detach())
    assert all(p.grad is None for p in net.parameters())               # autograd.grad: the module's .grad is not touched


def test_value_terms_leave_out_poisoned_rows_and_indices_outside_the_table():
    from mpc4rl_amd import ppo_value_terms
    nx, n_rows, M, vf = 4, 40, 24, 0.5
    net = _net(nx, 3)
    OBS, RET = _tables(n_rows, nx, 4)
    idx = torch.arange(M)                                              # distinct rows, so that each poisoned row is sampled once
    full = ppo_value_terms(OBS, RET, idx, net, vf)
    assert int(full[1]) == M
    OBS, RET, idx = OBS.clone(), RET.clone(), idx.clone()
    OBS[5, 2], RET[9] = float("nan"), float("inf")
    idx[0], idx[1] = -1, n_rows
    loss, count, grad = ppo_value_terms(OBS, RET, idx, net, vf)
    assert int(count) == M - 4 and torch.isfinite(grad).all() and torch.isfinite(loss)
    keep = torch.tensor([b for b in range(2, M) if b not in (5, 9)])
    ref_loss = vf * torch.nn.functional.mse_loss(net(OBS[keep]).reshape(-1), RET[keep])
    ref = torch.cat([g.reshape(-1) for g in torch.autograd.grad(ref_loss, list(net.parameters()))])
    assert float((grad - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert abs(float(loss) - float(ref_loss.detach())) <= 1e-12 * float(ref_loss.detach())
    # nothing valid: zero loss, zero gradient, count 0
    loss0, count0, grad0 = ppo_value_terms(torch.full_like(OBS, float("nan")), RET, idx, net, vf)
    assert int(count0) == 0 and float(loss0) == 0.0 and float(grad0.abs().max()) == 0.0


def test_value_terms_in_float32_round_the_tables_first():
    """Any dtype of the network: the float32 copy gets float32 inputs, and agrees with the float64 statement to float32 rounding."""
    from mpc4rl_amd import ppo_value_terms
    nx, n_rows, M = 3, 30, 16
    net = _net(nx, 5)
    OBS, RET = torch.randn(n_rows, nx, dtype=torch.float64), torch.randn(n_rows, dtype=torch.float64)      # not float32 numbers
    idx = torch.randint(0, n_rows, (M,))
    l64, n64, g64 = ppo_value_terms(OBS, RET, idx, net, 0.5)
    l32, n32, g32 = ppo_value_terms(OBS, RET, idx, copy.deepcopy(net).float(), 0.5)
    assert g32.dtype == torch.float32 and int(n32) == int(n64) == M
    assert float((g32.double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    lr, _, gr = ppo_value_terms(OBS.float().double(), RET.float().double(), idx, net, 0.5)
    assert torch.equal(gr, g64) and torch.equal(lr, l64)


@pytest.mark.parametrize("kw", [dict(net_arch=(32, 32)), dict(activation_fn=nn.ReLU), dict(net_arch=(64, 64, 64)), dict(obs=17)])
def test_value_kernels_argument_checks(kw):
    """value_kernels=True is written for 64 x 64 tanh and at most 16 observations: anything else is refused before a device is touched."""
    from mpc4rl_amd import MPCActorCriticPolicy, cartpole_ocp

    class Box:
        def __init__(self, n):
            self.shape = (n,)

    kw = dict(kw)
    obs = kw.pop("obs", 4)
    with pytest.raises(ValueError, match="value_kernels"):
        MPCActorCriticPolicy(Box(obs), Box(1), lambda _: 3e-4, cartpole_ocp(), batch=4, value_kernels=True, **kw)
