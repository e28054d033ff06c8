"""CPU checks of the batched cartpole Q-learning loop: the C ABI's new symbols, the TD step's torch statement against a per-environment
loop written from scripts/cartpole_mpc_qlearning.py:236-263, and the constructor's argument checks."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcrl_qlearning_cartpole_collect", "mpcrl_qlearning_td_workspace_bytes", "mpcrl_qlearning_td_grad", "mpcrl_qlearning_apply"]


def test_new_symbols_in_header_and_binding_abi132():
    """The Q-learning symbols are declared and bound; header and binding agree on ABI 132 (mpcrl_td3_policy_post selects masked
    entries out)."""
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.EXPORTS, name
    assert int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 132


def _script_loop(q, v, dq, sq, sv, cost, L, gamma, lr):
    """The reference's learning sweep per environment: n = size - 1 samples, td = cost[:-1] + GAMMA v[1:] - q[:-1], dp_i = LR td_i dQ_dp_i
    over i < n - 1, with a term kept only where the four solves it reads succeeded; returns the sums the message carries."""
    n_p = dq.shape[-1]
    g, ws, cnt = np.zeros(n_p), 0.0, 0
    tds = {}
    for e in range(len(L)):
        n = int(L[e]) - 1
        if n < 2:
            continue
        c, qq, vv = cost[:n, e], q[:n, e], v[:n, e]
        td = c[:-1] + gamma * vv[1:] - qq[:-1]
        for i in range(n - 1):
            if sq[i, e] == 0 and sv[i, e] == 0 and sq[i + 1, e] == 0 and sv[i + 1, e] == 0:
                g += lr * td[i] * dq[i, e]
                ws += lr * td[i]
                cnt += 1
                tds[(i, e)] = td[i]
    return g, ws, cnt, tds


@pytest.mark.parametrize("T", [2, 3, 7, 12])
def test_td_terms_match_per_environment_loop(T):
    from mpc4rl_amd import qlearning_td_terms
    rng = np.random.default_rng(T)
    E, n_p, gamma, lr = 2 * T + 3, 5, 0.99, 1e-3
    L = np.concatenate([np.arange(T + 1), rng.integers(0, T + 1, E - T - 1)])     # every length 0 ... T, then random ones
    live = (np.arange(T)[:, None] < L[None, :]).astype(np.uint8)
    cost = rng.uniform(0, 5, (T, E)) * live
    q, v = rng.normal(size=(T - 1, E)), rng.normal(size=(T - 1, E))
    dq = rng.normal(size=(T - 1, E, n_p))
    sq = np.where(rng.uniform(size=(T - 1, E)) < 0.15, 2, 0).astype(np.int32)
    sv = np.where(rng.uniform(size=(T - 1, E)) < 0.1, 4, 0).astype(np.int32)
    q[sq != 0], v[sv != 0] = np.nan, np.nan                    # a failed solve may leave NaN: it must never reach the sums
    dq[sq != 0] = np.nan
    msg, td, valid = qlearning_td_terms(*[torch.as_tensor(a) for a in (q, v, dq, sq, sv, cost, live)], gamma, lr)
    g, ws, cnt, tds = _script_loop(q, v, dq, sq, sv, cost, L, gamma, lr)
    assert msg.shape == (n_p + 2,) and td.shape == (max(T - 2, 0), E) and valid.shape == td.shape
    assert torch.isfinite(msg).all() and torch.isfinite(td).all()
    assert int(msg[-1]) == cnt == int(valid.sum())
    np.testing.assert_allclose(msg[:n_p].numpy(), g, rtol=1e-12, atol=1e-15)
    assert math.isclose(float(msg[n_p]), ws, rel_tol=1e-12, abs_tol=1e-15)
    got = {(int(i), int(e)) for i, e in zip(*np.nonzero(valid.numpy()))}
    assert got == set(tds)
    for (i, e), t in tds.items():
        assert math.isclose(float(td[i, e]), t, rel_tol=1e-14, abs_tol=0.0)
    assert float(td[~valid].abs().sum()) == 0.0


def test_constructor_argument_checks():
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedLinearSystemEnv, CartpoleQLearning, cartpole_ocp, linear_system_ocp
    ocp, env = cartpole_ocp(), BatchedCartPoleSwingUpEnv(4, device="cpu")
    with pytest.raises(ValueError):
        CartpoleQLearning(linear_system_ocp(), env, 10)
    with pytest.raises(TypeError):
        CartpoleQLearning(ocp, BatchedLinearSystemEnv(4, device="cpu"), 10)
    for kw in (dict(episode_length=1), dict(episode_length=2.0), dict(episode_length=10, lr=float("nan")),
               dict(episode_length=10, gamma=0.0), dict(episode_length=10, gamma=1.5), dict(episode_length=10, noise_scale=-0.1),
               dict(episode_length=10, noise_scale=float("inf"))):
        with pytest.raises(ValueError):
            CartpoleQLearning(ocp, env, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # valid arguments, CPU environment: refused, never emulated
        CartpoleQLearning(ocp, env, 10)
