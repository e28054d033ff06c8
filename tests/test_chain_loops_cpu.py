"""CPU checks of the chain of masses as a plant and of its Q-learning loop (csrc/chain_env_kernel.hpp, mpc4rl_amd/envs.py
BatchedChainMassEnv, mpc4rl_amd/qlearning_chain.py): the C ABI's two new symbols and their argument checks, the torch statement of the plant
against the oracle's chain model, the environment's CPU path, the constructors' argument checks, and the one-control learners' class
attributes after the generalisation of DeviceQLearning to NU controls.

The bar of the statement against the oracle is 1e-13, every entry scaled by max(1, |reference|): the two are the same map with its sums
associated differently (the statement follows the kernel's grouping), a few hundred operations deep, and differ by a few unit roundoffs
(2.2e-16)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcrl_env_chain_step", "mpcrl_qlearning_chain_collect"]
F64 = dict(dtype=torch.float64)


def _n_p(n_mass):
    from mpc4rl_amd.problems import chain_param_layout
    return chain_param_layout(n_mass)[5]


def test_new_symbols_in_header_binding_and_library():
    """Both symbols are declared, bound and exported, the binding's version is the library's, and every argument error of the two exports
    is MPCRL_E_ARG before any launch (no pointer below is device memory: a call that got as far as its launch could not return -1 for the
    argument alone); B = 0 and E = 0 return 0 without a launch."""
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.EXPORTS, name
    assert "ocp_utils.py:76-130" in hdr.split("#ifndef MPCRL_H")[0]             # the header table's row
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    lib.mpcrl_version.restype = ctypes.c_int
    assert lib.mpcrl_version() == _lib.ABI_VERSION == int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1))
    vp, ci, cd, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
    lib.mpcrl_env_chain_step.argtypes = [ci, cd, ci, vp, i64, vp, ci, vp, vp, vp, cd, vp, ci, vp, vp]
    lib.mpcrl_qlearning_chain_collect.argtypes = [ci, cd, ci, vp, i64, vp, cd, ci, ci] + [vp] * 7 + [cd] + [vp] * 7
    buf = (ctypes.c_double * 8)()          # never read: every call below returns before its launch
    p = ctypes.cast(buf, vp)
    lo, hi = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def step(n_mass=5, Ts=0.2, rk=2, stride=0, B=0, w_std=0.0, null=()):
        ptr = {k: (None if k in null else p) for k in ("p", "x_ss", "state", "action", "wn", "obs", "cost")}
        return lib.mpcrl_env_chain_step(n_mass, Ts, rk, ptr["p"], stride, ptr["x_ss"], B, ptr["state"], ptr["action"], ptr["wn"], w_std, ptr["obs"], 0,
                                        ptr["cost"], None)

    names = ("state", "u0", "status", "eps", "wn", "lo", "hi", "obs", "row", "cold", "S", "A", "C")

    def coll(n_mass=5, Ts=0.2, rk=2, stride=0, E=0, T=3, w_std=0.0, null=(), lo=lo, hi=hi, sigma=0.0):
        ptr = {k: (None if k in null else p) for k in ("p", "x_ss") + names}
        ptr["lo"], ptr["hi"] = (None if "lo" in null else lo), (None if "hi" in null else hi)
        return lib.mpcrl_qlearning_chain_collect(n_mass, Ts, rk, ptr["p"], stride, ptr["x_ss"], w_std, E, T, *[ptr[k] for k in names[:7]], sigma,
                                                 *[ptr[k] for k in names[7:]], None)

    for f in (step, coll):
        assert f() == 0                                                           # B = 0 / E = 0: nothing to do
        assert all(f(n_mass=n) == 0 for n in (3, 4, 5, 6, 7)) and all(f(n_mass=n) == -1 for n in (2, 8, 0, -1))
        assert f(rk=0) == -1 and f(rk=-1) == -1 and f(rk=1) == 0
        assert f(Ts=0.0) == -1 and f(Ts=-0.2) == -1 and f(Ts=float("nan")) == -1
        for n in (3, 5, 7):                                                       # 0 or this chain's n_p, nothing else
            assert f(n_mass=n, stride=_n_p(n)) == 0
            assert f(n_mass=n, stride=_n_p(n) - 1) == -1 and f(n_mass=n, stride=1) == -1 and f(n_mass=n, stride=-_n_p(n)) == -1
        assert f(n_mass=5, stride=_n_p(4)) == -1
        assert f(null=("p",)) == -1 and f(null=("x_ss",)) == -1
        assert f(null=("wn",)) == 0 and f(null=("wn",), w_std=0.05) == -1 and f(w_std=0.05) == 0      # wn: NULL only without noise
    assert step(B=-1) == -1 and all(step(null=(k,)) == -1 for k in ("state", "action", "cost")) and step(null=("obs",)) == 0
    assert coll(E=-1) == -1 and coll(T=0) == -1
    assert all(coll(null=(k,)) == -1 for k in names if k != "wn")
    assert coll(sigma=-0.1) == -1 and coll(sigma=float("nan")) == -1 and coll(sigma=float("inf")) == -1 and coll(sigma=0.3) == 0
    assert coll(hi=(ctypes.c_double * 3)(1.0, -1.0, 1.0)) == -1 and coll(lo=(ctypes.c_double * 3)(-1.0, -1.0, float("nan"))) == -1


def _random_points(n_mass, n, seed):
    """x0 + N(0, 0.05), u ~ U(-1, 1), dynamics parameters x U(0.8, 1.2), wn ~ N(0, 1) (w = 0.1 wn ~ N(0, 0.1))"""
    from mpc4rl_amd import chain_mass_ocp
    from mpc4rl_amd.problems import chain_param_layout
    ocp = chain_mass_ocp(n_mass, N=8)
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(ocp.x0) + 0.05 * torch.randn(n, nx, generator=g, **F64)
    u = torch.rand(n, 3, generator=g, **F64) * 2.0 - 1.0
    p = torch.tensor(ocp.p0).repeat(n, 1)
    nd = off["C"][1]                                                              # m, D, L, C
    p[:, :nd] *= 0.8 + 0.4 * torch.rand(n, nd, generator=g, **F64)
    wn = torch.randn(n, 3 * M, generator=g, **F64)
    return ocp, off, x, u, p, wn


@pytest.mark.parametrize("n_mass", [3, 5, 7])
def test_statement_equals_the_oracles_chain_model(n_mass):
    """chain_env_step_terms against oracle.problems.make_chain_mass(n_mass).F and .stage_cost at 20 random points with per-row parameters;
    the disturbance w_std * wn equals adding it to p's w."""
    from mpc4rl_amd import chain_env_step_terms
    from oracle.problems import make_chain_mass
    ocp, off, x, u, p, wn = _random_points(n_mass, 20, 10 + n_mass)
    prob = make_chain_mass(n_mass, N=8)
    x_ss = torch.tensor(ocp.consts)
    assert np.array_equal(ocp.p0, prob.p0) and float(np.abs(ocp.consts - prob.extra["x_ss"]).max()) < 1e-15
    new, cost = chain_env_step_terms(ocp, p, x_ss, x, u, wn, 0.1)
    pw = p.clone()
    pw[:, off["w"][0]: off["w"][1]] += 0.1 * wn
    ref = torch.stack([prob.F(x[i], u[i], pw[i]) for i in range(20)])
    ref_c = torch.stack([prob.stage_cost(0, x[i], u[i], pw[i]) for i in range(20)])
    e_x = float(((new - ref).abs() / ref.abs().clamp(min=1.0)).max())
    e_c = float(((cost - ref_c).abs() / ref_c.abs().clamp(min=1.0)).max())
    print(f"n_mass {n_mass}: new state {e_x:.3e}, cost {e_c:.3e}")
    assert e_x <= 1e-13 and e_c <= 1e-13
    assert float((new - x).abs().max()) > 1e-3 and float(cost.min()) > 0.0
    # the same through the parameters: w + noise inside the ODE; and the dims tuple, a shared p, no noise
    new_w, cost_w = chain_env_step_terms(ocp, pw, x_ss, x, u, None, 0.0)
    assert float(((new_w - new).abs() / new.abs().clamp(min=1.0)).max()) <= 1e-13 and torch.equal(cost_w, cost)
    assert float((chain_env_step_terms(ocp, p, x_ss, x, u, None, 0.0)[0] - new).abs().max()) > 1e-4            # the noise is felt
    one, c1 = chain_env_step_terms((n_mass, 0.2, 2), p[3], x_ss, x[3:4], u[3:4], wn[3:4], 0.1)
    assert torch.equal(one, new[3:4]) and torch.equal(c1, cost[3:4])
    coarse, _ = chain_env_step_terms((n_mass, 0.2, 1), p, x_ss, x, u, wn, 0.1)
    assert float((coarse - new).abs().max()) > 1e-6                              # rk_steps is honoured: one step of 0.2 is another map


def test_chain_collect_terms_action_rules():
    """good = status in {0, 2} and all three controls finite, else a zero action in all three components before the noise; sigma = 0 is u0
    itself beyond the bounds; sigma > 0 clips per component."""
    from mpc4rl_amd import chain_collect_terms, chain_env_step_terms
    ocp, off, x, u, p, wn = _random_points(3, 6, 5)
    x_ss = torch.tensor(ocp.consts)
    u = u * 3.0
    status = torch.tensor([0, 2, 1, 4, 0, 0], dtype=torch.int32)
    u[4, 1] = float("nan")
    lo, hi = [-1.0, -0.5, -1.0], [1.0, 1.0, 0.25]
    act, new, cost = chain_collect_terms(ocp, p, x_ss, x, u, status, torch.zeros(6, 3), wn, 0.05, lo, hi, 0.0)
    assert torch.equal(act[:2], u[:2]) and torch.equal(act[5], u[5]) and float(act[2:5].abs().max()) == 0.0 and float(act.abs().max()) > 1.0
    n2, c2 = chain_env_step_terms(ocp, p, x_ss, x, act, wn, 0.05)
    assert torch.equal(new, n2) and torch.equal(cost, c2)
    eps = torch.tensor([[0.5, -40.0, 40.0]] * 6)
    act, _, _ = chain_collect_terms(ocp, p, x_ss, x, u, status, eps, wn, 0.05, lo, hi, 0.1)
    n = (torch.tensor(0.1) * eps).double()
    assert torch.equal(act[2:5], torch.tensor([[0.05, -0.5, 0.25]], **F64).expand(3, 3).clone().copy_(n[2:5].clamp(torch.tensor(lo, **F64), torch.tensor(hi, **F64))))
    assert torch.equal(act[0], (u[0] + n[0]).clamp(torch.tensor(lo, **F64), torch.tensor(hi, **F64)))
    assert bool((act[:, 1] == -0.5).all()) and bool((act[:, 2] == 0.25).all())


def test_batched_chain_env_on_the_cpu():
    """reset touches the velocity entries only, step equals the statement bitwise (drawing its noise from env.gen), per-environment rows
    of p are honoured, and an in-place edit of env.p reaches the next step."""
    from mpc4rl_amd import BatchedChainMassEnv, chain_env_step_terms, chain_mass_ocp
    from mpc4rl_amd.problems import chain_param_layout
    E, n_mass = 5, 4
    ocp = chain_mass_ocp(n_mass, N=8)
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    env = BatchedChainMassEnv(E, ocp, w_std=0.05, vel_std=1e-2, seed=3)
    assert env.state.shape == (E, nx) and env.p.shape == (n_p,) and torch.equal(env.x_ss, torch.tensor(ocp.consts))
    obs = env.reset()
    x0 = torch.tensor(ocp.x0)
    assert torch.equal(obs, env.state) and obs.data_ptr() != env.state.data_ptr()
    assert torch.equal(obs[:, : nx - 3 * M], x0[: nx - 3 * M].repeat(E, 1))                      # positions: x0 exactly
    vel = obs[:, nx - 3 * M:]
    want = 1e-2 * torch.randn(E, 3 * M, generator=torch.Generator().manual_seed(3), **F64)
    assert torch.equal(vel, want) and float(vel.abs().min()) > 0.0
    # step: the statement on the generator's next draw
    g = torch.Generator().manual_seed(3)
    torch.randn(E, 3 * M, generator=g, **F64)
    wn = torch.randn(E, 3 * M, generator=g, **F64)
    a = torch.tensor([[0.5, -0.25, 1.0], [0.0, 0.0, 0.0], [-1.0, 1.0, 0.5], [2.0, -2.0, 0.1], [0.3, 0.3, 0.3]], **F64)
    s0 = env.state.clone()
    new, cost = chain_env_step_terms(ocp, env.p, env.x_ss, s0, a, wn, 0.05)
    obs, c, term, trunc = env.step(a)
    assert torch.equal(obs, new) and torch.equal(env.state, new) and torch.equal(c, cost)
    assert term.dtype == torch.bool and not bool(term.any()) and not bool(trunc.any())
    # the cost is l(s, a) of the state BEFORE the step
    e = s0 - env.x_ss
    Q = torch.tensor(ocp.p0[off["Q"][0]: off["Q"][1]]).reshape(nx, nx).T
    R = torch.tensor(ocp.p0[off["R"][0]: off["R"][1]]).reshape(3, 3).T
    want_c = 0.5 * (torch.einsum("ei,ij,ej->e", e, Q, e) + torch.einsum("ei,ij,ej->e", a, R, a))
    assert float(((c - want_c).abs() / want_c).max()) <= 1e-14
    # reset_where: the masked environments only
    mask = torch.tensor([True, False, True, False, False])
    before = env.state.clone()
    obs = env.reset_where(mask)
    assert torch.equal(obs[~mask], before[~mask]) and torch.equal(obs[mask][:, : nx - 3 * M], x0[: nx - 3 * M].repeat(2, 1))
    # per-environment parameters, float32 observations, no noise: nothing is drawn
    rows = torch.tensor(ocp.p0).repeat(E, 1)
    rows[:, off["m"][0]: off["m"][1]] *= torch.linspace(0.8, 1.2, E, **F64)[:, None]
    env = BatchedChainMassEnv(E, ocp, p=rows, seed=4, dtype=torch.float32)
    env.reset()
    s0, state_g = env.state.clone(), env.gen.get_state()
    obs, c, _, _ = env.step(a)
    assert torch.equal(env.gen.get_state(), state_g) and obs.dtype == torch.float32 and torch.equal(obs, env.state.float())
    for i in range(E):
        one, c1 = chain_env_step_terms(ocp, rows[i], env.x_ss, s0[i: i + 1], a[i: i + 1], None, 0.0)
        assert torch.equal(env.state[i: i + 1], one) and torch.equal(c[i: i + 1], c1)
    assert float((env.state[0] - chain_env_step_terms(ocp, rows[2], env.x_ss, s0[:1], a[:1], None, 0.0)[0]).abs().max()) > 1e-6
    env.p[:, off["m"][0]: off["m"][1]] = 0.033                                       # in place: honoured on the next step
    s1 = env.state.clone()
    env.step(a)
    assert torch.equal(env.state, chain_env_step_terms(ocp, torch.tensor(ocp.p0), env.x_ss, s1, a, None, 0.0)[0])
    with pytest.raises(ValueError):
        BatchedChainMassEnv(E, ocp, p=torch.zeros(3, n_p))
    with pytest.raises(ValueError):
        BatchedChainMassEnv(E, ocp, dtype=torch.float16)


def test_constructor_argument_checks():
    from mpc4rl_amd import (BatchedChainMassEnv, BatchedLinearSystemEnv, ChainQLearning, chain_mass_ocp, linear_system_ocp)
    ocp, lin = chain_mass_ocp(3, N=8), linear_system_ocp()
    env = BatchedChainMassEnv(4, ocp)
    with pytest.raises(ValueError, match="chain-of-masses OCP"):
        ChainQLearning(lin, env, 5)
    with pytest.raises(ValueError, match="chain-of-masses OCP"):
        BatchedChainMassEnv(4, lin)
    with pytest.raises(TypeError):
        ChainQLearning(ocp, BatchedLinearSystemEnv(4, device="cpu"), 5)
    with pytest.raises(ValueError, match="another chain"):
        ChainQLearning(ocp, BatchedChainMassEnv(4, chain_mass_ocp(4, N=8)), 5)
    with pytest.raises(ValueError, match="unknown block"):
        ChainQLearning(ocp, env, 5, learn=("m", "K"))
    for kw in (dict(episode_length=1), dict(episode_length=5, lr=float("nan")), dict(episode_length=5, gamma=0.0), dict(episode_length=5, noise_scale=-0.1)):
        with pytest.raises(ValueError):
            ChainQLearning(ocp, env, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # valid arguments, CPU environment: refused, never emulated
        ChainQLearning(ocp, env, 5, learn=("m", "D", "L", "C", "Q", "R", "w"))


def test_one_control_learners_keep_one_control():
    """DeviceQLearning's number of controls is a class attribute: 1 for the cartpole and the linear system, whose tables keep no control
    axis (tests/test_gpu_chain_loops.py checks the shapes on the device), 3 for the chain, whose state width is set per instance."""
    from mpc4rl_amd import CartpoleQLearning, ChainQLearning, LinearQLearning
    from mpc4rl_amd.qlearning import DeviceQLearning
    assert CartpoleQLearning.NU == LinearQLearning.NU == DeviceQLearning.NU == 1 and ChainQLearning.NU == 3
    assert (CartpoleQLearning.NX, LinearQLearning.NX, ChainQLearning.NX) == (4, 2, 0)
    assert "_initial_obs" not in vars(CartpoleQLearning) and "_initial_obs" not in vars(LinearQLearning)      # they start from zeros, as before
