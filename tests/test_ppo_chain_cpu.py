"""CPU checks of PPO on the chain of masses (csrc/ppo_chain_kernel.hpp, the nu-control surrogate of csrc/ppo_kernel.hpp, mpc4rl_amd/ppo.py):
the C ABI's new symbols and their argument checks, the torch statement of the nu-control surrogate against the one-control statement
(nu = 1, bit for bit) and against autograd (nu = 3), the statement of the roll-out step against the CPU path of BatchedChainMassEnv.step,
and the constructor's argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcrl_ppo_chain_collect", "mpcrl_ppo_surrogate_workspace_bytes_nu", "mpcrl_ppo_surrogate_grad_nu", "mpcrl_ppo_log_std_apply_nu"]


def test_new_symbols_in_header_binding_and_library():
    """The symbols are declared, bound and exported; header, binding and library agree on the version (the symbols are additions: the
    header's rule bumps the version only when an existing export changes, and existing tests pin it).  The argument checks that need no
    device: every NULL pointer, t outside [0, T), nu outside 1..3, episode_length = 0, n_mass outside 3..7 are MPCRL_E_ARG; E = 0 and
    M = 0 return 0 without a launch."""
    import __graft_entry__ as g
    from mpc4rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpcrl.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.EXPORTS, name
    if not os.path.exists(g.LIB):
        g.build()
    lib = ctypes.CDLL(g.LIB)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    lib.mpcrl_version.restype = ctypes.c_int
    assert lib.mpcrl_version() == _lib.ABI_VERSION == int(re.search(r"#define MPCRL_ABI_VERSION (\d+)", hdr).group(1))
    vp, ci, cd, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
    lib.mpcrl_ppo_chain_collect.argtypes = [ci, cd, ci, vp, i64, vp, cd, ci, ci, ci] + [vp] * 10 + [cd, i64, vp, cd, vp] + [vp] * 12
    lib.mpcrl_ppo_surrogate_workspace_bytes_nu.argtypes = [ci, ci, ci]
    lib.mpcrl_ppo_surrogate_workspace_bytes_nu.restype = i64
    lib.mpcrl_ppo_surrogate_grad_nu.argtypes = [vp, ci, i64] + [vp] * 7 + [ci, ci, vp, vp, vp, cd, cd, cd, ci, vp, vp, vp]
    lib.mpcrl_ppo_log_std_apply_nu.argtypes = [vp, ci, ci, vp, vp]
    buf = (ctypes.c_double * 8)()          # never read: every call below returns before its launch
    p = ctypes.cast(buf, vp)
    lo, hi = (ctypes.c_double * 3)(-1.0, -0.5, -1.0), (ctypes.c_double * 3)(1.0, 1.0, 0.25)
    lo_p, hi_p = ctypes.cast(lo, vp), ctypes.cast(hi, vp)
    n_p3 = 10 * 2 + 9 * 9 + 9 + 3          # ChainDev<3>::NP

    def coll(n_mass=3, E=0, T=4, t=0, L=3, null=None, lo=lo_p, hi=hi_p, stride=0):
        # pointers in order: p, x_ss | state, steps, u0, status, eps, wn, value, log_std, lo, hi | x_reset, rn | 9 tables, obs, ended
        ptrs = [p] * 25
        ptrs[10], ptrs[11] = lo, hi
        if null is not None:
            ptrs[null] = None
        return lib.mpcrl_ppo_chain_collect(n_mass, 0.2, 2, ptrs[0], stride, ptrs[1], 0.05, E, T, t, *ptrs[2:12], -1.0, L, ptrs[12], 1e-2, ptrs[13],
                                           *ptrs[14:], None)

    assert coll() == 0 and coll(stride=n_p3) == 0                      # E = 0: nothing to do
    assert coll(E=-1) == -1 and coll(T=0) == -1 and coll(t=4) == -1 and coll(t=-1) == -1 and coll(L=0) == -1
    assert coll(n_mass=2) == -1 and coll(n_mass=8) == -1 and coll(stride=n_p3 + 1) == -1
    assert all(coll(null=k) == -1 for k in range(25))                  # (wn and rn: NULL with w_std, vel_std != 0)
    assert coll(lo=hi_p, hi=lo_p) == -1 and coll(lo=lo_p, hi=lo_p) == -1

    def sur(M=0, n_rows=8, n_p=5, nu=3, null=None, lo=lo_p, hi=hi_p, clip=0.2):
        # pointers in order: idx, ACT, LOGP, ADV, OK, u0_new, status_new, dpi_dp | log_std, lo, hi | workspace, msg
        ptrs = [p] * 13
        ptrs[9], ptrs[10] = lo, hi
        if null is not None:
            ptrs[null] = None
        return lib.mpcrl_ppo_surrogate_grad_nu(ptrs[0], M, n_rows, *ptrs[1:8], n_p, nu, *ptrs[8:11], clip, 0.0, 1e-3, 1, ptrs[11], ptrs[12], None)

    assert sur() == 0 and sur(nu=1) == 0 and sur(nu=2) == 0            # M = 0: nothing to do
    assert sur(nu=0) == -1 and sur(nu=4) == -1 and sur(M=-1) == -1 and sur(n_rows=0) == -1 and sur(n_p=0) == -1 and sur(clip=0.0) == -1
    assert all(sur(null=k) == -1 for k in range(13))
    assert sur(lo=hi_p, hi=lo_p) == -1
    ws = lib.mpcrl_ppo_surrogate_workspace_bytes_nu
    assert ws(300, 499, 3) == 16 + 3 * (499 + 6 + 2) * 8 and ws(128, 5, 1) == 16 + (5 + 6) * 8 and ws(0, 5, 2) == 16
    assert ws(4, 5, 0) == -1 and ws(4, 5, 4) == -1 and ws(-1, 5, 1) == -1 and ws(4, 0, 1) == -1
    apply = lib.mpcrl_ppo_log_std_apply_nu
    assert apply(None, 5, 3, p, None) == -1 and apply(p, 5, 3, None, None) == -1
    assert apply(p, 5, 0, p, None) == -1 and apply(p, 5, 4, p, None) == -1 and apply(p, 0, 3, p, None) == -1


# ---------------------------------------------------------------------- the nu-control surrogate's statement
@pytest.mark.parametrize("normalize", [True, False])
def test_surrogate_terms_nu_at_one_control_are_the_one_control_terms(normalize):
    from mpc4rl_amd import ppo_surrogate_terms, ppo_surrogate_terms_nu
    from test_ppo_cpu import _surrogate_case
    for seed in (11, 12):
        c = _surrogate_case(seed)
        kw = dict(clip_range=0.2, ent_coef=0.01, lr=3e-3, normalize_adv=normalize)
        one, nu = ppo_surrogate_terms(**c, **kw), ppo_surrogate_terms_nu(**c, **kw)
        assert nu.shape == one.shape and torch.equal(one, nu) and float(one.abs().sum()) > 0.0


LO3, HI3, LS3 = [-1.0, -0.5, -1.0], [1.0, 1.0, 0.25], [-0.5, -0.2, -0.8]


def _case3(seed, n_p=7):
    """A three-control minibatch: a table of 160 rows written by the roll-out's statement, 120 rows of it re-solved with means that moved
    by up to 0.5 sigma per control (so that the summed log ratio leaves the band on both sides), plus rows that must never reach a sum."""
    from mpc4rl_amd.ppo import _collect_terms_nu
    rng = np.random.default_rng(seed)
    n_rows, M = 160, 120
    lo, hi, ls = np.array(LO3), np.array(HI3), np.array(LS3)
    u0 = lo + rng.uniform(0.1, 0.9, (n_rows, 3)) * (hi - lo)
    status = np.zeros(n_rows, np.int32)
    status[:6] = [2, 4, 1, 0, 0, 0]
    u0[3, 1] = np.nan                                          # one component only
    eps = rng.normal(size=(n_rows, 3)).astype(np.float32)
    _, act, logp, ok = _collect_terms_nu(torch.as_tensor(u0), torch.as_tensor(status), torch.as_tensor(eps), LS3, LO3, HI3)
    adv = torch.as_tensor(rng.normal(0.3, 1.0, n_rows))
    idx = torch.as_tensor(np.concatenate([np.arange(8), 8 + rng.permutation(n_rows - 8)[: M - 8]]))
    u0_new = np.nan_to_num(u0)[idx.numpy()] + rng.uniform(-1, 1, (M, 3)) * 0.5 * np.exp(ls) * 0.5 * (hi - lo)
    status_new = np.zeros(M, np.int32)
    status_new[8:12] = [4, 1, 2, 0]
    u0_new[11, 2] = np.nan
    dpi = rng.normal(size=(M, 3, n_p))
    dpi[8], dpi[11], dpi[1] = np.nan, np.nan, np.inf          # rows left out: their sensitivities may be anything
    dpi[20, 1, 2] = np.nan                                     # a NaN entry of a row that is left in: read as nan_to_num does
    return dict(idx=idx, act=act, logp=logp, adv=adv, ok=ok.to(torch.uint8), u0_new=torch.as_tensor(u0_new), status_new=torch.as_tensor(status_new),
                dpi_dp=torch.as_tensor(dpi), log_std=LS3, lo=LO3, hi=HI3)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_surrogate_terms_nu_match_autograd_at_three_controls(normalize, ent_coef):
    """The n_p gradient entries = -lr x autograd's d(sum of the clipped loss)/d u0_new contracted with dpi_dp; the three log_std entries =
    -lr x autograd's gradient with respect to log_std (entropy bonus included); float64, 1e-12 relative."""
    from mpc4rl_amd import ppo_surrogate_terms_nu
    c = _case3(21)
    clip, lr, n_p = 0.2, 3e-3, c["dpi_dp"].shape[-1]
    msg = ppo_surrogate_terms_nu(**c, clip_range=clip, ent_coef=ent_coef, lr=lr, normalize_adv=normalize)
    assert msg.shape == (n_p + 8 + 2,) and torch.isfinite(msg).all()
    j, st, un = c["idx"], c["status_new"], c["u0_new"]
    valid = c["ok"][j].bool() & ((st == 0) | (st == 2)) & torch.isfinite(un).all(1)
    expect_out = {1, 2, 3, 8, 9, 11}                           # OK = 0 (status 4, 1, a NaN u0 component), status_new 4 / 1, a NaN u0_new component
    assert set(torch.nonzero(~valid).reshape(-1).tolist()) == expect_out
    assert int(msg[n_p + 1]) == int(valid.sum()) == j.numel() - len(expect_out)
    a, lp_old, ad = c["act"][j][valid], c["logp"][j][valid], c["adv"][j][valid]
    A = (ad - ad.mean()) / (ad.std() + 1e-8) if normalize else ad
    u = un[valid].clone().requires_grad_(True)
    ls = torch.tensor(LS3, dtype=torch.float64, requires_grad=True)
    lo, hi = torch.tensor(LO3, dtype=torch.float64), torch.tensor(HI3, dtype=torch.float64)
    mu = 2.0 * ((u - lo) / (hi - lo)) - 1.0
    lp = (-((a - mu) ** 2) / (2.0 * torch.exp(ls) ** 2) - ls - 0.5 * math.log(2.0 * math.pi)).sum(1)
    r = torch.exp(lp - lp_old)
    loss = -torch.minimum(r * A, torch.clamp(r, 1.0 - clip, 1.0 + clip) * A)
    entropy = ls.sum() + 3 * (0.5 + 0.5 * math.log(2.0 * math.pi))
    (loss.sum() - ent_coef * int(valid.sum()) * entropy).backward()
    rd, below, above = r.detach(), r.detach() < 1.0 - clip, r.detach() > 1.0 + clip
    for sign in (A > 0, A < 0):                                # the inputs hold all six combinations of sign and region
        for region in (below, above, ~below & ~above):
            assert int((sign & region).sum()) >= 2
    G = torch.nan_to_num(c["dpi_dp"][valid])                   # [n, 3, n_p]
    assert bool(torch.isnan(c["dpi_dp"][valid]).any())         # the NaN entry of a row that is left in
    ref_grad = -lr * torch.einsum("bc,bcp->p", u.grad, G)
    np.testing.assert_allclose(msg[:n_p].numpy(), ref_grad.numpy(), rtol=1e-12, atol=0.0)
    got_ls = torch.stack([msg[n_p], msg[n_p + 8], msg[n_p + 9]])
    np.testing.assert_allclose(got_ls.numpy(), (-lr * ls.grad).numpy(), rtol=1e-12, atol=0.0)
    assert math.isclose(float(msg[n_p + 2]), float(loss.detach().sum()), rel_tol=1e-12)
    assert math.isclose(float(msg[n_p + 3]), float(((rd - 1.0) - torch.log(rd)).sum()), rel_tol=1e-12)
    assert int(msg[n_p + 4]) == int((below | above).sum())
    assert math.isclose(float(msg[n_p + 5]), float(rd.sum()), rel_tol=1e-12)
    assert math.isclose(float(msg[n_p + 6]), float(ad.sum()), rel_tol=1e-12)
    assert math.isclose(float(msg[n_p + 7]), float(ad.var() * (ad.numel() - 1)), rel_tol=1e-12)


def test_unchanged_three_control_policy_has_ratio_one_exactly():
    """u0_new the roll-out's u0 and LOGP from the roll-out's statement: sum r == count, approximate KL == 0 and no clipped row, exactly."""
    from mpc4rl_amd import ppo_surrogate_terms_nu
    from mpc4rl_amd.ppo import _collect_terms_nu
    rng = np.random.default_rng(5)
    E, n_p = 50, 4
    u0 = torch.as_tensor(rng.uniform(-1.5, 1.5, (E, 3)))
    status = torch.as_tensor((rng.uniform(size=E) < 0.2).astype(np.int32) * 2)
    eps = torch.as_tensor(rng.normal(size=(E, 3)).astype(np.float32))
    _, act, logp, ok = _collect_terms_nu(u0, status, eps, LS3, LO3, HI3)
    assert bool(ok.all())
    msg = ppo_surrogate_terms_nu(torch.arange(E), act, logp, torch.as_tensor(rng.normal(size=E)), ok.to(torch.uint8), u0, status,
                                 torch.as_tensor(rng.normal(size=(E, 3, n_p))), LS3, LO3, HI3, clip_range=0.2, ent_coef=0.0, lr=1e-3, normalize_adv=True)
    assert float(msg[n_p + 1]) == E == float(msg[n_p + 5]) and float(msg[n_p + 3]) == 0.0 and float(msg[n_p + 4]) == 0.0


# ---------------------------------------------------------------------- the roll-out step's statement
def test_chain_collect_terms_equal_the_environments_cpu_step():
    """ppo_chain_collect_terms over T = 4 steps with episode_length = 3 against BatchedChainMassEnv(device="cpu").step fed the same draws
    and the applied (physical) controls: torch.equal on the new state and the cost; DONE on the rows the count says; NEXT the pre-reset
    state; the reset state x0 + vel_std * rn on the velocities only."""
    from mpc4rl_amd import BatchedChainMassEnv, chain_mass_ocp, ppo_chain_collect_terms
    n_mass, E, T, L, w_std, vel_std, rs = 3, 5, 4, 3, 0.05, 1e-2, -0.5
    ocp = chain_mass_ocp(n_mass, N=8)
    M, nx = n_mass - 2, ocp.nx
    env = BatchedChainMassEnv(E, ocp, device="cpu", w_std=w_std, vel_std=vel_std, seed=4)
    env.reset()
    x0 = torch.tensor(ocp.x0)
    g = torch.Generator().manual_seed(7)
    state, steps = env.state.clone(), torch.tensor([0, 1, 2, 0, 2])
    counts = steps.clone()
    ends = 0
    for t in range(T):
        u0 = torch.rand(E, 3, generator=g, dtype=torch.float64) * 3.0 - 1.5
        status = torch.tensor([0, 2, 0, 4, 0], dtype=torch.int32)
        eps = (torch.randn(E, 3, generator=g) * 3.0).float()
        rn = torch.randn(E, 3 * M, generator=g, dtype=torch.float64)
        twin = torch.Generator()
        twin.set_state(env.gen.get_state())
        wn = torch.randn(E, 3 * M, generator=twin, dtype=torch.float64)                      # the environment's next draw
        o = ppo_chain_collect_terms(ocp, env.p, env.x_ss, state, steps, u0, status, eps, wn, w_std, LS3, LO3, HI3, rs, L, x0, vel_std, rn)
        assert o["ok"].tolist() == [True, True, True, False, True] and float(o["mu"][3].abs().max()) == 0.0
        lo, hi = torch.tensor(LO3, dtype=torch.float64), torch.tensor(HI3, dtype=torch.float64)
        assert torch.equal(o["applied"], lo + (0.5 * (o["act"].clamp(-1.0, 1.0) + 1.0)) * (hi - lo))
        assert bool((o["applied"] >= lo).all()) and bool((o["applied"] <= hi).all()) and bool((o["act"].abs() > 1.0).any())
        env.state.copy_(state)
        obs, cost, _, _ = env.step(o["applied"])
        assert torch.equal(o["next"], obs) and torch.equal(o["rew"], rs * cost)
        counts = counts + 1
        done = counts >= L
        assert torch.equal(o["done"], done)
        fresh = x0.repeat(E, 1)
        fresh[:, nx - 3 * M:] += vel_std * rn
        assert torch.equal(o["state"][done], fresh[done]) and torch.equal(o["state"][~done], obs[~done])
        assert torch.equal(o["state"][done][:, : nx - 3 * M], x0[: nx - 3 * M].repeat(int(done.sum()), 1))       # positions: x0 itself
        if bool(done.any()):
            assert not torch.equal(o["next"][done], o["state"][done]) and float((o["state"][done][:, nx - 3 * M:] - x0[nx - 3 * M:]).abs().min()) > 0.0
        counts = torch.where(done, torch.zeros_like(counts), counts)
        assert torch.equal(o["steps"], counts)
        state, steps = o["state"], o["steps"]
        ends += int(done.sum())
    assert ends == 1 + 1 + 2 + 1 + 2          # counts 0, 1, 2, 0, 2 at the start, four steps of episodes of three
    # without draws: rn = None / vel_std = 0 restarts at x0 itself, wn = None / w_std = 0 adds nothing
    o = ppo_chain_collect_terms(ocp, env.p, env.x_ss, state, torch.full((E,), L - 1), u0, status, eps, None, 0.0, LS3, LO3, HI3, rs, L, x0, 0.0, None)
    assert bool(o["done"].all()) and torch.equal(o["state"], x0.repeat(E, 1)) and int(o["steps"].sum()) == 0


# ---------------------------------------------------------------------- the policy's and the learner's argument checks
def test_constructor_argument_checks():
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedChainMassEnv, BatchedPPO, cartpole_ocp, chain_mass_ocp
    chain, cart = chain_mass_ocp(3, N=8), cartpole_ocp()
    env, cenv = BatchedChainMassEnv(8, chain, device="cpu"), BatchedCartPoleSwingUpEnv(8, device="cpu")
    kw = dict(n_steps=4, batch_size=16, n_epochs=1)
    with pytest.raises(TypeError):
        BatchedPPO(chain, cenv, episode_length=3, **kw)
    with pytest.raises(ValueError, match="episode_length"):
        BatchedPPO(chain, env, **kw)
    with pytest.raises(ValueError, match="episode_length"):
        BatchedPPO(chain, env, episode_length=0, **kw)
    with pytest.raises(ValueError, match="unknown block"):
        BatchedPPO(chain, env, episode_length=3, learn=("m", "X"), **kw)
    with pytest.raises(ValueError, match="learn"):
        BatchedPPO(cart, cenv, learn=("m",))
    with pytest.raises(ValueError, match="another chain"):
        BatchedPPO(chain, BatchedChainMassEnv(8, chain_mass_ocp(4, N=8), device="cpu"), episode_length=3, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # valid arguments, CPU environment: refused, never emulated
        BatchedPPO(chain, env, episode_length=3, learn=("C",), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BatchedPPO(chain, env, episode_length=3, **kw)
