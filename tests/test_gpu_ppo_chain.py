"""GPU tests of PPO on the chain of masses (csrc/ppo_chain_kernel.hpp, the nu-control surrogate of csrc/ppo_kernel.hpp, mpc4rl_amd/ppo.py):
the roll-out kernel against its torch statement and against mpcrl_env_chain_step on poisoned tables, the surrogate kernel against its
statement for one to three controls, the log_std step, the surrogate's parameter gradient through the chain solver against central finite
differences, and the learner end to end.

Tolerances are those of the tests of the same expressions: the new state, NEXT and REW to TOL = 1e-12 of tests/test_gpu_chain_loops.py
(every entry scaled by max(1, |reference|), for the reason that file's docstring gives: the kernel is compiled with floating-point
contraction, the statement rounds once per operation); ACT, LOGP and the surrogate's message to the 1e-12 relative of
tests/test_gpu_ppo.py.  What is copied or selected is compared bit for bit.  Every comparison prints its observed maximum."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
TOL = 1e-12
POISON = -7.0
LO3, HI3, LS3 = [-1.0, -0.5, -1.0], [1.0, 1.0, 0.25], [0.4, -0.3, 0.1]      # asymmetric bounds per control (test_gpu_chain_loops._collect_case)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _err(got, want):
    """the largest difference, every entry scaled by max(1, |want|)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) if want.numel() else 0.0


def _rel(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / np.where(want != 0.0, np.abs(want), 1.0))) if got.size else 0.0


def _same_bits(a, b):
    """equal as stored, NaN and inf included"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        as_int = torch.int64 if a.dtype == torch.float64 else torch.int32
        a, b = a.view(as_int), b.view(as_int)
    return torch.equal(a, b)


def _d3(v):
    return (C.c_double * len(v))(*v)


_OCPS = {}


def _ocp(n_mass, N=8, **kw):
    from mpc4rl_amd import chain_mass_ocp
    key = (n_mass, N, tuple(sorted(kw.items())))
    if key not in _OCPS:
        _OCPS[key] = chain_mass_ocp(n_mass, N=N, **kw)
    return _OCPS[key]


def _points(n_mass, E, seed):
    """States around x0, controls beyond the bounds, per-row dynamics parameters x U(0.8, 1.2) (all on the CPU)."""
    from mpc4rl_amd.problems import chain_param_layout
    ocp = _ocp(n_mass)
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(ocp.x0) + 0.05 * torch.randn(E, nx, generator=g, dtype=torch.float64)
    u = torch.rand(E, 3, generator=g, dtype=torch.float64) * 3.0 - 1.5
    rows = torch.tensor(ocp.p0).repeat(E, 1)
    nd = off["C"][1]
    rows[:, :nd] *= 0.8 + 0.4 * torch.rand(E, nd, generator=g, dtype=torch.float64)
    return ocp, g, x, u, rows


class _Tables:
    def __init__(self, T, E, nx):
        self.OBS, self.NEXT = torch.full((T, E, nx), POISON, **F64), torch.full((T, E, nx), POISON, **F64)
        self.ACT = torch.full((T, E, 3), POISON, **F64)
        self.LOGP, self.VAL, self.REW = (torch.full((T, E), POISON, **F64) for _ in range(3))
        self.TERM, self.DONE, self.OK = (torch.full((T, E), 9, dtype=torch.uint8, device=DEV) for _ in range(3))

    def all(self):
        return (self.OBS, self.ACT, self.LOGP, self.VAL, self.REW, self.NEXT, self.TERM, self.DONE, self.OK)


def _chain_collect(lib, ocp, n_mass, p, per_row, x_ss, w_std, E, T, t, state, steps, u0, status, eps, wn, value, log_std, lo, hi, rs, L, x_reset, vel_std,
                   rn, tab, obs, ended):
    return lib.mpcrl_ppo_chain_collect(n_mass, ocp.dT, ocp.rk_steps, _p(p), ocp.n_p if per_row else 0, _p(x_ss), w_std, E, T, t, _p(state), _p(steps),
                                       _p(u0), _p(status), _p(eps), _p(wn), _p(value), _p(log_std), _d3(lo), _d3(hi), rs, L, _p(x_reset), vel_std, _p(rn),
                                       *[_p(x) for x in tab.all()], _p(obs), _p(ended), _stream())


# ---------------------------------------------------------------------- 1. the collect kernel against its statement
@pytest.mark.parametrize("E", [1, 63, 65, 130])
@pytest.mark.parametrize("n_mass", [3, 5, 7])
def test_chain_collect_equals_its_statement_on_poisoned_tables(n_mass, E):
    """mpcrl_ppo_chain_collect, T = 3, rows t = 0 and 2, a shared and a per-row p, w_std 0 (wn NULL) and 0.05, vel_std 0 (rn NULL) and
    1e-2, on both sides of a 64-lane block: statuses 0, 1, 2, 4 and a NaN or an inf in ONE component of u0 (mu = 0 in all three), draws
    x 8 so that the samples clip at both ends of per-control bounds, step counts preset so that some environments end at this step and
    others do not (E = 1: the one environment ends at t = 2).  State, NEXT, REW to TOL; ACT, LOGP to 1e-12 relative; OBS, VAL, TERM, DONE,
    OK, obs, ended, steps and the reset state bit for bit; the other rows and all inputs untouched; mpcrl_env_chain_step on the applied
    action gives the bits of NEXT and REW."""
    from mpc4rl_amd import _lib, ppo_chain_collect_terms
    lib = _lib.load()
    T, L, rs = 3, 3, -0.5
    ocp, g, x, u0, rows = _points(n_mass, E, 3000 + 10 * n_mass + E)
    M, nx = n_mass - 2, ocp.nx
    i = torch.arange(E)
    status = torch.where(i % 5 == 2, 4, torch.where(i % 5 == 1, 2, torch.where(i % 5 == 4, 1, 0))).to(torch.int32)
    if E > 1:
        u0[i % 7 == 3, 1], u0[i % 11 == 5, 2] = float("nan"), float("inf")               # one component only
    eps = (torch.randn(E, 3, generator=g) * 8.0).float()                                  # sigma eps clips at both ends
    wn, rn = (torch.randn(E, 3 * M, generator=g, dtype=torch.float64) for _ in range(2))
    value = torch.randn(E, generator=g, dtype=torch.float64)
    x_ss, x_reset = torch.tensor(ocp.consts), torch.tensor(ocp.x0)
    lo_t, hi_t = torch.tensor(LO3, **F64), torch.tensor(HI3, **F64)
    d = lambda v: v.to(DEV).contiguous()
    worst, worst_a = 0.0, 0.0
    for t in (0, 2):
        steps0 = (i + t) % 3
        for per_row in (False, True):
            p = rows if per_row else rows[0].clone()
            for w_std in (0.0, 0.05):
                for vel_std in (0.0, 1e-2):
                    o = ppo_chain_collect_terms(ocp, p, x_ss, x, steps0, u0, status, eps, wn if w_std else None, w_std, LS3, LO3, HI3, rs, L, x_reset,
                                                vel_std, rn if vel_std else None)
                    state, steps, tab = d(x), d(steps0), _Tables(T, E, nx)
                    obs, ended = torch.full((E, nx), POISON, **F64), torch.full((E,), 9, dtype=torch.int32, device=DEV)
                    pd, xd, ud, sd, ed, wd, rd, vd, xr = d(p), d(x_ss), d(u0), d(status), d(eps), d(wn), d(rn), d(value), d(x_reset)
                    ls = torch.tensor(LS3, **F64)
                    rc = _chain_collect(lib, ocp, n_mass, pd, per_row, xd, w_std, E, T, t, state, steps, ud, sd, ed, wd if w_std else None, vd, ls, LO3, HI3,
                                        rs, L, xr, vel_std, rd if vel_std else None, tab, obs, ended)
                    assert rc == 0
                    torch.cuda.synchronize()
                    done, ok = o["done"], o["ok"]
                    e_act, e_lp = _rel(tab.ACT[t].cpu().numpy(), o["act"].numpy()), _rel(tab.LOGP[t].cpu().numpy(), o["logp"].numpy())
                    e_x, e_n, e_r = _err(state, o["state"]), _err(tab.NEXT[t], o["next"]), _err(tab.REW[t], o["rew"])
                    worst, worst_a = max(worst, e_x, e_n, e_r), max(worst_a, e_act, e_lp)
                    assert e_act <= 1e-12 and e_lp <= 1e-12, (e_act, e_lp)
                    assert e_x <= TOL and e_n <= TOL and e_r <= TOL, (e_x, e_n, e_r)
                    # copies, selections and counts: the bits
                    assert torch.equal(tab.OBS[t].cpu(), x) and torch.equal(tab.VAL[t].cpu(), value) and int(tab.TERM[t].sum()) == 0
                    assert torch.equal(tab.DONE[t].cpu().bool(), done) and torch.equal(tab.OK[t].cpu().bool(), ok)
                    assert torch.equal(obs, state) and torch.equal(ended.cpu().bool(), done) and torch.equal(steps.cpu(), o["steps"])
                    assert torch.equal(state.cpu()[done], o["state"][done])                       # x0 (+ vel_std rn): no product that contraction could fuse
                    assert torch.equal(state[~done.to(DEV)], tab.NEXT[t][~done.to(DEV)])
                    # the other rows, and the inputs
                    for tb in tab.all():
                        for row in set(range(T)) - {t}:
                            assert bool((tb[row] == (9 if tb.dtype == torch.uint8 else POISON)).all())
                    for got, want in ((pd, p), (xd, x_ss), (ud, u0), (sd, status), (ed, eps), (wd, wn), (rd, rn), (vd, value), (xr, x_reset)):
                        assert _same_bits(got, want)
                    assert torch.equal(ls.cpu(), torch.tensor(LS3, dtype=torch.float64))
                    # one step function: mpcrl_env_chain_step on the applied action
                    applied = (lo_t + (0.5 * (tab.ACT[t].clamp(-1.0, 1.0) + 1.0)) * (hi_t - lo_t)).contiguous()
                    st2, c2 = d(x), torch.full((E,), POISON, **F64)
                    assert lib.mpcrl_env_chain_step(n_mass, ocp.dT, ocp.rk_steps, _p(pd), ocp.n_p if per_row else 0, _p(xd), E, _p(st2), _p(applied),
                                                    _p(wd) if w_std else None, w_std, None, 0, _p(c2), _stream()) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(st2, tab.NEXT[t]) and torch.equal(rs * c2, tab.REW[t])
        # what the case holds
        if E > 1:
            act = o["act"]
            assert 0 < int(done.sum()) < E and 0 < int(ok.sum()) < E and float(o["mu"][~ok].abs().max()) == 0.0
            assert sorted(set(status[~ok].tolist())) == [0, 1, 2, 4]
            assert bool((act < -1.0).any(0).all()) and bool((act > 1.0).any(0).all())          # every control clips at both ends
        else:
            assert bool(done.all()) == (t == 2)
    print(f"n_mass {n_mass} E {E}: state / NEXT / REW largest {worst:.3e}, ACT / LOGP largest {worst_a:.3e}")


def test_chain_collect_argument_errors_on_device_pointers():
    from mpc4rl_amd import _lib
    lib = _lib.load()
    E, T, n_mass = 4, 3, 3
    ocp = _ocp(n_mass)
    nx = ocp.nx
    p, x_ss = torch.tensor(ocp.p0, **F64), torch.tensor(ocp.consts, **F64)
    state = torch.tensor(ocp.x0, **F64).repeat(E, 1)
    z, zi, z64 = torch.zeros(T, E, nx, **F64), torch.zeros(E, dtype=torch.int32, device=DEV), torch.zeros(E, dtype=torch.int64, device=DEV)
    zf = torch.zeros(E, 3, dtype=torch.float32, device=DEV)
    zb = torch.zeros(T, E, dtype=torch.uint8, device=DEV)
    host = (C.c_double * (E * nx))()

    def coll(n_mass=n_mass, E=E, t=0, L=3, state=_p(state), wn=z, w_std=0.05, rn=z, vel_std=1e-2, lo=LO3, hi=HI3, OBS=z):
        return lib.mpcrl_ppo_chain_collect(n_mass, 0.2, 2, _p(p), 0, _p(x_ss), w_std, E, T, t, state, _p(z64), _p(z), _p(zi), _p(zf), _p(wn), _p(z), _p(z),
                                           _d3(lo), _d3(hi), -1.0, L, _p(x_ss), vel_std, _p(rn), _p(OBS), _p(z), _p(z), _p(z), _p(z), _p(z), _p(zb), _p(zb),
                                           _p(zb), _p(z), _p(zi), _stream())

    assert coll(n_mass=2) == -1 and coll(n_mass=8) == -1 and coll(t=T) == -1 and coll(t=-1) == -1 and coll(L=0) == -1 and coll(E=-1) == -1
    assert coll(wn=None) == -1 and coll(rn=None) == -1 and coll(OBS=None) == -1 and coll(state=None) == -1 and coll(hi=LO3) == -1
    assert coll(state=C.cast(host, C.c_void_p)) == -1                                # not device memory
    assert coll(E=0) == 0 and coll(wn=None, w_std=0.0) == 0 and coll(rn=None, vel_std=0.0) == 0 and coll() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all())


# ---------------------------------------------------------------------- 2. the surrogate kernel against its statement
def _surrogate_inputs(M, n_p, nu, seed):
    """tests/test_gpu_ppo.py's minibatch for nu controls, over a table of 2 M + 5 rows: ratios on both sides of the clip band, advantages of
    both signs, rows left out for every reason (OK = 0, a rejected re-solve, a NaN component of u0_new, a non-finite table entry, an index
    outside the table) where M allows, NaN / inf sensitivities in rows left out and a NaN entry in a row that may be left in.  The
    sensitivities are built so that every gradient entry is a well-conditioned sum (see below)."""
    from mpc4rl_amd.ppo import _collect_terms_nu
    rng = np.random.default_rng(seed)
    n_rows = 2 * M + 5
    lo, hi, ls = np.array(LO3[:nu]), np.array(HI3[:nu]), np.array([-0.5, -0.2, -0.8][:nu])
    u0 = lo + rng.uniform(-0.1, 1.1, (n_rows, nu)) * (hi - lo)
    status = np.where(rng.uniform(size=n_rows) < 0.1, 4, np.where(rng.uniform(size=n_rows) < 0.1, 2, 0)).astype(np.int32)
    eps = rng.normal(size=(n_rows, nu)).astype(np.float32)
    _, act, logp, ok = _collect_terms_nu(torch.as_tensor(u0), torch.as_tensor(status), torch.as_tensor(eps), list(ls), list(lo), list(hi))
    adv = torch.as_tensor(rng.normal(0.3, 1.0, n_rows))
    idx = rng.permutation(n_rows)[:M].astype(np.int64)
    u0_new = u0[idx] + rng.uniform(-1, 1, (M, nu)) * (0.8 / math.sqrt(nu)) * np.exp(ls) * 0.5 * (hi - lo)
    status_new = np.where(rng.uniform(size=M) < 0.08, 4, np.where(rng.uniform(size=M) < 0.1, 2, 0)).astype(np.int32)
    # A row's sensitivities carry the sign of its weight, -sign(A) sign(a - mu) (up to the rows whose advantage changes sign under the
    # normalisation or whose mean moved past the sample), so that no gradient entry is a cancelling sum: sum |terms| <= about 2 |sum|.
    # A fixed-order fp64 sum of n <= 900 terms is then within n u 2 = 2e-13 of its own value, and the 1e-12 relative bound is one on the
    # kernel; on a column of pure noise (terms of random sign) it would be a bound on how close to zero the sum happens to fall.
    h = -np.sign(adv.numpy()[idx])[:, None] * np.sign(eps[idx])
    dpi = h[:, :, None] * rng.uniform(0.5, 1.5, (M, nu, n_p)) + 0.25 * rng.normal(size=(M, nu, n_p))
    dpi[status_new == 4] = np.nan
    if M > 8:
        u0_new[3, nu - 1], dpi[3] = np.nan, np.inf
        adv[idx[5]] = float("inf")
        idx[6], idx[7] = -1, n_rows
        dpi[8, nu - 1, n_p - 1] = np.nan                          # a NaN entry of a row that may be left in: read as nan_to_num does
    return dict(idx=torch.as_tensor(idx), act=act if nu > 1 else act.reshape(-1), logp=logp, adv=adv, ok=ok.to(torch.uint8), u0_new=torch.as_tensor(u0_new),
                status_new=torch.as_tensor(status_new), dpi_dp=torch.as_tensor(dpi), log_std=list(ls), lo=list(lo), hi=list(hi))


def _surrogate_call(lib, c, nu, ws, clip, ent, lr, norm, msg):
    M, n_p = c["idx"].numel(), c["dpi_dp"].shape[-1]
    return lib.mpcrl_ppo_surrogate_grad_nu(_p(c["idx"]), M, c["logp"].numel(), _p(c["act"]), _p(c["logp"]), _p(c["adv"]), _p(c["ok"]), _p(c["u0_new"]),
                                           _p(c["status_new"]), _p(c["dpi_dp"]), n_p, nu, _p(c["log_std"]), _d3(c["lo"]), _d3(c["hi"]), clip, ent, lr, norm,
                                           _p(ws), _p(msg), _stream())


@pytest.mark.parametrize("n_p", [113, 256, 499])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_surrogate_kernel_nu_matches_its_statement(nu, M, n_p):
    """msg of mpcrl_ppo_surrogate_grad_nu against ppo_surrogate_terms_nu at 1e-12 relative on every entry, with and without advantage
    normalisation; M around PPO_ROWS = 128 and over several workgroups; n_p below, at and above PPO_PMAX = 256 (499 + 6 + nu - 1 entries: a
    ragged last chunk of the final sum); the call repeated gives equal bits; the workspace is all zero afterwards; nu = 1 gives the bits
    of mpcrl_ppo_surrogate_grad."""
    from mpc4rl_amd import _lib, ppo_surrogate_terms_nu
    lib = _lib.load()
    clip, ent, lr = 0.2, 0.01, 3e-3
    c = _surrogate_inputs(M, n_p, nu, 1000 * nu + 100 * M + n_p)
    d = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}
    d["log_std"] = torch.tensor(c["log_std"], **F64)
    nb = int(lib.mpcrl_ppo_surrogate_workspace_bytes_nu(M, n_p, nu))
    assert nb == 16 + 8 * (n_p + 6 + nu - 1) * ((M + 127) // 128)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    n_msg = n_p + 8 + nu - 1
    for norm in (1, 0):
        msgs = []
        for _ in range(2):
            msg = torch.full((n_msg,), -5.0, **F64)
            assert _surrogate_call(lib, d, nu, ws, clip, ent, lr, norm, msg) == 0
            msgs.append(msg)
        torch.cuda.synchronize()
        assert torch.equal(msgs[0], msgs[1])                                   # same inputs, same bits
        assert int(ws.count_nonzero()) == 0                                    # the workspace is left zero
        ref = ppo_surrogate_terms_nu(**c, clip_range=clip, ent_coef=ent, lr=lr, normalize_adv=bool(norm))
        got = msgs[0].cpu()
        assert ref.shape == (n_msg,) and torch.isfinite(got).all() and torch.isfinite(ref).all()
        err = _rel(got.numpy(), ref.numpy())
        print(f"nu={nu} M={M} n_p={n_p} normalize={norm}: count {int(got[n_p + 1])}, clipped {int(got[n_p + 4])}, max rel err {err:.2e}")
        assert int(got[n_p + 1]) == int(ref[n_p + 1]) and (M == 1 or 0 < int(got[n_p + 1]) < M)
        assert M < 100 or 0 < int(got[n_p + 4]) < int(got[n_p + 1])             # rows inside and outside the clip band
        assert err <= 1e-12
        if nu == 1:                                                            # the one-control entry point: the same kernel, the same bits
            one = torch.full((n_p + 8,), -5.0, **F64)
            assert lib.mpcrl_ppo_surrogate_grad(_p(d["idx"]), M, d["logp"].numel(), _p(d["act"]), _p(d["logp"]), _p(d["adv"]), _p(d["ok"]), _p(d["u0_new"]),
                                                _p(d["status_new"]), _p(d["dpi_dp"]), n_p, _p(d["log_std"]), c["lo"][0], c["hi"][0], clip, ent, lr, norm,
                                                _p(ws), _p(one), _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(one, msgs[0])
    msg = torch.zeros(n_msg, **F64)
    assert _surrogate_call(lib, d, nu, None, clip, ent, lr, 1, msg) == -1
    assert _surrogate_call(lib, d, 0, ws, clip, ent, lr, 1, msg) == -1 and _surrogate_call(lib, d, 4, ws, clip, ent, lr, 1, msg) == -1
    assert _surrogate_call(lib, {**d, "lo": c["hi"]}, nu, ws, clip, ent, lr, 1, msg) == -1


def test_log_std_apply_nu_is_the_masked_mean():
    from mpc4rl_amd import _lib
    lib = _lib.load()
    n_p = 5
    for count, c in ((4.0, 4.0), (0.0, 1.0)):
        msg = torch.zeros(n_p + 10, **F64)
        msg[n_p], msg[n_p + 1], msg[n_p + 8], msg[n_p + 9] = -0.75, count, 0.5, -3.0
        msg[n_p + 2: n_p + 8] = 100.0                                         # the statistics: not read
        ls = torch.tensor([0.25, -1.0, 2.0], **F64)
        assert lib.mpcrl_ppo_log_std_apply_nu(_p(msg), n_p, 3, _p(ls), _stream()) == 0
        torch.cuda.synchronize()
        assert ls.tolist() == [0.25 + -0.75 / c, -1.0 + 0.5 / c, 2.0 + -3.0 / c]
        one = torch.tensor([0.25, -1.0, 2.0], **F64)
        assert lib.mpcrl_ppo_log_std_apply_nu(_p(msg), n_p, 1, _p(one), _stream()) == 0
        torch.cuda.synchronize()
        assert one.tolist() == [0.25 + -0.75 / c, -1.0, 2.0]
    assert lib.mpcrl_ppo_log_std_apply_nu(None, n_p, 3, _p(ls), _stream()) == -1
    assert lib.mpcrl_ppo_log_std_apply_nu(_p(msg), n_p, 4, _p(ls), _stream()) == -1


# ---------------------------------------------------------------------- 3. the gradient through the chain solver
@pytest.mark.parametrize("n_mass", [3, 5])
def test_surrogate_gradient_through_the_chain_solver_vs_finite_differences(oracle_port, n_mass):
    """The chain solve (du0*/dp [3][n_p]) -> mpcrl_ppo_surrogate_grad_nu: msg[k] / (-lr) against central finite differences of the summed
    surrogate through re-solves at theta' (1 +- 1e-5) in m_0, m_{nl-1} and one entry each of D, L, C; tolerance 1e-4 relative (the
    project's finite-difference rule).  N = 8, tol 1e-10, 64 states x0 + 0.05 N(0, 1); one roll-out row at the nominal
    theta through mpcrl_ppo_chain_collect with log_std = (-1, -0.7, -1.3), fixed advantages N(0.2, 1) without normalisation, the surrogate
    evaluated at theta' = theta with the m, D, L, C block x 1.01.  The CPU oracle port converges on all 64 instances at all 11 parameter
    points (asserted), so no instance is left out: the count is 64.  On the MI355X the largest relative difference of the five entries was
    2.6e-9 at n_mass 3 and 7.8e-8 at n_mass 5 (the port's own dpi gives 4e-9 and 8e-8)."""
    from mpc4rl_amd import MPCBatch, _lib
    from mpc4rl_amd.problems import chain_param_layout
    from oracle.problems import make_chain_mass
    lib = _lib.load()
    B, lr, clip = 64, 1e-3, 0.2
    ocp = _ocp(n_mass, tol=1e-10)
    M, nl, nx, nu, off, n_p = chain_param_layout(n_mass)
    rng = np.random.default_rng(3)
    x0 = np.array(ocp.x0) + 0.05 * rng.normal(size=(B, nx))
    nd = off["C"][1]                                                             # the m, D, L, C block
    th1 = np.array(ocp.p0, float)
    th1[:nd] *= 1.01
    ks = [off["m"][0], off["m"][1] - 1, off["D"][0] + 1, off["L"][0] + 3, off["C"][0] + 2]
    points = {"0": th1}
    for k in ks:
        for sgn in (+1, -1):
            th = th1.copy()
            th[k] += sgn * 1e-5 * th1[k]
            points[f"{k}{'+' if sgn > 0 else '-'}"] = th
    prob = make_chain_mass(n_mass, N=8)
    for th in [np.array(ocp.p0, float)] + list(points.values()):
        assert np.all(oracle_port.solve(prob, x0, p=th, flags=0, tol=1e-10).status == 0)
    mpc = MPCBatch(ocp, B, DEV)
    x0t = torch.as_tensor(x0, **F64)
    # the roll-out row at the nominal parameters, through the roll-out kernel
    r0 = mpc.solve(x0t, cold=True)
    lo, hi = [float(v) for v in ocp.lbu], [float(v) for v in ocp.ubu]
    state, steps = x0t.clone(), torch.zeros(B, dtype=torch.int64, device=DEV)
    tab = _Tables(1, B, nx)
    eps = torch.as_tensor(rng.normal(size=(B, 3)).astype(np.float32), device=DEV)
    log_std = torch.tensor([-1.0, -0.7, -1.3], **F64)
    obs, ended = torch.zeros(B, nx, **F64), torch.zeros(B, dtype=torch.int32, device=DEV)
    p0, x_ss = torch.tensor(ocp.p0, **F64), torch.tensor(ocp.consts, **F64)
    assert _chain_collect(lib, ocp, n_mass, p0, False, x_ss, 0.0, B, 1, 0, state, steps, r0.u0, r0.status, eps, None, torch.zeros(B, **F64), log_std, lo, hi,
                          -1.0, 10, torch.tensor(ocp.x0, **F64), 0.0, None, tab, obs, ended) == 0
    adv = torch.as_tensor(rng.normal(0.2, 1.0, B), **F64)
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    res, ok = {}, tab.OK[0].bool() & (r0.status == 0)
    for name, th in points.items():
        mpc.set_theta(torch.as_tensor(th))
        res[name] = mpc.solve(x0t, sens_pi=(name == "0"), cold=True)
        ok = ok & (res[name].status == 0)
    okt = ok.to(torch.uint8).contiguous()
    ws = torch.zeros(int(lib.mpcrl_ppo_surrogate_workspace_bytes_nu(B, n_p, 3)), dtype=torch.uint8, device=DEV)
    zeros = torch.zeros(B, 3, n_p, **F64)

    def surrogate(r):
        msg = torch.zeros(n_p + 10, **F64)
        assert lib.mpcrl_ppo_surrogate_grad_nu(_p(idx), B, B, _p(tab.ACT), _p(tab.LOGP), _p(adv), _p(okt), _p(r.u0), _p(r.status),
                                               _p(zeros if r.dpi_dp is None else r.dpi_dp), n_p, 3, _p(log_std), _d3(lo), _d3(hi), clip, 0.0, lr, 0, _p(ws),
                                               _p(msg), _stream()) == 0
        return msg.cpu().numpy()

    m0 = surrogate(res["0"])
    n_in = int(okt.sum())
    assert int(m0[n_p + 1]) == n_in == B                                          # no instance is left out
    grad = m0[ks] / (-lr)
    fd = np.array([(surrogate(res[f"{k}+"])[n_p + 2] - surrogate(res[f"{k}-"])[n_p + 2]) / (2e-5 * th1[k]) for k in ks])
    err = np.abs(grad - fd) / np.maximum(np.abs(fd), 1.0)
    print(f"n_mass {n_mass}: surrogate gradient", grad, "finite differences", fd, "rel err", err, "instances", n_in, "clipped rows", int(m0[n_p + 4]),
          "mean ratio", m0[n_p + 5] / n_in)
    assert np.abs(m0[n_p + 5] / n_in - 1.0) > 1e-6 and np.abs(fd).min() > 0.0        # the ratios moved; no difference is trivially zero
    assert np.all(np.isfinite(m0[:nd])) and np.all(np.isfinite(m0))                  # the learned block's other entries
    assert err.max() < 1e-4


# ---------------------------------------------------------------------- 4. the learner end to end
def _learner(learn=None, lr=1e-6, **kw):
    from mpc4rl_amd import BatchedChainMassEnv, BatchedPPO
    ocp = _ocp(3)
    env = BatchedChainMassEnv(8, ocp, device=DEV, w_std=0.05, seed=3)
    extra = {} if learn is None else dict(learn=learn)
    return BatchedPPO(ocp, env, n_steps=4, batch_size=16, n_epochs=1, episode_length=3, lr=lr, ent_coef=0.01, log_std_init=-1.0, seed=11, **extra, **kw)


def test_ppo_on_the_chain_end_to_end():
    """n_mass 3, N 8, E 8, n_steps 4, batch_size 16, episode_length 3, w_std 0.05: a roll-out against ppo_chain_collect_terms + ppo_gae on
    the recorded solves and draws (DONE on the rows the count says, the cold mask of the next solve, TERM zero), one minibatch's message
    against ppo_surrogate_terms_nu, then learn(1): theta moved on the learn mask only, log_std (3,) moved, statistics finite."""
    from mpc4rl_amd import ppo_chain_collect_terms, ppo_gae, ppo_surrogate_terms_nu
    from mpc4rl_amd.problems import chain_param_layout
    ppo = _learner()
    env, ocp, T, E, B, L = ppo.env, ppo.ocp, 4, 8, 16, 3
    off = chain_param_layout(3)[4]
    mask = torch.zeros(ppo.n_p, dtype=torch.bool)
    mask[: off["C"][1]] = True                                                      # m, D, L, C
    assert torch.equal(ppo.learn_mask.cpu() != 0.0, mask)
    assert ppo.ACT.shape == (T, E, 3) and ppo.OBS.shape == (T, E, ocp.nx) and ppo.LOGP.shape == (T, E) and ppo.log_std.shape == (3,)
    assert ppo.wn.shape == ppo.rn.shape == (T, E, 3) and ppo.msg.shape == (ppo.n_p + 10,) and isinstance(ppo.lo, tuple) and len(ppo.hi) == 3
    assert float(ppo.obs.abs().max()) > 0.0 and torch.equal(ppo.obs, env.state)                      # a state of the chain, not the zero state
    ws = ppo.workspace_bytes()
    assert ws == (ppo.rollout_mpc.workspace_bytes(), ppo.sample_mpc.workspace_bytes()) and ws[1] > ws[0] > 0
    rec, step = [], ppo._collect_step

    def recording(t):
        before = (env.state.clone(), ppo.steps.clone(), ppo.ended.clone())
        step(t)
        rec.append(before + ppo.last_collect)

    ppo._collect_step = recording
    ppo.collect()
    torch.cuda.synchronize()
    ppo._collect_step = step
    ls = ppo.log_std.cpu()
    worst = 0.0
    for t in range(T):
        s0, n0, cold, r, eps, wn, value, rn = [x.cpu() if torch.is_tensor(x) else x for x in rec[t]]
        assert torch.equal(wn, ppo.wn[t].cpu()) and torch.equal(rn, ppo.rn[t].cpu())
        o = ppo_chain_collect_terms(ocp, env.p.cpu(), env.x_ss.cpu(), s0, n0, r.u0.cpu(), r.status.cpu(), eps, wn, env.w_std, ls, ppo.lo, ppo.hi,
                                    ppo.reward_scale, L, ppo.x_reset.cpu(), env.vel_std, rn)
        assert _rel(ppo.ACT[t].cpu().numpy(), o["act"].numpy()) <= 1e-12 and _rel(ppo.LOGP[t].cpu().numpy(), o["logp"].numpy()) <= 1e-12
        assert torch.equal(ppo.OK[t].cpu().bool(), o["ok"]) and bool(o["ok"].all())
        assert torch.equal(ppo.OBS[t].cpu(), s0) and torch.equal(ppo.VAL[t].cpu(), value)
        e_n, e_r = _err(ppo.NEXT[t], o["next"]), _err(ppo.REW[t], o["rew"])
        worst = max(worst, e_n, e_r)
        assert e_n <= TOL and e_r <= TOL, (t, e_n, e_r)
        done = o["done"]
        assert torch.equal(ppo.DONE[t].cpu().bool(), done) and bool(done.all()) == (t % L == L - 1) == bool(done.any())
        nxt_state, nxt_cold = (rec[t + 1][0], rec[t + 1][2]) if t + 1 < T else (env.state, ppo.ended)
        assert torch.equal(nxt_cold.cpu().bool(), done)                               # the rows that ended start the next solve cold
        assert _err(nxt_state, o["state"]) <= TOL and torch.equal(nxt_state.cpu()[done], o["state"][done])
        assert torch.equal((ppo.steps if t + 1 == T else rec[t + 1][1]).cpu(), o["steps"])
    assert bool(rec[0][2].bool().all())                                              # the first solve starts every instance cold
    assert int(ppo.TERM.sum()) == 0 and int(ppo.DONE.sum()) == E and float(ppo.REW.max()) < 0.0
    adv, ret = ppo_gae(ppo.REW.cpu(), ppo.VAL.cpu(), ppo.VNEXT.cpu(), ppo.TERM.cpu(), ppo.DONE.cpu(), ppo.gamma, ppo.gae_lambda)
    assert _rel(ppo.ADV.cpu().numpy(), adv.numpy()) <= 1e-12 and _rel(ppo.RET.cpu().numpy(), ret.numpy()) <= 1e-12
    # one minibatch
    box, solve = {}, ppo.sample_mpc.solve

    def recording_solve(*a, **k):
        box["r"] = solve(*a, **k)
        return box["r"]

    ppo.sample_mpc.solve = recording_solve
    idx = torch.randperm(T * E, generator=torch.Generator().manual_seed(1))[:B].to(DEV).contiguous()
    theta0, ls0 = ppo.theta.clone(), ppo.log_std.clone()
    ppo._minibatch(idx)
    torch.cuda.synchronize()
    ppo.sample_mpc.solve = solve
    r = box["r"]
    assert r.dpi_dp.shape == (B, 3, ppo.n_p)
    ref = ppo_surrogate_terms_nu(idx.cpu(), ppo.ACT.cpu(), ppo.LOGP.cpu(), ppo.ADV.cpu(), ppo.OK.cpu(), r.u0.cpu(), r.status.cpu(), r.dpi_dp.cpu(), ls0.cpu(),
                                 ppo.lo, ppo.hi, ppo.clip_range, ppo.ent_coef, ppo.lr, ppo.normalize_advantage)
    got = ppo.msg.cpu()
    # As in tests/test_gpu_linear_loops.py: the re-solve runs at the roll-out's parameters, the ratios are 1 to the solver's tolerance and
    # entries n_p + 2 (sum loss = -sum of the normalised advantages) and n_p + 3 (sum (r - 1) - log r) are sums that cancel; they are held
    # to 1e-12 of the sum of the magnitudes of their terms, at most B.  Every other entry to 1e-12 relative.
    n_p = ppo.n_p
    loss, kl = n_p + 2, n_p + 3
    keep = ~np.isin(np.arange(n_p + 10), (loss, kl))
    per = np.abs(got.numpy() - ref.numpy()) / np.where(ref.numpy() != 0.0, np.abs(ref.numpy()), 1.0)
    err, err_c = float(per[keep].max()), float(np.abs(got.numpy() - ref.numpy())[[loss, kl]].max())
    print(f"table rows largest {worst:.3e}; surrogate message rel err {err:.3e}, cancelling sums {err_c:.3e}; count {int(got[n_p + 1])}; "
          f"log_std entries {got[[n_p, n_p + 8, n_p + 9]].tolist()}")
    assert err <= 1e-12 and err_c <= 1e-12 * B and int(got[n_p + 1]) == B
    step_out = ppo.step_out.cpu()
    assert np.array_equal(step_out[mask].numpy(), (got[:n_p] / B)[mask].numpy()) and float(step_out[~mask].abs().max()) == 0.0
    assert torch.equal(ppo.theta, theta0 + ppo.step_out) and int((step_out[mask] != 0.0).sum()) > 3
    want_ls = ls0.cpu() + torch.stack([got[n_p], got[n_p + 8], got[n_p + 9]]) / B
    assert torch.equal(ppo.log_std.cpu(), want_ls) and bool((ppo.log_std != ls0).all())
    assert torch.equal(ppo.rollout_mpc.get_theta(), ppo.theta) and torch.equal(ppo.sample_mpc.get_theta(), ppo.theta)
    # a whole iteration
    theta1, ls1 = ppo.theta.clone(), ppo.log_std.clone()
    ppo.learn(1)
    st = ppo.last_stats()
    torch.cuda.synchronize()
    print("PPO statistics on the chain of masses:", st)
    moved = (ppo.theta != theta1).cpu()
    assert int(moved.sum()) > 3 and not bool(moved[~mask].any()) and torch.equal(ppo.theta[~mask.to(DEV)], theta1[~mask.to(DEV)])
    assert ppo.log_std.shape == (3,) and bool((ppo.log_std != ls1).all())
    assert torch.isfinite(ppo.theta).all() and torch.isfinite(ppo.log_std).all() and torch.isfinite(ppo.ADV).all()
    assert all(math.isfinite(v) for v in st.values()) and st["valid_fraction"] == 1.0
    assert int(ppo._ws.count_nonzero()) == 0 and ppo.iterations == 1


def test_ppo_on_the_chain_with_lr_zero_and_another_block():
    """lr = 0: theta and log_std are bitwise unchanged by a learn iteration.  learn = ("C",): only the C block moves."""
    from mpc4rl_amd.problems import chain_param_layout
    ppo = _learner(lr=0.0)
    theta0, ls0 = ppo.theta.clone(), ppo.log_std.clone()
    ppo.learn(1)
    torch.cuda.synchronize()
    assert torch.equal(ppo.theta, theta0) and torch.equal(ppo.log_std, ls0) and ppo.last_stats()["valid_fraction"] == 1.0
    ppo = _learner(learn=("C",))
    off = chain_param_layout(3)[4]
    mask = torch.zeros(ppo.n_p, dtype=torch.bool)
    mask[off["C"][0]: off["C"][1]] = True
    assert torch.equal(ppo.learn_mask.cpu() != 0.0, mask)
    theta0 = ppo.theta.clone()
    ppo.learn(1)
    st = ppo.last_stats()
    torch.cuda.synchronize()
    moved = (ppo.theta != theta0).cpu()
    assert int(moved.sum()) > 3 and not bool(moved[~mask].any()) and st["valid_fraction"] == 1.0 and all(math.isfinite(v) for v in st.values())
