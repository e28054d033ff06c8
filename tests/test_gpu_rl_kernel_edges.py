"""GPU tests of the RL-loop kernels at the shapes and edges the loop tests do not reach: the TD kernel of the cartpole Q-learning loop,
the policy gradient's contraction, the steps after the collective, the two roll-out kernels and the K5 reduction (csrc/qlearning_kernel.hpp,
replay_kernel.hpp, td3_kernel.hpp, reduce_kernel.hpp) — ragged last workgroups, fewer workgroups than the four slices of the final sum, a
final sum of several 256-entry chunks, > 1000 workgroups, NULL optional arguments, reused workspaces and sentinel tails.  Every value is
checked against float64 torch / numpy: bit for bit where the kernel keeps the reference's order of operations; where it only reorders a
sum, to 1e-12 of the sum of the magnitudes of the terms of that entry (a bound that holds for any summation order)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.float64 else t


@pytest.fixture(scope="module")
def lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def _check_sum(got, ref, mag, rel=1e-12):
    """got, ref, mag: float64 numpy arrays; mag = the sum of |terms| of each entry (inf where a term overflows).  An entry whose reference
    is non-finite (an overflowing product) must be non-finite in the kernel too; every other one agrees to rel * mag."""
    assert np.all(~np.isfinite(got[~np.isfinite(ref)])), "the reference overflows where the kernel's entry is finite"
    fin = np.isfinite(ref) & np.isfinite(mag)
    err = np.abs(got[fin] - ref[fin])
    bad = ~(err <= rel * mag[fin])
    assert not bad.any(), (np.nonzero(fin)[0][bad][:8], got[fin][bad][:4], ref[fin][bad][:4])


# ---------------------------------------------------------------------------------------------------------------------------- TD kernel

# (T, E, n_p): one term; one ragged workgroup; a second workgroup of one row; 3 workgroups (< 4 slices); P2 = 256 (one chunk of the
# final sum), 257 (a second chunk of one entry); three chunks over 27 ragged workgroups
TD_SHAPES = [(3, 1, 1), (3, 127, 5), (3, 129, 7), (5, 128, 86), (7, 101, 254), (7, 101, 255), (12, 333, 600)]


def _td_inputs(T, E, n_p, seed):
    """An episode table with live prefixes of length T, 0, 1, 2, 3 (then random), failed Q and V solves (NaN Q, V, dQ/dp), and NaN /
    +inf / -inf in dQ/dp on terms that are valid and on terms that are left out."""
    from mpc4rl_amd import qlearning_td_terms
    rng = np.random.default_rng(seed)
    L = rng.integers(0, T + 1, E)
    L[: min(E, 5)] = [T, 0, 1, 2, 3][: min(E, 5)]
    live = (np.arange(T)[:, None] < L[None, :]).astype(np.uint8)
    cost = rng.uniform(0, 10, (T, E)) * live
    q, v = rng.normal(50, 10, (T - 1, E)), rng.normal(50, 10, (T - 1, E))
    dq = rng.normal(size=(T - 1, E, n_p))
    sq = np.where(rng.uniform(size=(T - 1, E)) < 0.08, 2, 0).astype(np.int32)
    sv = np.where(rng.uniform(size=(T - 1, E)) < 0.08, 1, 0).astype(np.int32)
    sq[:, 0], sv[:, 0] = 0, 0                    # (environment 0 runs the whole episode: (3, 1, 1) has its one term)
    q[sq != 0], v[sv != 0], dq[sq != 0] = np.nan, np.nan, np.nan
    if E > 1:
        _, _, valid = qlearning_td_terms(*[torch.as_tensor(a) for a in (q, v, dq, sq, sv, cost, live)], 0.99, 1.0)
        valid = valid.numpy()
        for sel in (valid, ~valid & (sq[: T - 2] == 0)):
            ii, ee = np.nonzero(sel)
            for k, bad in enumerate((np.nan, np.inf, -np.inf)[: len(ii)]):
                dq[ii[k], ee[k], (3 * k) % n_p] = bad
    return q, v, dq, sq, sv, cost, live, L


def _td_reference(inp, gamma, lr):
    """qlearning_td_terms (float64, CPU) and the magnitudes of the terms of every entry."""
    from mpc4rl_amd import qlearning_td_terms
    q, v, dq, sq, sv, cost, live, L = inp
    msg, td, valid = qlearning_td_terms(*[torch.as_tensor(a) for a in (q, v, dq, sq, sv, cost, live)], gamma, lr)
    T = cost.shape[0]
    w = torch.where(valid, lr * td, torch.zeros_like(td))
    g = torch.nan_to_num(torch.as_tensor(dq[: T - 2])) * valid[..., None]
    mag = torch.cat([(w[..., None] * g).abs().sum((0, 1)), w.abs().sum().reshape(1), torch.zeros(1, dtype=torch.float64)])
    return msg.numpy(), td.numpy(), valid.numpy(), mag.numpy()


def _script_loop(inp, gamma, lr):
    """scripts/cartpole_mpc_qlearning.py:236-263 per environment (n = size - 1 samples, td[:-1]; failed solves left out; dQ/dp read as
    nan_to_num)."""
    q, v, dq, sq, sv, cost, live, L = inp
    g, ws, cnt = np.zeros(dq.shape[-1]), 0.0, 0
    for e in range(len(L)):
        n = int(L[e]) - 1
        if n < 2:
            continue
        td = cost[: n - 1, e] + gamma * v[1:n, e] - q[: n - 1, e]
        for i in range(n - 1):
            if sq[i, e] == 0 and sv[i, e] == 0 and sq[i + 1, e] == 0 and sv[i + 1, e] == 0:
                g, ws, cnt = g + lr * td[i] * np.nan_to_num(dq[i, e]), ws + lr * td[i], cnt + 1
    return g, ws, cnt


def _dev(inp):
    return [torch.as_tensor(a, device=DEV).contiguous() for a in inp[:7]]


def _td_call(lib, d, T, E, n_p, gamma, lr, ws, stream=None):
    td = torch.full((T - 2, E), -5.0, **F64)
    valid = torch.full((T - 2, E), 9, dtype=torch.uint8, device=DEV)
    msg = torch.full((n_p + 2 + 3,), -5.0, **F64)                # three sentinels past the message
    assert lib.mpcrl_qlearning_td_grad(*[_p(t) for t in d], T, E, n_p, gamma, lr, _p(ws), _p(td), _p(valid), _p(msg),
                                       _stream() if stream is None else stream) == 0
    return msg, td, valid


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _td_check(got, ref, n_p):
    msg, td, valid = [t.cpu().numpy() for t in got]
    mr, tdr, vr, mag = ref
    assert np.array_equal(valid, vr.astype(np.uint8)) and np.array_equal(td, tdr)
    assert np.all(msg[n_p + 2:] == -5.0)
    assert msg[n_p + 1] == mr[n_p + 1] == vr.sum()                 # the count, exactly
    _check_sum(msg[: n_p + 1], mr[: n_p + 1], mag[: n_p + 1])


@pytest.mark.parametrize("T,E,n_p", TD_SHAPES)
def test_td_grad_shapes(lib, T, E, n_p):
    """mpcrl_qlearning_td_grad against qlearning_td_terms and the script's per-environment loop, lr = 1e-4 (finite products) and
    lr = 0.5 (w_j nan_to_num(+-inf) overflows: the entry must be non-finite in the kernel too); two calls give the same bits and leave
    the ticket zero."""
    inp = _td_inputs(T, E, n_p, seed=T * 1000 + E + n_p)
    d = _dev(inp)
    ws = torch.zeros(int(lib.mpcrl_qlearning_td_workspace_bytes(T, E, n_p)), dtype=torch.uint8, device=DEV)
    gamma = 0.99
    for lr in (1e-4, 0.5):
        ref = _td_reference(inp, gamma, lr)
        a = _td_call(lib, d, T, E, n_p, gamma, lr, ws)
        torch.cuda.synchronize()
        assert int(ws[:16].count_nonzero()) == 0                   # the ticket is left zero
        b = _td_call(lib, d, T, E, n_p, gamma, lr, ws)
        torch.cuda.synchronize()
        assert int(ws[:16].count_nonzero()) == 0 and _same_bits(a, b)
        _td_check(a, ref, n_p)
        if lr == 1e-4:
            g, wsum, cnt = _script_loop(inp, gamma, lr)
            mag, msg = ref[3], a[0].cpu().numpy()
            _check_sum(msg[:n_p], g, mag[:n_p])
            assert abs(msg[n_p] - wsum) <= 1e-12 * mag[n_p] and msg[n_p + 1] == cnt
        assert int(ref[2].sum()) >= (1 if E == 1 else 2)


def test_td_grad_one_workspace_across_shapes_and_two_streams(lib):
    """One workspace, sized for the largest shape, reused by every shape in turn (partials left over from a larger launch), every
    shape twice; then two shapes at once on two streams, each with its own workspace: the bits of the serial calls."""
    gamma, lr = 0.97, 1e-3
    ws = torch.zeros(max(int(lib.mpcrl_qlearning_td_workspace_bytes(*s)) for s in TD_SHAPES), dtype=torch.uint8, device=DEV)
    serial = {}
    for s in sorted(TD_SHAPES, key=lambda s: -s[0] * s[1] * s[2]) + TD_SHAPES:
        inp = _td_inputs(*s, seed=7 + sum(s))
        out = _td_call(lib, _dev(inp), *s, gamma, lr, ws)
        torch.cuda.synchronize()
        assert int(ws[:16].count_nonzero()) == 0
        _td_check(out, _td_reference(inp, gamma, lr), s[2])
        if s in serial:
            assert _same_bits(out, serial[s])
        serial[s] = out
    shapes = [(12, 333, 600), (7, 101, 255)]
    inps = [_dev(_td_inputs(*s, seed=7 + sum(s))) for s in shapes]
    wss = [torch.zeros(int(lib.mpcrl_qlearning_td_workspace_bytes(*s)), dtype=torch.uint8, device=DEV) for s in shapes]
    streams = [torch.cuda.Stream(DEV) for _ in shapes]
    torch.cuda.synchronize()
    outs = []
    for s, d, w, st in zip(shapes, inps, wss, streams):
        with torch.cuda.stream(st):
            outs.append(_td_call(lib, d, *s, gamma, lr, w, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for s, out, w in zip(shapes, outs, wss):
        assert int(w[:16].count_nonzero()) == 0 and _same_bits(out, serial[s])


def test_td_grad_many_workgroups_same_bits(lib):
    """T = 12, E = 13000: 1016 workgroups, the last-workgroup hand-off across the XCDs — ten calls, the same bits, the reference."""
    T, E, n_p, gamma, lr = 12, 13000, 10, 0.99, 1e-4
    inp = _td_inputs(T, E, n_p, seed=11)
    d = _dev(inp)
    ws = torch.zeros(int(lib.mpcrl_qlearning_td_workspace_bytes(T, E, n_p)), dtype=torch.uint8, device=DEV)
    outs = [_td_call(lib, d, T, E, n_p, gamma, lr, ws) for _ in range(10)]
    torch.cuda.synchronize()
    assert int(ws[:16].count_nonzero()) == 0
    assert all(_same_bits(o, outs[0]) for o in outs[1:])
    _td_check(outs[0], _td_reference(inp, gamma, lr), n_p)


# ---------------------------------------------------------------------------------------------------------------------------- DPG kernel

@pytest.mark.parametrize("B,nu,n_p", [(1, 1, 1), (32, 8, 255), (33, 5, 256), (97, 7, 300), (100, 8, 600), (40000, 1, 83)])
def test_dpg_grad_shapes(lib, B, nu, n_p):
    """mpcrl_dpg_grad against the einsum of td3.py in float64: one row; nu up to 8 (the w[32][8] table); P1 = 256, 257 (a second chunk
    of one entry), 301, 601 (three chunks); 1250 workgroups; scale on and off with asymmetric bounds; a random ok, ok = NULL and an ok of
    zeros; non-finite sensitivities on rows left in and left out.  Two calls: the same bits, the ticket left zero, sentinels kept."""
    g = torch.Generator(device=DEV).manual_seed(B + nu + n_p)
    dq = torch.randn(B, nu, generator=g, device=DEV) * 3.0
    dpi = torch.randn(B, nu, n_p, generator=g, **F64)
    if n_p > 3:
        dpi[0, 0, 3] = float("nan")
    if B > 4:
        dpi[1] = float("nan")
        dpi[4, nu - 1, 7 % n_p] = float("inf")
        dpi[2, 0, n_p - 1] = float("-inf")
    lo = -torch.rand(nu, generator=g, **F64) - 0.5
    hi = torch.rand(nu, generator=g, **F64) * 3.0 + 0.1
    ok_rand = (torch.rand(B, generator=g, device=DEV) < 0.8).to(torch.uint8)
    ok_rand[0] = 1
    if B > 4:
        ok_rand[1], ok_rand[2], ok_rand[4] = 0, 0, 1
    ws = torch.zeros(int(lib.mpcrl_dpg_workspace_bytes(B, n_p)), dtype=torch.uint8, device=DEV)
    for ok in (ok_rand, None, torch.zeros(B, dtype=torch.uint8, device=DEV)):
        okb = torch.ones(B, dtype=torch.bool, device=DEV) if ok is None else ok.bool()
        for scale in (1, 0):
            outs = []
            for _ in range(2):
                out = torch.full((3 + n_p + 1 + 3,), -1.0, **F64)
                assert lib.mpcrl_dpg_grad(_p(dq), _p(ok), _p(dpi), B, nu, n_p, _p(lo), _p(hi), scale, _p(ws), _p(out[3:]), _stream()) == 0
                outs.append(out)
            torch.cuda.synchronize()
            assert int(ws[:16].count_nonzero()) == 0 and torch.equal(_bits(outs[0]), _bits(outs[1]))
            out = outs[0].cpu().numpy()
            assert np.all(out[:3] == -1.0) and np.all(out[-3:] == -1.0)
            chain = 2.0 / (hi - lo) if scale else torch.ones_like(lo)
            w = torch.where(okb[:, None], dq.double() * chain, 0.0)
            t = w[:, :, None] * torch.nan_to_num(dpi)
            ref = torch.einsum("bu,bup->p", w, torch.nan_to_num(dpi))
            ref = torch.where(torch.isfinite(t).all(1).all(0), ref, t.sum((0, 1)))      # (an overflowing product: a non-finite sum)
            _check_sum(out[3: 3 + n_p], ref.cpu().numpy(), t.abs().sum((0, 1)).cpu().numpy())
            assert out[3 + n_p] == float(okb.sum())


# ------------------------------------------------------------------------------------------------------------- steps after the collective

@pytest.mark.parametrize("n_theta", [1, 86, 256, 257, 1000])
def test_qlearning_apply(lib, n_theta):
    """mpcrl_qlearning_apply: step = msg / max(1, count) bit for bit on the learnable entries and theta + step bit for bit, count 0, 1
    and 7; a masked entry keeps its theta bits and gets step 0 even where its message is NaN or +-inf; mask = NULL; nothing past n_theta
    is written."""
    rng = np.random.default_rng(n_theta)
    for use_mask in (True, False):
        for count in (0.0, 1.0, 7.0):
            msg = rng.normal(size=n_theta + 2) * 1e-2
            msg[n_theta + 1] = count
            mask = (rng.uniform(size=n_theta) < 0.6) * rng.choice([1.0, 0.5], n_theta)
            if n_theta == 1:
                mask[0] = float(count != 1.0)
            if use_mask:
                bad = np.nonzero(mask == 0)[0]
                msg[bad] = np.resize([np.nan, np.inf, -np.inf], len(bad))
            theta = rng.normal(size=n_theta + 8)
            theta[n_theta:] = 123.25
            th_d, msg_d = torch.as_tensor(theta, device=DEV), torch.as_tensor(msg, device=DEV)
            st_d = torch.full((n_theta + 8,), -9.5, **F64)
            mask_d = torch.as_tensor(mask, device=DEV) if use_mask else None
            assert lib.mpcrl_qlearning_apply(_p(msg_d), n_theta, _p(mask_d), _p(th_d), _p(st_d), _stream()) == 0
            torch.cuda.synchronize()
            th_g, st_g = th_d.cpu().numpy(), st_d.cpu().numpy()
            learn = mask != 0 if use_mask else np.ones(n_theta, bool)
            with np.errstate(invalid="ignore"):
                st_ref = np.where(learn, msg[:n_theta] / max(1.0, count), 0.0)
            assert np.array_equal(st_g[:n_theta].view(np.uint64), st_ref.view(np.uint64))
            assert np.array_equal(th_g[:n_theta].view(np.uint64), (theta[:n_theta] + st_ref).view(np.uint64))
            assert np.array_equal(th_g[:n_theta][~learn].view(np.uint64), theta[:n_theta][~learn].view(np.uint64))
            assert np.all(st_g[:n_theta][~learn] == 0.0)
            assert np.all(th_g[n_theta:] == 123.25) and np.all(st_g[n_theta:] == -9.5)


@pytest.mark.parametrize("n_crit", [0, 5, 86, 10000])
@pytest.mark.parametrize("n_theta", [1, 86, 300])
def test_td3_policy_post(lib, n_theta, n_crit):
    """mpcrl_td3_policy_post: step = lr mask msg / max(1, count) bit for bit (the same operation order), theta + step bit for bit, theta'
    within 2 ulp of (1 - tau) theta' + tau theta (the compiler may contract it to an FMA), the target critics within float32 rounding of
    their float64 Polyak update, over a grid sized by max(n_theta, n_crit) (n_crit = 0: no critic pointers); nothing past n_theta or
    n_crit is written.  A masked (frozen) entry keeps its theta bits and gets step 0 even where its message is NaN or +-inf."""
    rng = np.random.default_rng(n_theta * 7 + n_crit)
    lr, tau = 3e-3, 0.005
    for count in (0.0, 7.0):
        msg = rng.normal(size=n_theta + 1)
        msg[n_theta] = count
        mask = (rng.uniform(size=n_theta) < 0.6) * rng.choice([1.0, 0.5], n_theta)
        if n_theta == 1:
            mask[0] = float(count == 0.0)
        bad = np.nonzero(mask == 0)[0]
        msg[bad] = np.resize([np.nan, np.inf, -np.inf], len(bad))
        theta = rng.uniform(0.5, 2.0, n_theta + 8) * rng.choice([-1.0, 1.0], n_theta + 8)
        theta_t = theta * (1.0 + 0.1 * rng.normal(size=n_theta + 8))         # (the same sign: no cancellation in the Polyak update)
        theta[n_theta:], theta_t[n_theta:] = 77.5, -77.5
        crit = rng.normal(size=n_crit + 8).astype(np.float32)
        crit_t = (crit * (1.0 + 0.1 * rng.normal(size=n_crit + 8))).astype(np.float32)
        crit_t[n_crit:] = 5.5
        d = {k: torch.as_tensor(v, device=DEV) for k, v in dict(msg=msg, mask=mask, theta=theta, theta_t=theta_t, crit=crit, crit_t=crit_t).items()}
        step = torch.full((n_theta + 8,), -9.5, **F64)
        cp, ctp = (_p(d["crit"]), _p(d["crit_t"])) if n_crit else (None, None)
        assert lib.mpcrl_td3_policy_post(_p(d["msg"]), n_theta, lr, _p(d["mask"]), tau, _p(d["theta"]), _p(d["theta_t"]), _p(step), cp, ctp,
                                         n_crit, _stream()) == 0
        torch.cuda.synchronize()
        th, tht, st, ct = d["theta"].cpu().numpy(), d["theta_t"].cpu().numpy(), step.cpu().numpy(), d["crit_t"].cpu().numpy()
        n, learn = n_theta, mask != 0
        with np.errstate(invalid="ignore"):
            st_ref = np.where(learn, lr * mask * msg[:n] / max(1.0, count), 0.0)
        th_ref = theta[:n] + st_ref
        assert np.array_equal(th[:n][~learn].view(np.uint64), theta[:n][~learn].view(np.uint64)), "a frozen entry moved"
        assert np.all(st[:n][~learn] == 0.0) and np.all(np.isfinite(tht[:n]))
        assert np.array_equal(st[:n].view(np.uint64), st_ref.view(np.uint64))
        assert np.array_equal(th[:n].view(np.uint64), th_ref.view(np.uint64))
        tht_ref = (1.0 - tau) * theta_t[:n] + tau * th_ref
        assert np.all(np.abs(tht[:n] - tht_ref) <= 2.0 * np.spacing(np.abs(tht_ref)))
        assert np.all(th[n:] == 77.5) and np.all(tht[n:] == -77.5) and np.all(st[n:] == -9.5)
        if n_crit:
            ct_ref = (1.0 - tau) * crit_t[:n_crit].astype(np.float64) + tau * crit[:n_crit].astype(np.float64)
            assert np.all(np.abs(ct[:n_crit] - ct_ref) <= 2.0 ** -22 * np.abs(ct_ref))
        assert np.all(ct[n_crit:] == 5.5)


# ------------------------------------------------------------------------------------------------------------------------- argument limits

def test_argument_refusals_at_the_limits(lib):
    """nx + nu = 65 (> CRITIC_DMAX), n_critics = 3 (and 0) and dpg nu = 9 are refused (-1) before anything is launched; the limits
    themselves are accepted by the workspace queries."""
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = _p(buf)
    assert lib.mpcrl_critic_workspace_bytes(8, 60, 5, 2) == -1 and lib.mpcrl_critic_workspace_bytes(8, 4, 1, 3) == -1
    assert lib.mpcrl_critic_workspace_bytes(8, 60, 4, 2) > 0 and lib.mpcrl_critic_workspace_bytes(8, 4, 1, 1) > 0
    for nx, nu, nc in ((60, 5, 2), (4, 1, 3), (4, 1, 0)):
        assert lib.mpcrl_critic_td_grad(p, 2 * nx + nu + 2, 8, nx, nu, p, p, p, p, nc, 0.99, 1.0, p, p, p, p, _stream()) == -1
    assert lib.mpcrl_critic_dq_da(p, 65, 8, 60, 5, p, p, p, p, p, _stream()) == -1
    assert lib.mpcrl_dpg_grad(p, None, p, 4, 9, 3, p, p, 1, p, p, _stream()) == -1
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0


# ------------------------------------------------------------------------------------------------------------------------ roll-out kernels

@pytest.mark.parametrize("E", [1, 255, 257, 1000])
def test_qlearning_cartpole_collect_rows_and_nulls(lib, E):
    """mpcrl_qlearning_cartpole_collect with environments on different table rows (0, T - 1, T = a full table, and in between), alive
    and dead ones, over three calls, against mpcrl_policy_action + the clip in torch + BatchedCartPoleSwingUpEnv.step + the table writes
    per environment, bit for bit; a full table writes nothing; the same calls with obs = NULL and cold = NULL change nothing else."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv
    T, sigma, lo, hi, K = 6, 0.1, -30.0, 30.0, 3
    g = torch.Generator(device=DEV).manual_seed(E)
    x0 = (torch.rand(E, 4, generator=g, **F64) * 2 - 1) * torch.tensor([0.5, 1.0, 0.3, 1.0], **F64)
    x0[::7] = torch.tensor([0.01, 0.0, 0.005, 0.0], **F64)                # inside the goal box: terminated at their first step
    row0 = torch.randint(0, T + 1, (E,), generator=g, device=DEV).to(torch.int32)
    row0[0::3], row0[1::3], row0[2::5] = 0, T - 1, T
    if E == 1:
        row0[0] = T - 1
    alive0 = (torch.rand(E, generator=g, device=DEV) < 0.85).to(torch.uint8)
    alive0[0] = 1
    steps0 = torch.randint(0, 3, (E,), generator=g, device=DEV)
    eps = torch.randn(T, E, generator=g, dtype=torch.float32, device=DEV)
    U0 = (torch.rand(K, E, generator=g, **F64) * 2 - 1) * 35.0
    ST = torch.where(torch.rand(K, E, generator=g, **F64) < 0.15, torch.randint(1, 4, (K, E), generator=g, device=DEV), 0).to(torch.int32)
    U0[ST == 1] = float("nan")
    U0[:, ::7], ST[:, ::7] = 0.0, 0
    envs = [BatchedCartPoleSwingUpEnv(E, device=DEV, seed=0, max_episode_steps=4) for _ in range(3)]
    runs = []
    for k, with_opt in enumerate((True, False)):
        env = envs[k]
        env.state.copy_(x0), env.steps.copy_(steps0)
        alive, row = alive0.clone(), row0.clone()
        obs = torch.full((E, 4), -3.0, **F64) if with_opt else None
        cold = torch.full((E,), 5, dtype=torch.int32, device=DEV) if with_opt else None
        S, A, Cc = torch.full((T, E, 4), -1.0, **F64), torch.full((T, E), -1.0, **F64), torch.full((T, E), -1.0, **F64)
        live = torch.full((T, E), 7, dtype=torch.uint8, device=DEV)
        obs_seen = []
        for t in range(K):
            assert lib.mpcrl_qlearning_cartpole_collect(env._par(), E, T, _p(env.state), _p(env.steps), _p(U0[t].contiguous()), _p(ST[t].contiguous()),
                                                        _p(eps), lo, hi, sigma, _p(obs), _p(alive), _p(row), _p(cold), _p(S), _p(A), _p(Cc), _p(live),
                                                        _stream()) == 0
            if with_opt:
                obs_seen.append(obs.clone())
        runs.append((env.state, env.steps, alive, row, S, A, Cc, live, obs_seen, cold))
    # the separate launches, per environment at its own row
    ref = envs[2]
    ref.state.copy_(x0), ref.steps.copy_(steps0)
    al, row = alive0.bool().clone(), row0.clone().long()
    lo_t, hi_t = torch.tensor([lo], **F64), torch.tensor([hi], **F64)
    Sr, Ar, Cr = torch.full((T, E, 4), -1.0, **F64), torch.full((T, E), -1.0, **F64), torch.full((T, E), -1.0, **F64)
    Lr = torch.full((T, E), 7, dtype=torch.uint8, device=DEV)
    obs_r, cold_r, ar = torch.full((E, 4), -3.0, **F64), torch.full((E,), 5, dtype=torch.int32, device=DEV), torch.arange(E, device=DEV)
    obs_ref = []
    for t in range(K):
        a = torch.empty(E, 1, dtype=torch.float32, device=DEV)
        assert lib.mpcrl_policy_action(_p(U0[t].contiguous()), _p(ST[t].contiguous()), None, _p(lo_t), _p(hi_t), E, 1, 1, 0.0, 0.0, 1, _p(a), None,
                                       _stream()) == 0
        wr = row < T
        a = torch.clamp(a[:, 0] + sigma * eps[row.clamp(max=T - 1), ar], -1.0, 1.0)
        old, old_steps = ref.state.clone(), ref.steps.clone()
        _, rew, term, trunc = ref.step(a)
        stepped = al & wr
        ref.state.copy_(torch.where(stepped[:, None], ref.state, old)), ref.steps.copy_(torch.where(stepped, ref.steps, old_steps))
        i, r = ar[wr], row[wr]
        Sr[r, i] = old[i]
        Ar[r, i] = torch.where(al, 0.5 * (hi - lo) * (a.to(torch.float64) + 1.0) + lo, torch.zeros_like(rew))[i]
        Cr[r, i] = torch.where(al, rew, torch.zeros_like(rew))[i]
        Lr[r, i] = al.to(torch.uint8)[i]
        obs_r[i] = ref.state[i]
        cold_r[i] = 0
        obs_ref.append(obs_r.clone())
        al = torch.where(stepped, al & ~(term | trunc), al)
        row = torch.where(wr, row + 1, row)
    torch.cuda.synchronize()
    (st, sp, alive, row_k, S, A, Cc, live, obs_seen, cold), other = runs
    assert torch.equal(st, ref.state) and torch.equal(sp, ref.steps) and torch.equal(alive, al.to(torch.uint8)) and torch.equal(row_k.long(), row)
    assert torch.equal(S, Sr) and torch.equal(A, Ar) and torch.equal(Cc, Cr) and torch.equal(live, Lr)
    assert all(torch.equal(x, y) for x, y in zip(obs_seen, obs_ref)) and torch.equal(cold, cold_r)
    assert all(torch.equal(x, y) for x, y in zip(runs[0][:8], other[:8]))
    full = row0 == T
    assert bool((row_k == torch.clamp(row0 + K, max=T)).all()) and bool((cold[full] == 5).all()) and (E < 3 or int(full.sum()) > 0)
    last = row0 == T - 1
    assert int(last.sum()) > 0 and int(live[T - 1][last].sum()) > 0


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("E", [1, 256, 257])
def test_td3_cartpole_collect_wrap_and_stats(lib, E, cap):
    """mpcrl_td3_cartpole_collect with one workgroup (E = 1, 256) and a ragged second one (257), a one-slot and a three-slot table over
    cap + 2 calls (the write position wraps), the workspace of 2 + 3 nblocks doubles that td3.py allocates: the replay rows, states,
    position and statistics (counts exact, reward sum to 1e-12) against the launches it stands for; the ticket is left zero."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv
    gen = torch.Generator(device=DEV).manual_seed(E * 10 + cap)
    env = BatchedCartPoleSwingUpEnv(E, device=DEV, seed=0, max_episode_steps=3)
    env.state.copy_(torch.randn(E, 4, generator=gen, **F64) * torch.tensor([0.5, 1.0, 3.0, 2.0], **F64))
    env.state[::5] *= 0.01                                   # some inside the terminal box after the step
    env.steps.copy_(torch.randint(0, 3, (E,), generator=gen, device=DEV))
    lo, hi = torch.tensor([-30.0], **F64), torch.tensor([30.0], **F64)
    st = _stream()
    state1, steps1 = env.state.clone(), env.steps.clone()
    obs, ended = env.state.clone(), torch.zeros(E, dtype=torch.int32, device=DEV)
    table, pos = torch.zeros(cap, E, 11, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    iter_ok, rows = torch.zeros(cap, E, dtype=torch.uint8, device=DEV), torch.zeros(E, dtype=torch.int64, device=DEV)
    nb = (E + 255) // 256
    stats, ws = torch.zeros(3, **F64), torch.zeros(2 + 3 * nb, **F64)
    ref_table, ref_rew, ref_conv, ref_done, rew_mag = torch.zeros_like(table), 0.0, 0, 0, 0.0
    for call in range(cap + 2):
        u0 = torch.randn(E, 1, generator=gen, **F64) * 20
        status = torch.randint(0, 5, (E,), generator=gen, device=DEV, dtype=torch.int32)
        eps = torch.randn(E, 1, generator=gen, device=DEV)
        u01 = torch.rand(E, generator=gen, **F64)
        u0[::5], eps[::5], status[::5] = 0.0, 0.0, 0             # (no force: the near-origin states stay in the terminal box)
        if call % 2:
            u0[0] = float("nan")
        a, ok = torch.empty(E, 1, device=DEV), torch.empty(E, dtype=torch.uint8, device=DEV)
        assert lib.mpcrl_policy_action(_p(u0), _p(status), _p(eps), _p(lo), _p(hi), E, 1, 1, 0.1, 0.0, 1, _p(a), _p(ok), st) == 0
        obs_before = env.state.clone()
        nxt, rew, term, trunc = env.step(a)
        done = term | trunc
        m8, new_obs = done.to(torch.uint8), torch.empty(E, 4, **F64)
        assert lib.mpcrl_env_cartpole_reset(E, _p(env.state), _p(env.steps), _p(m8), _p(u01), _p(new_obs), 0, st) == 0
        slot = call % cap
        ref_table[slot] = torch.cat([obs_before.float(), nxt.float(), a, (-1.0 * rew).float()[:, None], term.float()[:, None]], dim=1)
        ref_rew, rew_mag = ref_rew + float(rew.sum()), rew_mag + float(rew.abs().sum())
        ref_conv, ref_done = ref_conv + int((status == 0).sum()), ref_done + int(done.sum())
        assert lib.mpcrl_td3_cartpole_collect(env._par(), E, _p(state1), _p(steps1), _p(u0), _p(status), _p(eps), _p(u01), -30.0, 30.0, 1, 0.1,
                                              _p(obs), _p(ended), _p(table), cap, -1.0, _p(pos), _p(iter_ok), _p(rows), _p(stats), _p(ws), st) == 0
        torch.cuda.synchronize()
        assert int(pos) == (call + 1) % cap and float(ws[0]) == 0.0
        assert torch.equal(table, ref_table)
        assert torch.equal(state1, env.state) and torch.equal(steps1, env.steps) and torch.equal(obs, new_obs) and torch.equal(ended.bool(), done)
        assert torch.equal(iter_ok[slot].bool(), ok.bool() & (status == 0)) and torch.equal(rows, slot * E + torch.arange(E, device=DEV))
        assert float(stats[1]) == ref_conv and float(stats[2]) == ref_done
        assert abs(float(stats[0]) - ref_rew) <= 1e-12 * rew_mag
    assert ref_done > 0


# ------------------------------------------------------------------------------------------------------------------------------- K5 reduce

@pytest.mark.parametrize("n", [16, 17])
def test_weighted_grad_sum(lib, n):
    """mpcrl_weighted_grad_sum on both sides of the row-parallel / column-parallel switch (REDUCE_MAXN_ROWPAR = 16), a strided ld > n
    whose padding holds NaN (never to be read), weight = NULL, rows = 0 (all zeros, the count included), 70000 rows (the grid-stride
    loop); against float64 torch; nothing past out[n + 1] is written."""
    ld = n + 3
    for rows in (0, 1, 300, 70000):
        g = torch.randn(max(rows, 1), ld, **F64)
        g[:, n:] = float("nan")
        w = torch.randn(max(rows, 1), **F64)
        for weight in (w, None):
            out = torch.full((n + 2 + 4,), -7.0, **F64)
            assert lib.mpcrl_weighted_grad_sum(_p(g), ld, _p(weight), rows, n, _p(out), _stream()) == 0
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.all(o[n + 2:] == -7.0) and o[n + 1] == rows
            ww = (w if weight is not None else torch.ones_like(w))[:rows]
            t = ww[:, None] * g[:rows, :n]
            _check_sum(o[:n], t.sum(0).cpu().numpy(), t.abs().sum(0).cpu().numpy())
            _check_sum(o[n: n + 1], ww.sum().reshape(1).cpu().numpy(), ww.abs().sum().reshape(1).cpu().numpy())
            if rows == 0:
                assert np.all(o[: n + 2] == 0.0)
