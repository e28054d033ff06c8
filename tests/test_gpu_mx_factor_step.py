"""The matrix-core factor sweep of the cartpole kernels (small_kernel.hpp, SmallSolver::mx_factor) through the probe export
mpcrl_debug_mx_factor (include/mpcrl_probe_ext.h; one wavefront, one launch): the sweep as the kernels run it (which = 1: p_k carried in
column 3 as well and stored from there, three stores a step; the pivot flag a lane mask; the only step that can be pinned peeled)
against the copy of the sweep as it was before (which = 0, in the probe's unit only).  The arithmetic of every stored value is the same
instruction sequence on the same operands, so the bar is equality of the bit patterns on everything a later phase reads: P_k, K, d, q,
p_k (with WANT_P), 1/R, kff, beta and the flag of each block.

Horizons 1, 2, 5, 20: 2, 3, 6, 21 lanes per instance, so 4, 4, 4, 3 instances in the wavefront — at N = 20 the fourth block is idle and
shadows block 0.  Each with u_0 pinned and free, and with and without p_k.  The reference copy itself is held to a numpy restatement of
the recursion (1e-9 of the largest entry: IEEE double, at most 20 well-conditioned steps, a reciprocal of ~1 ulp).

The second part is the QP set-up's `recentre` on warm starts: a cold solve and two warm ones of 7 instances (two wavefronts, the second
partly filled) at N = 20 against the CPU port, each warm-started from its own previous result — statuses and both iteration counts
equal, u0*, V, dV/dp, du0*/dp at the 1e-6 of the cartpole parity tests (tests/test_gpu_parity.py, tests/small_mode_cases.py: RTOL)."""
import numpy as np
import pytest
import torch

import small_mode_cases as C

pytestmark = pytest.mark.gpu

SLOT, WAVE = 66, 64
AH, COL, ROW, KK, MISC = 0, 32, 48, 56, 60      # the slot layout of small_kernel.hpp
HORIZONS = (1, 2, 5, 20)
SENTINEL = 7.0


def layout(N):
    lpi = N + 1
    return lpi, min(WAVE // lpi, 4)


def stage_data(N, seed):
    """[64, 66]: a well-conditioned stage in every lane's slot (A = I + 0.1 G, Hxx + D = 2 I + small symmetric, Huu + D >= 1)."""
    rng = np.random.default_rng(seed)
    s = np.full((WAVE, SLOT), SENTINEL)
    for lane in range(WAVE):
        A = np.eye(4) + 0.1 * rng.normal(size=(4, 4))
        G = 0.1 * rng.normal(size=(4, 4))
        H = 2.0 * np.eye(4) + 0.5 * (G + G.T)
        B, hxu, bb, gx = 0.3 * rng.normal(size=4), 0.05 * rng.normal(size=4), 0.1 * rng.normal(size=4), rng.normal(size=4)
        s[lane, AH:AH + 32:2], s[lane, AH + 1:AH + 32:2] = A.ravel(), H.ravel()
        s[lane, COL:COL + 16:4], s[lane, COL + 1:COL + 16:4] = B, hxu
        s[lane, COL + 2:COL + 16:4], s[lane, COL + 3:COL + 16:4] = bb, gx
        s[lane, ROW:ROW + 8:2] = [1.0 + rng.uniform(), rng.normal(), 0.0, 123.0]     # (entry 54 is the probe's: whatever is here is replaced)
        s[lane, ROW + 1:ROW + 8:2] = hxu
    return s


def run(slots, N, which, pin, want_p):
    from mpc4rl_amd import _lib
    dev = torch.device("cuda:0")
    xin = torch.as_tensor(slots, dtype=torch.float64, device=dev).contiguous()
    out = torch.full_like(xin, 12345.0)
    ok = torch.full((4,), 12345.0, dtype=torch.float64, device=dev)
    flags = (_lib.PROBE_MX_PIN if pin else 0) | (_lib.PROBE_MX_WANT_P if want_p else 0)
    assert _lib.call("mpcrl_debug_mx_factor", xin, N, flags, which, out, ok, device=dev) == 0
    return out, ok


def compared(N):
    """[64, 66] bool: everything but entry 54 where no step writes q_k[3] over it (terminal stages, lanes without a stage)."""
    lpi, ipw = layout(N)
    keep = np.ones((WAVE, SLOT), bool)
    for lane in range(WAVE):
        if lane >= ipw * lpi or lane % lpi == N:
            keep[lane, ROW + 6] = False
    return torch.as_tensor(keep, device="cuda:0")


def riccati(slots, N, blk, pin):
    """The recursion of one instance in numpy: {stage: (P, K, d, q, p, 1/R, kff, beta)}."""
    lpi, _ = layout(N)
    sl = slots[blk * lpi:(blk + 1) * lpi]
    P, p = sl[N, AH + 1:AH + 32:2].reshape(4, 4), sl[N, COL + 3:COL + 16:4]
    res = {}
    for k in range(N - 1, -1, -1):
        A, H = sl[k, AH:AH + 32:2].reshape(4, 4), sl[k, AH + 1:AH + 32:2].reshape(4, 4)
        B, hxu, bb, gx = sl[k, COL:COL + 16:4], sl[k, COL + 1:COL + 16:4], sl[k, COL + 2:COL + 16:4], sl[k, COL + 3:COL + 16:4]
        huu, gu = sl[k, ROW], sl[k, ROW + 2]
        y1, y2 = p + P @ bb, P @ bb
        Q, S = A.T @ P @ A + H, A.T @ P @ B + hxu
        R, mvu, beta = B @ P @ B + huu, B @ y1 + gu, B @ y2
        rinv = 0.0 if (pin and k == 0) else 1.0 / R
        K, kff = S * rinv, mvu * rinv
        P, p, q = Q - np.outer(K, S), A.T @ y1 + gx - K * mvu, A.T @ y2 - K * beta
        res[k] = (P, K, bb - B * kff, q, p, rinv, kff, beta)
    return res


def fields(row):
    """(P, K, d, q, p, 1/R, kff, beta) of one slot after the sweep."""
    return (row[AH + 1:AH + 32:2].reshape(4, 4), row[KK:KK + 4], row[COL + 3:COL + 16:4], row[ROW:ROW + 8:2], row[COL + 1:COL + 16:4],
            row[MISC], row[MISC + 1], row[MISC + 2])


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("N", HORIZONS)
def test_factor_step_equals_the_step_before(N):
    lpi, ipw = layout(N)
    assert (lpi, ipw) == {1: (2, 4), 2: (3, 4), 5: (6, 4), 20: (21, 3)}[N]
    slots = stage_data(N, 100 + N)
    keep = compared(N)
    for pin in (False, True):
        for want_p in (False, True):
            (o0, k0), (o1, k1) = run(slots, N, 0, pin, want_p), run(slots, N, 1, pin, want_p)
            torch.cuda.synchronize()
            tag = (N, pin, want_p)
            assert torch.equal(bits(o1)[keep], bits(o0)[keep]), tag
            assert torch.equal(bits(k1), bits(k0)), tag
            assert k0.tolist() == [1.0] * ipw + [-1.0] * (4 - ipw), (tag, k0.tolist())
            a = o0.cpu().numpy()
            assert np.array_equal(a[ipw * lpi:, :ROW + 6], slots[ipw * lpi:, :ROW + 6])            # lanes without a stage: untouched
            for blk in range(ipw):
                ref = riccati(slots, N, blk, pin)
                for k in range(N):
                    row = a[blk * lpi + k]
                    for name, got, want in zip(("P", "K", "d", "q", "p", "1/R", "kff", "beta"), fields(row), ref[k]):
                        if name == "p" and not want_p:
                            assert np.array_equal(got, slots[blk * lpi + k, COL + 1:COL + 16:4]), tag       # left as published (Hxu)
                            continue
                        err = np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))
                        assert err < 1e-9, (tag, blk, k, name, err)
                if pin:
                    assert np.all(a[blk * lpi, KK:KK + 4] == 0.0) and a[blk * lpi, MISC] == 0.0 and a[blk * lpi, MISC + 1] == 0.0


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("bad", (-1.0e3, 0.0, float("nan")))
def test_bad_pivot_clears_the_flag_of_its_block_only(N, bad):
    """Huu + D_u of one stage of one block so that R <= 0 (the block's P B is then garbage, finite or not) or R = NaN."""
    lpi, ipw = layout(N)
    keep = compared(N)
    for blk in range(ipw):
        slots = stage_data(N, 200 + N)
        stage = (N - 1) // 2
        slots[blk * lpi + stage, ROW] = bad
        if bad == 0.0:      # R = 0 exactly: no curvature at all in that stage (B = 0 as well)
            slots[blk * lpi + stage, COL:COL + 16:4] = 0.0
        want = [0.0 if b == blk else 1.0 for b in range(ipw)] + [-1.0] * (4 - ipw)
        for want_p in (False, True):
            (o0, k0), (o1, k1) = run(slots, N, 0, False, want_p), run(slots, N, 1, False, want_p)
            torch.cuda.synchronize()
            assert k0.tolist() == want and k1.tolist() == want, (N, bad, blk, k0.tolist(), k1.tolist())
            others = keep.clone()
            others[blk * lpi:(blk + 1) * lpi] = False
            assert torch.equal(bits(o1)[others], bits(o0)[others]), (N, bad, blk)
            mine = keep & ~others       # the block itself: the same values, any NaN equal to any NaN
            a, b = o0[mine], o1[mine]
            assert bool(((a == b) | (a.isnan() & b.isnan())).all()), (N, bad, blk)


@pytest.mark.parametrize("N", HORIZONS)
def test_pinned_stage_excuses_its_own_pivot_only(N):
    """Q-mode: the pivot of stage 0 is not looked at (u_0 is pinned, 1/R_0 = 0); every other stage's is."""
    lpi, ipw = layout(N)
    slots = stage_data(N, 300 + N)
    slots[0, ROW] = -1.0e3                     # block 0, stage 0
    if N >= 2:
        slots[lpi + 1, ROW] = float("nan")     # block 1, stage 1
    for which in (0, 1):
        _, ok = run(slots, N, which, True, True)
        assert ok.tolist() == [1.0] + ([0.0] if N >= 2 else [1.0]) + [1.0] * (ipw - 2) + [-1.0] * (4 - ipw), (N, which, ok.tolist())
        _, ok = run(slots, N, which, False, True)
        assert ok.tolist()[0] == 0.0, (N, which)


def test_probe_refuses_what_it_cannot_run():
    from mpc4rl_amd import _lib
    buf = torch.zeros(WAVE, SLOT, dtype=torch.float64, device="cuda:0")
    ok = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    for N, flags, which in ((0, 0, 1), (64, 0, 1), (20, 4, 1), (20, 0, 2), (20, 0, -1)):
        with pytest.raises(RuntimeError):
            _lib.call("mpcrl_debug_mx_factor", buf, N, flags, which, buf, ok, device="cuda:0")
    with pytest.raises(RuntimeError):
        _lib.call("mpcrl_debug_mx_factor", None, 20, 0, 1, buf, ok, device="cuda:0")


def test_recentred_warm_starts_vs_port(oracle_port):
    """Cold, warm, warm at moving states: every QP of the two warm calls (and every QP after an instance's first in the cold one) is set
    up from the previous QP's rows through `recentre`."""
    from mpc4rl_amd import MPCBatch
    B, N = 7, 20
    ocp, P = C.problem("cartpole", N)
    x0, _, step = C.inputs("cartpole")
    x0, step = x0[:B], step[:B]
    mpc = MPCBatch(ocp, B)
    ref = None
    for n in range(3):
        x = x0 + n * step
        r = mpc.solve(x, sens_v=True, sens_pi=True, cold=(n == 0))
        torch.cuda.synchronize()
        ref = oracle_port.solve(P, x, warm=ref)
        got = C.outputs(mpc, r)
        err = C.largest_error(got, ref, fields=("u0", "V", "dV", "dpi"))
        print(f"[factor step] call {n}: status {got['status'].tolist()} port {ref.status.tolist()}; SQP {got['iters'][:, 0].tolist()} port "
              f"{ref.sqp_iter.tolist()}; interior point {got['iters'][:, 1].tolist()} port {ref.ipm_iter.tolist()}; largest error {err:.3e} "
              f"{C.largest_error.last}")
        assert np.array_equal(got["status"], ref.status) and np.all(ref.status == 0), n
        assert np.array_equal(got["iters"][:, 0], ref.sqp_iter) and np.array_equal(got["iters"][:, 1], ref.ipm_iter), n
        assert err < C.RTOL, (n, C.largest_error.last)
        if n:
            assert np.all(ref.sqp_iter >= 1)      # a warm call that did set up QPs
