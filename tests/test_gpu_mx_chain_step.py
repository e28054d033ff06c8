"""The affine chains of the cartpole kernels' vector sweeps (small_kernel.hpp, SmallSolver::mx_chain) through the probe export
mpcrl_debug_mx_chain (include/mpcrl_probe_chain_ext.h; one wavefront, one launch): the chain as the kernels run it (which = 1: the loop runs
only while the step it fetches exists, so its addresses walk by constants, and the last turns of the operand ring are peeled) against the
copy of the chain as it was before (which = 0, in the probe's unit only: every fetch clamps its stage).  Every stored value is the same
fma and the same MFMA on the same operands, so the bar is equality of the bit patterns of the whole slot array after the chain.

Horizons 1, 2 (shorter than the ring of three: the earlier form runs its remainder only; the shipped one its peeled steps, the fill of
the ring clamped), 3 (exactly one turn of the ring), 4, 5 (a turn and one or two more steps: in the shipped form still all peeled, the
fetches for steps 3 and 4 among them) and 20 (earlier form: six turns and a remainder of two; shipped: five turns of the loop, then five
peeled steps), and 6, 7, 8 for the shipped form's sake (one turn of its loop, then three, four and five peeled steps); four instances
in the wavefront but at N = 20: 21 lanes per instance, three instances, the fourth block shadows block 0 and must store nowhere.  Both
directions.  The slots are what a factor sweep leaves of the well-conditioned stages of tests/test_gpu_mx_factor_step.py
(the factor probe's reference form makes them: K, d_k and P_k belong to the A, B of the slot), with the backward chain's
c_k = q_k + g_x - K_k g_u of a fresh right-hand side at the place the stage lanes write it.

The reference copy itself is held to a numpy restatement of the recursion at 1e-9 of the largest entry, the bound the factor-step test
argues for its own: IEEE double, at most 20 steps of a contraction-sized map (|Acl| ~ 1), no reciprocal on the way."""
import numpy as np
import pytest
import torch

from test_gpu_mx_factor_step import AH, COL, KK, ROW, SLOT, WAVE, layout, stage_data

pytestmark = pytest.mark.gpu

HORIZONS = (1, 2, 3, 4, 5, 6, 7, 8, 20)
SENTINEL = 7.0
OUT = {True: ROW + 1, False: COL + 1}       # first word the chain writes: Dx_k[r] at 49 + 2 r, p_k[r] at 33 + 4 r
STRIDE = {True: 2, False: 4}


def bits(t):
    return t.contiguous().view(torch.int64)


def factored(N, seed):
    """[64, 66] float64 (numpy): the slots after a factor sweep, the sentinel where the chain is going to write."""
    from mpc4rl_amd import _lib
    dev = torch.device("cuda:0")
    xin = torch.as_tensor(stage_data(N, seed), dtype=torch.float64, device=dev).contiguous()
    out, ok = torch.empty_like(xin), torch.empty(4, dtype=torch.float64, device=dev)
    assert _lib.call("mpcrl_debug_mx_factor", xin, N, _lib.PROBE_MX_WANT_P, 0, out, ok, device=dev) == 0
    torch.cuda.synchronize()
    lpi, ipw = layout(N)
    assert ok.tolist() == [1.0] * ipw + [-1.0] * (4 - ipw)
    return out.cpu().numpy()


def chain_input(N, forward, seed):
    lpi, ipw = layout(N)
    s = factored(N, seed)
    rng = np.random.default_rng(seed + 1)
    if not forward:         # the corrector's right-hand side, as the stage lanes leave it: c_k = q_k + g_x - K g_u, c_N = g_x
        for lane in range(ipw * lpi):
            gx, gu = rng.normal(size=4), rng.normal()
            q, K = s[lane, ROW:ROW + 8:2].copy(), s[lane, KK:KK + 4]
            s[lane, COL + 3:COL + 16:4] = gx if lane % lpi == N else q + gx - K * gu
    o = OUT[forward]
    s[:, o:o + 4 * STRIDE[forward]:STRIDE[forward]] = SENTINEL
    return s


def written(N, forward):
    """[64, 66] bool: the words the chain stores to."""
    lpi, ipw = layout(N)
    w = np.zeros((WAVE, SLOT), bool)
    o = OUT[forward]
    for lane in range(ipw * lpi):
        if not forward or lane % lpi != 0:
            w[lane, o:o + 4 * STRIDE[forward]:STRIDE[forward]] = True
    return w


def run(slots, N, forward, which):
    from mpc4rl_amd import _lib
    dev = torch.device("cuda:0")
    xin = torch.as_tensor(slots, dtype=torch.float64, device=dev).contiguous()
    out = torch.full_like(xin, 12345.0)
    assert _lib.call("mpcrl_debug_mx_chain", xin, N, 1 if forward else 0, which, out, device=dev) == 0
    return out


def recursion(slots, N, blk, forward):
    """{stage: vector} of one instance in numpy."""
    lpi, _ = layout(N)
    sl = slots[blk * lpi:(blk + 1) * lpi]

    def acl(k):
        return sl[k, AH:AH + 32:2].reshape(4, 4) - np.outer(sl[k, COL:COL + 16:4], sl[k, KK:KK + 4])

    res = {}
    if forward:
        v = np.zeros(4)
        for k in range(N):
            v = acl(k) @ v + sl[k, COL + 3:COL + 16:4]
            res[k + 1] = v
    else:
        v = sl[N, COL + 3:COL + 16:4].copy()
        res[N] = v
        for k in range(N - 1, -1, -1):
            v = acl(k).T @ v + sl[k, COL + 3:COL + 16:4]
            res[k] = v
    return res


@pytest.mark.parametrize("forward", (True, False), ids=("forward", "backward"))
@pytest.mark.parametrize("N", HORIZONS)
def test_chain_equals_the_chain_before(N, forward):
    lpi, ipw = layout(N)
    assert (lpi, ipw) == {1: (2, 4), 2: (3, 4), 3: (4, 4), 4: (5, 4), 5: (6, 4), 6: (7, 4), 7: (8, 4), 8: (9, 4), 20: (21, 3)}[N]
    slots = chain_input(N, forward, 400 + N)
    o0, o1 = run(slots, N, forward, 0), run(slots, N, forward, 1)
    torch.cuda.synchronize()
    tag = (N, forward)
    w = written(N, forward)
    wt = torch.as_tensor(w, device="cuda:0")
    assert torch.equal(bits(o1)[wt], bits(o0)[wt]), tag             # what the chain writes: the same bits
    assert torch.equal(bits(o1), bits(o0)), tag                      # and everything else
    a0, a1 = o0.cpu().numpy(), o1.cpu().numpy()
    for a in (a0, a1):                                               # every word the chain does not write is as it came in:
        assert np.array_equal(a[~w], slots[~w]), tag                 # the sentinels of stage 0 (forward), lanes without a stage
        assert not np.any(a[w] == SENTINEL), tag                     # and it did write where it should
    o, st = OUT[forward], STRIDE[forward]
    for blk in range(ipw):
        ref = recursion(slots, N, blk, forward)
        scale = max(1.0, max(np.max(np.abs(v)) for v in ref.values()))
        for k, want in ref.items():
            got = a0[blk * lpi + k, o:o + 4 * st:st]
            err = np.max(np.abs(got - want)) / scale
            print(f"[chain step] N {N} {'forward' if forward else 'backward'} block {blk} stage {k}: error {err:.3e} of {scale:.3e}")
            assert err < 1e-9, (tag, blk, k, err)


def test_chain_probe_refuses_what_it_cannot_run():
    from mpc4rl_amd import _lib
    buf = torch.zeros(WAVE, SLOT, dtype=torch.float64, device="cuda:0")
    for N, forward, which in ((0, 1, 1), (64, 1, 1), (20, 2, 1), (20, -1, 1), (20, 1, 2), (20, 0, -1)):
        with pytest.raises(RuntimeError):
            _lib.call("mpcrl_debug_mx_chain", buf, N, forward, which, buf, device="cuda:0")
    with pytest.raises(RuntimeError):
        _lib.call("mpcrl_debug_mx_chain", None, 20, 1, 1, buf, device="cuda:0")
    with pytest.raises(RuntimeError):
        _lib.call("mpcrl_debug_mx_chain", buf, 20, 1, 1, None, device="cuda:0")
