"""``_lib.call`` on the device (mpc4rl_amd/_lib.py): the same launch as a direct call of the library, bit for bit, with strided views,
on another stream, captured into a graph, with a NULL, with a refusal and with a positive return.  All on mpcrl_weighted_grad_sum at
rows = 3, n = 2: the smallest shape with more than one row and column, on the kernel's row-parallel path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, N = 3, 2


@pytest.fixture(scope="module")
def case():
    """grad: a [3, 2] view of a [3, 5] table (ld = 5), weight [3], and what the direct call returns for them (with and without weight)."""
    from mpc4rl_amd import _lib
    from mpc4rl_amd._lib import _ptr
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(5)
    table = torch.randn(ROWS, 5, dtype=torch.float64, device="cuda", generator=gen)
    weight = torch.randn(ROWS, dtype=torch.float64, device="cuda", generator=gen)
    stream = torch.cuda.current_stream().cuda_stream

    def direct(grad, ld, w):
        out = torch.full((N + 2,), float("nan"), dtype=torch.float64, device="cuda")
        assert lib.mpcrl_weighted_grad_sum(_ptr(grad), ld, _ptr(w), ROWS, N, _ptr(out), stream) == 0
        torch.cuda.synchronize()
        return out

    dense = table[:, 1:1 + N].contiguous()
    ref = {"dense": direct(dense, N, weight), "view": direct(table[:, 1:1 + N], 5, weight), "unweighted": direct(dense, N, None)}
    assert torch.equal(ref["dense"], ref["view"]) and float(ref["dense"][N + 1]) == ROWS
    assert float(ref["unweighted"][N]) == ROWS and not torch.equal(ref["dense"], ref["unweighted"])
    return dict(table=table, dense=dense, weight=weight, ref=ref)


def through_call(grad, ld, w, out=None):
    from mpc4rl_amd import _lib
    out = torch.full((N + 2,), float("nan"), dtype=torch.float64, device="cuda") if out is None else out
    assert _lib.call("mpcrl_weighted_grad_sum", grad, ld, w, ROWS, N, out, device=out.device) == 0
    return out


def test_call_equals_the_direct_call(case):
    assert torch.equal(through_call(case["dense"], N, case["weight"]), case["ref"]["dense"])


def test_strided_view_goes_through_as_it_is(case):
    view = case["table"][:, 1:1 + N]
    assert not view.is_contiguous()
    assert torch.equal(through_call(view, 5, case["weight"]), case["ref"]["view"])


def test_call_under_a_non_default_stream(case):
    """The same bits with a side stream current.  (That the launch IS on the current stream is what the capture test below pins: a
    launch on any other stream would not be captured.)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = through_call(case["dense"], N, case["weight"])      # (its NaN fill is queued on the side stream, in front of the launch)
    side.synchronize()
    assert torch.equal(out, case["ref"]["dense"])


def test_call_is_captured_into_a_graph(case):
    out = torch.zeros(N + 2, dtype=torch.float64, device="cuda")
    grad = case["dense"].clone()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):       # one node chain: no parallel branches
        through_call(grad, N, case["weight"], out)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))       # captured, not run: the launch went to the current (capturing) stream
    for scale in (1.0, 2.0):                              # replayed twice, on inputs changed in place
        grad.copy_(case["dense"] * scale)
        graph.replay()
        torch.cuda.synchronize()
        want = case["ref"]["dense"].clone()
        want[:N] *= scale                                  # (a scaling by 2 is exact)
        assert torch.equal(out, want)


def test_none_is_null(case):
    assert torch.equal(through_call(case["dense"], N, None), case["ref"]["unweighted"])


def test_negative_return_raises(case):
    from mpc4rl_amd import _lib
    out = torch.full((N + 2,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="mpcrl_weighted_grad_sum failed with -1"):
        _lib.call("mpcrl_weighted_grad_sum", case["dense"], N, None, -1, N, out, device=out.device)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))       # refused on the host: nothing was launched


def test_positive_return_comes_back():
    from mpc4rl_amd import MPCBatch, cartpole_ocp
    mpc = MPCBatch(cartpole_ocp(), 4)
    perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32, device="cuda")
    assert mpc.get_order()[0] is None
    mpc.set_order(perm)
    got, _ = mpc.get_order()
    torch.cuda.synchronize()
    assert got is not None and torch.equal(got, perm)
