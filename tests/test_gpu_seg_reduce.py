"""The segmented reductions of the small-model kernels on the device, through the probe export mpcrl_debug_seg_reduce (one wavefront,
one launch): the helpers as the kernels instantiate them against a copy of the tree with every move a __shfl_down / __shfl, and both
against the host restatement of tests/seg_reduce_cases.py (held to a lane-by-lane simulation in tests/test_seg_reduce_cpu.py).

Every lpi in 2 .. 64, every instance slot that lies inside the wave (slot * lpi + lpi <= 64), the shapes (1, 1), (2, 2), (4, 1) of the
interior point's and the SQP round's passes; random doubles of mixed sign over 24 decades, the max-values with +-inf and NaN.  IEEE
double + and fmax are exact, so the bar is equality: torch.equal on the bit patterns between the two device paths (a NaN has to be
the same NaN), and bit for bit against the host with any NaN equal to any NaN.

The lanes of a slot the wave cuts off are not compared: there the helpers' two one-lane shifts hand lane 62 another value than
__shfl_down(v, 2) does (small_kernel.hpp, seg_partner); such lanes shadow an instance and never store."""
import numpy as np
import pytest
import torch

import seg_reduce_cases as S

pytestmark = pytest.mark.gpu


def probe(lib, x, lpi, n_max, n_sum, which):
    from mpc4rl_amd.batch import _ptr
    xin = torch.as_tensor(x, dtype=torch.float64, device="cuda:0").contiguous()
    out = torch.full_like(xin, 12345.0)
    assert tuple(xin.shape) == (n_max + n_sum, S.WAVE)
    with torch.cuda.device(0):
        rc = lib.mpcrl_debug_seg_reduce(_ptr(xin), lpi, n_max, n_sum, which, _ptr(out), None)
    assert rc == 0
    return out


@pytest.mark.parametrize("shape", S.SHAPES)
def test_helpers_equal_the_shfl_tree_and_the_host(shape):
    from mpc4rl_amd import _lib
    lib = _lib.load()
    n_max, n_sum = shape
    outs = []
    for lpi in S.LPI:
        x = S.inputs(lpi, n_max, n_sum)
        outs.append((lpi, x, [probe(lib, x, lpi, n_max, n_sum, which) for which in (0, 1, 2)]))
    torch.cuda.synchronize()
    for lpi, x, (ref, cart, lin) in outs:
        _, _, complete = S.lanes(lpi)
        keep = torch.as_tensor(complete, device=ref.device)
        for name, got in (("cartpole helpers", cart), ("linear-system helpers", lin)):
            assert torch.equal(got[:, keep].view(torch.int64), ref[:, keep].view(torch.int64)), (name, lpi)
        host = np.stack([S.emulate(x[i], lpi, i < n_max) for i in range(n_max + n_sum)])
        for name, got in (("shfl tree", ref), ("cartpole helpers", cart)):
            assert S.same_bits(got.cpu().numpy()[:, complete], host[:, complete]), (name, lpi)
        assert S.same_bits(ref.cpu().numpy(), host), ("shfl tree, all 64 lanes", lpi)


def test_probe_refuses_what_it_does_not_reduce():
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import _ptr
    lib = _lib.load()
    buf = torch.zeros(8, S.WAVE, dtype=torch.float64, device="cuda:0")
    for lpi, n_max, n_sum, which in ((0, 1, 1, 1), (65, 1, 1, 1), (21, 3, 3, 1), (21, 1, 1, 3), (21, 1, 1, -1)):
        assert lib.mpcrl_debug_seg_reduce(_ptr(buf), lpi, n_max, n_sum, which, _ptr(buf), None) != 0
    assert lib.mpcrl_debug_seg_reduce(None, 21, 1, 1, 1, _ptr(buf), None) != 0
