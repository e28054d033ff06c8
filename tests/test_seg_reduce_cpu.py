"""The segmented reduction tree of the small-model kernels (csrc/small_kernel.hpp, seg_reduce) on the host: what "the same tree" means.

tests/seg_reduce_cases.py restates the tree with whole-array moves (`emulate`); here it is held, for every lpi in 2 .. 64, to a
lane-by-lane simulation of __shfl_down and __shfl written with plain loops, and the two ways the kernels' helpers move a value
differently from __shfl_down are shown to change no bit of any instance slot that lies inside the wave:
  * for lpi <= 32 the level at distance 32 is not run (no lane has k + 32 < lpi);
  * distances 2 and 1 are two and one one-lane shifts.  After two shifts lane 62 holds lane 63's value where __shfl_down(v, 2) hands
    it its own — in a slot inside the wave that lane has k + 2 >= lpi and takes nothing in.
tests/test_gpu_seg_reduce.py holds the device to `emulate`."""
import math

import numpy as np
import pytest

import seg_reduce_cases as S


def simulate(v, lpi, is_max):
    """The kernels' tree lane by lane: __shfl_down(v, s) = value of lane + s, the lane's own past lane 63; __shfl(v, base) at the end."""
    v = [float(t) for t in v]
    for s in (32, 16, 8, 4, 2, 1):
        fetched = [v[lane + s] if lane + s < S.WAVE else v[lane] for lane in range(S.WAVE)]
        for lane in range(S.WAVE):
            k = lane % lpi
            if k + s < lpi:
                a, b = v[lane], fetched[lane]
                if is_max:      # fmax: a NaN operand is dropped
                    v[lane] = b if math.isnan(a) else (a if math.isnan(b) else max(a, b))
                else:
                    v[lane] = a + b
    return np.array([v[(lane // lpi) * lpi] for lane in range(S.WAVE)])


@pytest.mark.parametrize("shape", S.SHAPES)
def test_emulation_is_the_lane_by_lane_tree(shape):
    n_max, n_sum = shape
    for lpi in S.LPI:
        x = S.inputs(lpi, n_max, n_sum)
        for i in range(n_max + n_sum):
            got, ref = S.emulate(x[i], lpi, i < n_max), simulate(x[i], lpi, i < n_max)
            assert S.same_bits(got, ref), (lpi, i)      # all 64 lanes, the slot the wave cuts off included


@pytest.mark.parametrize("shape", S.SHAPES)
def test_production_moves_change_no_bit_inside_the_wave(shape):
    n_max, n_sum = shape
    differs_outside = 0
    for lpi in S.LPI:
        _, _, complete = S.lanes(lpi)
        x = S.inputs(lpi, n_max, n_sum)
        for i in range(n_max + n_sum):
            ref, got = S.emulate(x[i], lpi, i < n_max), S.emulate(x[i], lpi, i < n_max, moves="production")
            assert S.same_bits(got[complete], ref[complete]), (lpi, i)
            differs_outside += not S.same_bits(got[~complete], ref[~complete])
    assert differs_outside > 0      # the cut-off slot is where the two shifts show: the restriction above is not vacuous


def test_the_tree_is_not_a_left_to_right_sum():
    """The inputs make the order of the additions visible: the tree's sum differs from the sequential one in some slot at most sizes —
    a reduction that associated differently would not pass as 'the same tree'."""
    seen = 0
    for lpi in S.LPI:
        x = S.inputs(lpi, 0, 1)[0]
        k, base, complete = S.lanes(lpi)
        tree = S.emulate(x, lpi, False)
        for b in np.unique(base[complete]):
            seq = 0.0
            for t in x[b:b + lpi]:
                seq += t
            seen += tree[b] != seq
    assert seen > len(S.LPI) // 2


def test_inputs_cover_the_special_values():
    for lpi in (2, 21, 33, 64):
        x = S.inputs(lpi, 2, 2)
        assert np.isnan(x[:2]).any() and np.isposinf(x[:2]).any() and np.isneginf(x[:2]).any()
        assert np.isnan(x[0, :lpi]).all() and np.isfinite(x[2:]).all()
        assert (x[2:] > 0).any() and (x[2:] < 0).any() and np.abs(x[2:]).max() / np.abs(x[2:]).min() > 1e12
        assert np.isnan(S.emulate(x[0], lpi, True)[0])      # a slot of NaNs only reduces to NaN
