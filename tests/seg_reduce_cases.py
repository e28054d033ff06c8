"""What tests/test_seg_reduce_cpu.py and tests/test_gpu_seg_reduce.py share (no test of its own): the segmented reduction tree of
csrc/small_kernel.hpp (seg_reduce) restated on the host, and the inputs of the probe.

The tree: a wavefront of 64 lanes holds instances of lpi lanes each (lane = slot * lpi + k).  Levels s = 32, 16, 8, 4, 2, 1: every lane
fetches the value of lane + s (its own where lane + s > 63) and takes it in when k + s < lpi, as own + partner or fmax(own, partner);
then every lane reads lane slot * lpi.  IEEE double + and fmax are exact on the host, so "the same tree" is the same bits.

`emulate` is written with whole-array numpy moves; `simulate` in tests/test_seg_reduce_cpu.py is the lane-by-lane restatement of
__shfl_down it is held to.  moves = "production" restates the two ways the kernels' helpers move a value differently from __shfl_down
(no level at distance 32 for lpi <= 32; distances 2 and 1 as two and one one-lane shifts, where lane 63 keeps its own value)."""
import numpy as np

WAVE = 64
LPI = tuple(range(2, 65))
SHAPES = ((1, 1), (2, 2), (4, 1))      # (max-values, sum-values) of the interior point's passes and of the SQP round


def lanes(lpi):
    """(k, base, complete) per lane: stage index, first lane of the lane's slot, and whether the slot lies inside the wave."""
    lane = np.arange(WAVE)
    slot = lane // lpi
    base = slot * lpi
    return lane - base, base, base + lpi <= WAVE


def shift_down(v, s):
    """What __shfl_down(v, s) hands every lane: the value of lane + s, its own past the end of the wave."""
    o = v.copy()
    o[: WAVE - s] = v[s:]
    return o


def emulate(v, lpi, is_max, moves="shfl"):
    """One value [64] through the tree; returns what every lane holds after the broadcast."""
    k, base, _ = lanes(lpi)
    v = np.array(v, dtype=np.float64)
    for s in (32, 16, 8, 4, 2, 1):
        if moves == "production" and s == 32 and lpi <= 32:
            continue
        if moves == "production" and s <= 2:
            o = v
            for _ in range(s):
                o = shift_down(o, 1)
        else:
            o = shift_down(v, s)
        take = k + s < lpi
        with np.errstate(invalid="ignore"):
            v = np.where(take, np.fmax(v, o) if is_max else v + o, v)
    return v[base]


def same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN (a maximum over NaNs only: its payload is the hardware's business)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | both_nan))


def inputs(lpi, n_max, n_sum):
    """[n_max + n_sum, 64] doubles, max-values first: mixed sign, magnitudes over 24 decades (sums that cancel and absorb, so that the
    order of the additions shows in the last bits); the max-values also hold +-inf and NaN — one slot of the first max-value is all NaN."""
    rng = np.random.default_rng(1000 * lpi + 10 * n_max + n_sum)
    x = rng.standard_normal((n_max + n_sum, WAVE)) * 10.0 ** rng.integers(-12, 13, (n_max + n_sum, WAVE))
    for i in range(n_max):
        idx = rng.permutation(WAVE)
        x[i, idx[:6]] = np.nan
        x[i, idx[6:9]] = np.inf
        x[i, idx[9:12]] = -np.inf
    if n_max:
        x[0, :lpi] = np.nan
    return x
