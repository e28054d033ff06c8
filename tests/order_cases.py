"""What tests/test_order_cpu.py and tests/test_gpu_order.py share (no test of its own): a numpy restatement of the packing-order kernel
(csrc/order_kernel.hpp), written from the rule the kernel documents and not from its code, the batches it is compared on, the explicit
permutations the solve kernels are run under, and the per-instance inputs of those runs.

The rule.  A from-scratch call (refresh) looks at every coordinate of x0 [B, nx]: minimum and maximum over the entries that are not NaN
(1e300 / -1e300 where there are none), and keeps {spread, minimum, coordinate} of the first coordinate whose spread max - min is
strictly the largest, starting from a spread of -1.  Every call then buckets the batch along the remembered coordinate (clamped to
[0, nx)): with scale = 1024 / spread (0 where the spread is not positive) the key of a value v is trunc(min(max((v - minimum) * scale,
0), 1023)), and 1023 for a NaN.  A bucket of more than 64 entries makes the order the identity; otherwise the order is by key, and by
instance index inside a key — a stable argsort.  The library is built without fast-math and (v - minimum) * scale cannot contract into
a fused multiply-add, so float64 numpy computes the kernel's keys bit for bit: the device comparison is array_equal, not a tolerance."""
import functools

import numpy as np

BUCKETS, BUCKET_MAX, ORDER_MAX = 1024, 64, 8192
NEVER_REFRESHED = (-1.0, 0.0, 0.0)      # the state of a handle whose order was never built from scratch


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def refresh_state(x0):
    """(spread, minimum, coordinate) a from-scratch call remembers."""
    x0 = np.asarray(x0, float)
    best = NEVER_REFRESHED
    for d in range(x0.shape[1]):
        col = x0[:, d]
        col = col[~np.isnan(col)]
        lo, hi = (float(col.min()), float(col.max())) if len(col) else (1e300, -1e300)
        if hi - lo > best[0]:
            best = (hi - lo, lo, float(d))
    return best


def keys(x0, state):
    x0 = np.asarray(x0, float)
    spread, lo, d = state
    dim = min(max(int(d), 0), x0.shape[1] - 1)
    scale = float(BUCKETS) / spread if spread > 0.0 else 0.0
    v = x0[:, dim]
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.fmin(np.fmax((v - lo) * scale, 0.0), float(BUCKETS - 1))
    return np.where(np.isnan(v), BUCKETS - 1, np.trunc(q)).astype(np.int64)


def largest_bucket(x0, state):
    return int(np.bincount(keys(x0, state), minlength=BUCKETS).max())


def order(x0, state):
    """The permutation a call on this state writes: slot i of a launch works on instance order[i]."""
    k = keys(x0, state)
    if np.bincount(k, minlength=BUCKETS).max() > BUCKET_MAX:
        return np.arange(len(k), dtype=np.int32)
    return np.argsort(k, kind="stable").astype(np.int32)


def is_permutation(p, B):
    p = np.asarray(p)
    return p.shape == (B,) and np.array_equal(np.sort(p), np.arange(B))


def is_identity(p):
    return np.array_equal(np.asarray(p), np.arange(len(p)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the batches (computed once, never written to)
# ---------------------------------------------------------------------------------------------------------------------------------
UNIFORM_B = (129, 1000, 1023, 1024, 1025, 8191, 8192)      # either side of the kernel's 1024 threads and of its 8192 entries
EQUAL_B = (1, 2, 63, 64, 65)                                # one bucket: 64 goes through the sort, 65 through the crowded exit
CROWD_B, CROWD_K = 200, (64, 65)
TIE_B = NAN_B = CHEAP_B = 300
NAN_COUNTS = (3, 63, 64)
NX2_B = 130


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def uniform(B, seed=5):
    """The roll-out batch of the benchmark: the pole angle (coordinate 2) spread around pi, a little cart position."""
    rng = np.random.default_rng(seed + B)
    x0 = np.zeros((B, 4))
    x0[:, 2] = rng.uniform(0.9 * np.pi, 1.1 * np.pi, B)
    x0[:, 0] = rng.uniform(-0.01, 0.01, B)
    return _frozen(x0)


@functools.lru_cache(maxsize=None)
def equal_rows(B):
    return _frozen(np.tile(np.array([0.1, -0.2, 3.0, 0.4]), (B, 1)))


@functools.lru_cache(maxsize=None)
def crowding(k):
    """Coordinate 1 descending from 1 to -1 (neighbouring rows five buckets apart), the first k rows on the maximum: bucket 1023 holds
    exactly those k."""
    x0 = np.zeros((CROWD_B, 4))
    x0[:, 1] = np.linspace(1.0, -1.0, CROWD_B)
    x0[:k, 1] = 1.0
    return _frozen(x0)


@functools.lru_cache(maxsize=None)
def tie():
    """Coordinates 1 and 3 hold the same values in another order, and spread wider than 0 and 2: the first of them wins."""
    rng = np.random.default_rng(17)
    x0 = rng.uniform(-1.0, 1.0, (TIE_B, 4)) * np.array([0.5, 2.0, 0.3, 1.0])
    x0[:, 3] = rng.permutation(x0[:, 1])
    return _frozen(x0)


@functools.lru_cache(maxsize=None)
def nan_base():
    rng = np.random.default_rng(23)
    return _frozen(rng.uniform(-1.0, 1.0, (NAN_B, 4)) * np.array([0.5, 0.3, 2.0, 0.5]))


@functools.lru_cache(maxsize=None)
def nan_rows(n):
    """The rows that hold a NaN: scattered over the batch, never the rows of the minimum and the maximum of coordinate 2."""
    base = nan_base()
    keep = {int(base[:, 2].argmin()), int(base[:, 2].argmax())}
    rows = [int(i) for i in np.random.default_rng(29).permutation(NAN_B) if int(i) not in keep][:n]
    return np.sort(np.array(rows))


@functools.lru_cache(maxsize=None)
def nan_keys(n):
    """n NaNs in the chosen coordinate (2)."""
    x0 = nan_base().copy()
    x0[nan_rows(n), 2] = np.nan
    return _frozen(x0)


@functools.lru_cache(maxsize=None)
def nan_elsewhere():
    """One NaN in a coordinate the order is not built along."""
    x0 = nan_base().copy()
    x0[nan_rows(1)[0], 0] = np.nan
    return _frozen(x0)


@functools.lru_cache(maxsize=None)
def cheap_a():
    """Widest along coordinate 2, which it fills between -1 and 1."""
    rng = np.random.default_rng(31)
    return _frozen(rng.uniform(-1.0, 1.0, (CHEAP_B, 4)) * np.array([0.5, 0.3, 1.0, 0.5]))


@functools.lru_cache(maxsize=None)
def cheap_b():
    """Half as wide again as A along coordinate 2 (a sixth of the batch clips into either end bucket of A's range), and widest along
    coordinate 0, which a call on A's state must not look at."""
    rng = np.random.default_rng(37)
    return _frozen(rng.uniform(-1.0, 1.0, (CHEAP_B, 4)) * np.array([3.0, 0.3, 1.5, 0.5]))


@functools.lru_cache(maxsize=None)
def cheap_c():
    """B above A's range along coordinate 2: one bucket."""
    x0 = cheap_b().copy()
    x0[:, 2] += 10.0
    return _frozen(x0)


@functools.lru_cache(maxsize=None)
def nx2():
    """The linear system's state."""
    rng = np.random.default_rng(43)
    return _frozen(np.column_stack([rng.uniform(0.15, 0.85, NX2_B), rng.uniform(-0.2, 0.5, NX2_B)]))


def refresh_cases():
    """{name: x0} of every batch ordered from scratch on a fresh handle."""
    cases = {f"uniform {B}": uniform(B) for B in UNIFORM_B}
    cases.update({f"equal rows {B}": equal_rows(B) for B in EQUAL_B})
    cases.update({f"crowding {k}": crowding(k) for k in CROWD_K})
    cases["tie"] = tie()
    cases.update({f"nan keys {n}": nan_keys(n) for n in NAN_COUNTS})
    cases["nan elsewhere"] = nan_elsewhere()
    cases["cheap A"], cases["cheap B"] = cheap_a(), cheap_b()
    cases["nx 2"] = nx2()
    return cases


REFRESH_NAMES = tuple(refresh_cases())


# ---------------------------------------------------------------------------------------------------------------------------------
# explicit orders and the per-instance inputs of the solves run under them
# ---------------------------------------------------------------------------------------------------------------------------------
def explicit_orders(B):
    """(reversal, rotation by one — every wavefront boundary moves —, a fixed-seed shuffle) of 0 .. B-1."""
    i = np.arange(B, dtype=np.int32)
    return i[::-1].copy(), np.roll(i, -1), np.random.default_rng(53).permutation(B).astype(np.int32)


ORDER_CP_N = (3, 16, 20, 21, 32, 62)      # 4, 3, 3, 2, 1, 1 instances per wavefront; the parked instance in LDS up to 20, in HBM from 21
ORDER_LIN_N = (7, 8, 24, 48)              # small_solve_kernel, lq_solve_kernel<3, 8>, <3, 16>, <4, 16>
ORDER_GENERIC_N, ORDER_SPL1_N = 20, 24    # the generic bound rows (cartpole), one stage per lane (linear) at these horizons as well
ORDER_STATUS_N, ORDER_NAN_N = 16, 16
MAX_ITER = 2                              # test_max_iter_two_is_status_two of tests/test_small_modes_cpu.py
N_DYNAMICS = {"cartpole": 3, "linear": 8}      # M, m, l; A, B, b: the leading entries of p


def theta_rows(ocp, model, B):
    """Per-instance parameters: p0 (1 + 0.05 xi_i) on the dynamics entries, xi ~ U(-1, 1)."""
    n = N_DYNAMICS[model]
    th = np.tile(np.asarray(ocp.p0, float), (B, 1))
    th[:, :n] *= 1.0 + 0.05 * np.random.default_rng(59).uniform(-1.0, 1.0, (B, n))
    return th


def cold_mask(B):
    """Every third instance."""
    return np.arange(B) % 3 == 0


# the learners' sequences
SEQ_B, SEQ_STEPS = 130, 34


def sequence_inputs(model, t):
    """x0 [SEQ_B, nx] of step t = 0 .. 33 of a slowly moving batch (the small-modes inputs tiled, every copy a little off, drifting along
    their `step` at a fifth of its size per call) and the cold mask of that step: another tenth of the instances every time."""
    import small_mode_cases as C
    x0, _, step = C.inputs(model)
    reps = -(-SEQ_B // len(x0))
    rng = np.random.default_rng(61)
    base = np.tile(x0, (reps, 1))[:SEQ_B] + rng.normal(0.0, 0.01, (SEQ_B, x0.shape[1]))
    drift = np.tile(step, (reps, 1))[:SEQ_B]
    return base + 0.2 * t * drift, np.arange(SEQ_B) % 10 == t % 10


ARGSORT_B = 8200
