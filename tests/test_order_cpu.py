"""The conditions tests/test_gpu_order.py relies on, held on the CPU alone (no GPU): the numpy restatement of the packing-order kernel
(tests/order_cases.py) returns a valid permutation on every batch, every batch is crowded or not and ordered or not as its case says, so
that no device comparison can pass vacuously; the explicit orders are permutations other than the identity; and on the C++ CPU port the
per-instance parameters, the iteration cap and the NaN row of the solves run under those orders have an effect above the comparison bar."""
import numpy as np
import pytest

import order_cases as O
import small_mode_cases as C


def facts(x0, state=None):
    state = O.refresh_state(x0) if state is None else state
    p = O.order(x0, state)
    assert p.dtype == np.int32 and O.is_permutation(p, len(x0))
    k = O.keys(x0, state)
    if not O.is_identity(p):      # ordered by key, by index inside a key
        assert np.all(np.diff(k[p]) >= 0) and np.all(np.diff(p)[np.diff(k[p]) == 0] > 0)
    return state, p, O.largest_bucket(x0, state)


@pytest.mark.parametrize("B", O.UNIFORM_B)
def test_uniform_batches(B):
    x0 = O.uniform(B)
    state, p, crowd = facts(x0)
    assert x0.shape == (B, 4) and state[2] == 2.0 and crowd <= O.BUCKET_MAX and not O.is_identity(p)
    assert np.all(np.diff(O.keys(x0, state)[p]) >= 0)
    # buckets are coarser than values: the order is not the argsort of the coordinate, the index rule inside a bucket is in play
    assert not np.array_equal(p, np.argsort(x0[:, 2], kind="stable"))


@pytest.mark.parametrize("B", O.EQUAL_B)
def test_equal_rows(B):
    state, p, crowd = facts(O.equal_rows(B))
    assert state == (0.0, 0.1, 0.0) and crowd == B and O.is_identity(p)      # spread 0 > -1: coordinate 0 wins, scale 0, one bucket
    assert (crowd > O.BUCKET_MAX) == (B == 65)


def test_crowding_threshold():
    """More than 64 in a bucket: 64 is sorted, 65 is the identity."""
    state, p, crowd = facts(O.crowding(64))
    assert state == (2.0, -1.0, 1.0) and crowd == 64 and not O.is_identity(p)
    assert list(p[-64:]) == list(range(64)) and p[0] == O.CROWD_B - 1
    state, p, crowd = facts(O.crowding(65))
    assert state == (2.0, -1.0, 1.0) and crowd == 65 and O.is_identity(p)


def test_tie_goes_to_the_first_coordinate():
    x0 = O.tie()
    spread = x0.max(0) - x0.min(0)
    assert spread[1] == spread[3] and spread[1] > max(spread[0], spread[2])
    assert not np.array_equal(x0[:, 1], x0[:, 3])
    state, p, _ = facts(x0)
    assert state[2] == 1.0 and not O.is_identity(p)
    assert not np.array_equal(p, O.order(x0, (state[0], state[1], 3.0)))      # the other coordinate would give another order


def test_nan_keys():
    base_state, base_p, _ = facts(O.nan_base())
    assert base_state[2] == 2.0
    top = int(O.nan_base()[:, 2].argmax())
    for n in O.NAN_COUNTS:
        x0, rows = O.nan_keys(n), O.nan_rows(n)
        assert len(rows) == n and int(np.isnan(x0).sum()) == n and top not in rows
        state, p, crowd = facts(x0)
        assert state == base_state      # NaN entries take no part in the range
        k = O.keys(x0, state)
        assert np.all(k[rows] == O.BUCKETS - 1) and k[top] == O.BUCKETS - 1 and crowd == n + 1
        if n == 3:      # sorted last, by index, together with the maximum
            assert list(p[-4:]) == sorted(list(rows) + [top]) and not O.is_identity(p)
        if n == 63:      # 64 in the bucket: not more than 64
            assert not O.is_identity(p) and list(p[-64:]) == sorted(list(rows) + [top])
        if n == 64:
            assert O.is_identity(p)
    state, p, _ = facts(O.nan_elsewhere())
    assert int(np.isnan(O.nan_elsewhere()[:, 0]).sum()) == 1 and state == base_state and np.array_equal(p, base_p)


def test_cheap_path_batches():
    a, b, c = O.cheap_a(), O.cheap_b(), O.cheap_c()
    sa, pa, _ = facts(a)
    sb, pb, _ = facts(b)
    assert sa[2] == 2.0 and sb[2] == 0.0 and not O.is_identity(pa) and not O.is_identity(pb)
    # B on A's state: along coordinate 2, clipped into both end buckets, not crowded; another order than B's own
    _, p, crowd = facts(b, sa)
    k = np.bincount(O.keys(b, sa), minlength=O.BUCKETS)
    print(f"[order cpu] B on A's state: end buckets {k[0]}, {k[-1]}, largest {crowd}")
    assert 10 < k[0] <= O.BUCKET_MAX and 10 < k[-1] <= O.BUCKET_MAX and crowd == max(k[0], k[-1])
    assert not O.is_identity(p) and not np.array_equal(p, pb)
    assert b[:, 2].min() < a[:, 2].min() and b[:, 2].max() > a[:, 2].max()
    # C on A's state: one bucket; on B's state: B's order (they differ along coordinate 2 only)
    _, p, crowd = facts(c, sa)
    assert crowd == O.CHEAP_B and O.is_identity(p)
    assert np.array_equal(facts(c, sb)[1], pb)
    # a state nobody refreshed
    _, p, crowd = facts(a, O.NEVER_REFRESHED)
    assert crowd == O.CHEAP_B and O.is_identity(p)


def test_nx2_batch():
    x0 = O.nx2()
    state, p, crowd = facts(x0)
    assert x0.shape == (O.NX2_B, 2) and crowd <= O.BUCKET_MAX and not O.is_identity(p)
    # a remembered coordinate beyond nx is clamped
    assert np.array_equal(O.order(x0, (state[0], state[1], 3.0)), O.order(x0, (state[0], state[1], 1.0)))


def test_refresh_cases_are_all_of_them():
    cases = O.refresh_cases()
    assert tuple(cases) == O.REFRESH_NAMES and len(cases) == 22
    assert max(len(x) for x in cases.values()) == O.ORDER_MAX
    for x0 in cases.values():
        facts(x0)


@pytest.mark.parametrize("B", (5, C.CP_B, C.LIN_B, O.SEQ_B))
def test_explicit_orders(B):
    orders = O.explicit_orders(B)
    assert len(orders) == 3
    for p in orders:
        assert p.dtype == np.int32 and O.is_permutation(p, B) and not O.is_identity(p)
    assert all(not np.array_equal(orders[i], orders[j]) for i in range(3) for j in range(i))
    assert np.all(orders[1] != np.arange(B))      # the rotation leaves no instance in its slot


@pytest.mark.parametrize("model,N", [("cartpole", N) for N in O.ORDER_CP_N] + [("linear", N) for N in O.ORDER_LIN_N])
def test_per_instance_inputs_are_felt(oracle_port, model, N):
    """A parameter row, a pinned u_0 or a cold flag read at a neighbour's index changes that instance's answer by more than RTOL."""
    c, w = C.case(oracle_port, model, N), C.warm_case(oracle_port, model, N)
    th = O.theta_rows(c.ocp, model, c.B)
    assert np.array_equal(th[:, O.N_DYNAMICS[model]:], np.tile(c.ocp.p0[O.N_DYNAMICS[model]:], (c.B, 1)))
    own = oracle_port.solve(c.P, c.x0, p=th)
    assert np.all(own.status == 0)
    assert (np.abs(own.V - c.ref_v.V) / np.maximum(np.abs(c.ref_v.V), 1.0)).min() > C.RTOL      # ... than the shared parameters' V
    # the warm calls of the GPU sequence converge under these parameters, and Q mode is another problem than V mode
    q = oracle_port.solve(c.P, w.x1, p=th, u0fix=c.u0, warm=own)
    v = oracle_port.solve(c.P, w.x1, p=th, warm=q)
    assert np.all(q.status == 0) and np.all(v.status == 0)
    assert (np.abs(q.V - v.V) / np.maximum(np.abs(own.V), 1.0)).max() > C.RTOL
    for other in (oracle_port.solve(c.P, c.x0, p=np.roll(th, 1, 0)), oracle_port.solve(c.P, c.x0, p=np.roll(th, -1, 0))):
        rel = np.abs(other.V - own.V) / np.maximum(np.abs(own.V), 1.0)
        print(f"[order cpu] {model} N {N}: V under a neighbour's parameters moves by {rel.min():.2e} .. {rel.max():.2e}")
        assert np.all(other.status == 0) and rel.min() > C.RTOL
    # two instances given the same x0: the parameters alone move V
    same = oracle_port.solve(c.P, np.tile(c.x0[:1], (c.B, 1)), p=th)
    assert np.abs(same.V[1:] - same.V[0]).min() > C.RTOL * max(1.0, abs(same.V[0]))
    # the pinned u_0 rows differ from their neighbours', and the Q-mode value follows them
    assert np.abs(c.u0 - np.roll(c.u0, 1, 0)).min() > 1e-3 and np.abs(c.u0 - np.roll(c.u0, -1, 0)).min() > 1e-3
    # the cold mask selects some and leaves some, in every wavefront of every layout (at most eight instances per wavefront)
    m = O.cold_mask(c.B)
    assert m.any() and not m.all() and not np.array_equal(m, np.roll(m, 1)) and w.x1.shape == c.x0.shape


def test_iteration_cap_rows_differ(oracle_port):
    """max_iter = 2 at cartpole N = 16: status 2 everywhere, and (status, SQP, interior-point iterations) is not one row repeated."""
    c = C.case(oracle_port, "cartpole", O.ORDER_STATUS_N)
    assert O.ORDER_STATUS_N in C.CP_MAXITER_N
    r = oracle_port.solve(c.P, c.x0, max_iter=O.MAX_ITER)
    assert np.all(r.status == 2)
    rows = np.column_stack([r.status, r.sqp_iter, r.ipm_iter])
    print(f"[order cpu] interior-point iterations at max_iter = {O.MAX_ITER}: {r.ipm_iter}")
    assert len(np.unique(rows, axis=0)) > 1
    # the same cap on a warm call at x1: enough for some instances and not for others, neither by a narrow margin (tol = 1e-6)
    w = C.warm_case(oracle_port, "cartpole", O.ORDER_STATUS_N)
    r = oracle_port.solve(c.P, w.x1, warm=c.ref_v, max_iter=O.MAX_ITER)
    res = r.res.max(1)
    print(f"[order cpu] warm call at max_iter = {O.MAX_ITER}: statuses {r.status}, residuals {res}")
    assert sorted(set(r.status.tolist())) == [0, 2]
    assert res[r.status == 0].max() < 0.8e-6 and res[r.status == 2].min() > 2e-6


@pytest.mark.parametrize("model", ("cartpole", "linear"))
def test_sequence_inputs(oracle_port, model):
    """The 34-step sequences: every step another batch and another tenth of it cold; the range the order is built along has moved by
    step 33; the first and the last batch solve cold on the port; no step is crowded on the state it is ordered on."""
    N = 20 if model == "cartpole" else 8
    P = C.problem(model, N)[1]
    xs, masks = zip(*[O.sequence_inputs(model, t) for t in range(O.SEQ_STEPS)])
    assert all(x.shape == (O.SEQ_B, P.nx) for x in xs) and all(m.sum() == 13 for m in masks)
    assert all(not np.array_equal(masks[t], masks[t + 1]) and not np.array_equal(xs[t], xs[t + 1]) for t in range(O.SEQ_STEPS - 1))
    s0, s32 = O.refresh_state(xs[0]), O.refresh_state(xs[32])
    assert s0 != s32
    for t in range(O.SEQ_STEPS):
        state = s0 if t < 32 else s32
        assert O.largest_bucket(xs[t], state) <= O.BUCKET_MAX and not O.is_identity(O.order(xs[t], state))
    for t in (0, O.SEQ_STEPS - 1):
        assert np.all(oracle_port.solve(P, xs[t], flags=0).status == 0)
