"""The packing order (include/mpcrl.h: mpcrl_set_order, mpcrl_auto_order; csrc/order_kernel.hpp) and every solve kernel under one.

1. order_kernel against the numpy restatement of tests/order_cases.py, permutation and remembered range both array_equal, read back
   through mpcrl_debug_get_order: every from-scratch case on a fresh handle, the cheap path and the refresh cadence (calls 1 and 33),
   calls captured into a graph, the no-ops and the refusals.  tests/test_order_cpu.py holds the restatement to what each case is for.
2. small_solve_kernel, small_solve_sliced_kernel (both park forms), small_sens_kernel, the generic bound rows, lq_solve_kernel<3, 8>,
   <3, 16>, <4, 16> and the chain kernel under explicit permutations (reversal, rotation by one, a shuffle), with per-instance
   parameters, Q mode, a cold mask, warm starts from iterates stored under another order and MPCRL_NO_BND_STORE: torch.equal with an
   identity-order handle run through the same calls, on every output, the stored iterate and the Lagrangian.  The identity run's cold
   V-mode call is held to the C++ CPU port by the comparison rule of tests/small_mode_cases.py.
3. The order as the learners use it: 34 consecutive MPCBatch.solve(reorder=True) calls against reorder=False, and the torch.argsort
   path of batches above 8192.

Measured on an MI355X: the file's 50 cases pass in 4.1 s of wall time, the slowest 0.27 s (cartpole N = 3: eight handles, 50 solves), the
two 34-step sequences 0.03 s each, the 8192- and 8200-instance cases 0.1 s.  Every order comparison is array_equal and every comparison
with the identity run torch.equal.  Largest error of the identity run's cold V-mode call against the port, per family: cartpole 5.2e-14
(N = 62; 1.1e-14 at N = 20, the same with the generic bound rows, and the same bits in both launch shapes), linear system 2.3e-14 at
N = 7 (small_solve_kernel), 2.7e-15 / 1.1e-11 / 2.1e-10 at N = 8 / 24 / 48 (lq_solve_kernel), 2.3e-11 at N = 24 with one stage per lane;
no instance needed the looser bar.

No test found a defect: the order kernel, the refresh cadence, the capture rule and the `perm` reads of all kernels are as documented,
and nothing in the library changed but the read-back probe.  That the tests can fail was checked once against four builds with one
line changed each, every read still in bounds: the crowded-bucket test as `>=`, the widest-coordinate test as `>=` and the cadence as
every 16th call (11 cases fail: equal rows, crowding 64, nan keys 63, tie, cadence, both sequences); the parameter row of
small_solve_kernel read at the slot's index (9 cases: every plain-launch family); the parameter row of small_sens_kernel and the cold
flag of lq_solve_kernel read at the slot's index (14 cases); the pinned u_0 of small_solve_sliced_kernel read at the slot's index
(7 cases: every time-sliced family)."""
import numpy as np
import pytest
import torch

import order_cases as O
import small_mode_cases as C
from small_mode_cases import bit_equal, compare, outputs, raw_solve, same_bits, same_statuses, snapshot

pytestmark = pytest.mark.gpu

E_ARG = -1
SLICING_ILLEGAL = (31, 63)      # as tests/test_gpu_small_modes.py: no spare lane beside the resident slots


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dtype, device="cuda")      # (a copy: the shared batches are read-only)


def order_handle(nx, B):
    """The cheapest handle with more than one instance per wavefront: cartpole N = 3 (nx 4), the linear system at N = 7 (nx 2)."""
    from mpc4rl_amd import MPCBatch
    return MPCBatch(C.problem("cartpole", 3)[0] if nx == 4 else C.problem("linear", 7)[0], B)


def auto_order(mpc, xt):
    from mpc4rl_amd.batch import _ptr
    assert xt.dtype == torch.float64 and xt.is_contiguous() and tuple(xt.shape) == (mpc.B, mpc.nx)
    return mpc.lib.mpcrl_auto_order(mpc._h, _ptr(xt), mpc._stream())


def probe(mpc):
    """(permutation or None, state) of the handle as numpy arrays."""
    perm, state = mpc.get_order()
    torch.cuda.synchronize()
    return (None if perm is None else perm.cpu().numpy()), state.cpu().numpy()


def check_order(mpc, x0, state, what=""):
    """The handle holds the reference's permutation of x0 on this state, and this state: every bit."""
    perm, got = probe(mpc)
    assert perm is not None and perm.dtype == np.int32, what
    assert np.array_equal(got, np.array(state)), (what, got, state)
    assert O.is_permutation(perm, len(x0)), what
    assert np.array_equal(perm, O.order(x0, state)), what
    return perm


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the order kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.REFRESH_NAMES)
def test_refresh_cases(name):
    x0 = O.refresh_cases()[name]
    mpc = order_handle(x0.shape[1], len(x0))
    assert probe(mpc)[0] is None and np.array_equal(probe(mpc)[1], np.array(O.NEVER_REFRESHED))
    assert auto_order(mpc, dev(x0)) == 0
    check_order(mpc, x0, O.refresh_state(x0), name)


def test_order_is_deterministic():
    """The buckets are filled through LDS atomics in arrival order: two fresh handles give the same permutation all the same."""
    x0 = O.uniform(O.ORDER_MAX)
    perms = []
    for _ in range(2):
        mpc = order_handle(4, len(x0))
        xt = dev(x0)
        assert auto_order(mpc, xt) == 0 and auto_order(mpc, xt) == 0      # a from-scratch call, then the cheap path on its own state
        perms.append(check_order(mpc, x0, O.refresh_state(x0)))
    assert np.array_equal(perms[0], perms[1])


def test_refresh_cadence():
    """Call 1 builds the state from scratch, calls 2 .. 32 bucket on it whatever the batch is, call 33 builds it again."""
    a, b, c = O.cheap_a(), O.cheap_b(), O.cheap_c()
    sa, sb = O.refresh_state(a), O.refresh_state(b)
    ta, tb, tc = dev(a), dev(b), dev(c)
    mpc = order_handle(4, O.CHEAP_B)
    assert auto_order(mpc, ta) == 0
    check_order(mpc, a, sa, "call 1")
    for call in range(2, 33):
        assert auto_order(mpc, tb) == 0
        if call in (2, 32):
            check_order(mpc, b, sa, f"call {call}")
    assert auto_order(mpc, tb) == 0
    check_order(mpc, b, sb, "call 33")
    assert auto_order(mpc, tc) == 0
    check_order(mpc, c, sb, "call 34")
    # and C on A's state, one bucket: the identity (a handle of its own: one call on A, one on C)
    mpc = order_handle(4, O.CHEAP_B)
    assert auto_order(mpc, ta) == 0 and auto_order(mpc, tc) == 0
    assert O.is_identity(check_order(mpc, c, sa, "C on A's state"))


def capture_order(mpc, xt):
    torch.cuda.synchronize()
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = auto_order(mpc, xt)
    assert rc == 0
    return g


def replay(g, xt, x0):
    xt.copy_(dev(x0))
    g.replay()
    torch.cuda.synchronize()


def test_order_in_a_captured_graph_on_a_fresh_handle():
    """A first call inside a capture builds the state from scratch at every replay, and does not count as the handle's first call."""
    a, b = O.cheap_a(), O.cheap_b()
    mpc = order_handle(4, O.CHEAP_B)
    xt = dev(a).clone()
    g = capture_order(mpc, xt)
    for x0 in (a, b, a, b):
        replay(g, xt, x0)
        check_order(mpc, x0, O.refresh_state(x0), "replay")
    assert auto_order(mpc, dev(a)) == 0      # the state is B's: a cheap call would leave it
    check_order(mpc, a, O.refresh_state(a), "first eager call")
    assert auto_order(mpc, dev(b)) == 0      # ... and the second eager call is cheap
    check_order(mpc, b, O.refresh_state(a), "second eager call")


def test_order_in_a_captured_graph_after_an_eager_call():
    """Once the state exists a captured call is the cheap form, at every replay."""
    a, b, c = O.cheap_a(), O.cheap_b(), O.cheap_c()
    sa = O.refresh_state(a)
    mpc = order_handle(4, O.CHEAP_B)
    assert auto_order(mpc, dev(a)) == 0
    xt = dev(a).clone()
    g = capture_order(mpc, xt)
    for x0 in (b, b, c, b, a, b):
        replay(g, xt, x0)
        check_order(mpc, x0, sa, "replay")


def test_order_no_ops_and_misuse():
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from mpc4rl_amd.batch import _ptr
    # more instances than the kernel takes: refused, nothing set
    big = order_handle(4, O.ORDER_MAX + 1)
    assert auto_order(big, torch.zeros(O.ORDER_MAX + 1, 4, dtype=torch.float64, device="cuda")) == E_ARG
    assert probe(big)[0] is None
    assert big.lib.mpcrl_auto_order(big._h, None, None) == E_ARG and big.lib.mpcrl_auto_order(None, None, None) == E_ARG
    assert big.lib.mpcrl_debug_get_order(None, None, None, None) == E_ARG
    # one instance per wavefront: a no-op that clears an explicit order
    B = 130
    for ocp in (C.problem("cartpole", 32)[0], chain_mass_ocp(n_mass=3, N=10)):
        mpc = MPCBatch(ocp, B)
        xt = torch.zeros(B, mpc.nx, dtype=torch.float64, device="cuda")
        assert auto_order(mpc, xt) == 0 and probe(mpc)[0] is None
        rev = O.explicit_orders(B)[0]
        mpc.set_order(dev(rev, torch.int32))
        assert np.array_equal(probe(mpc)[0], rev)
        assert mpc.lib.mpcrl_debug_get_order(mpc._h, None, None, None) == 1      # the answer alone
        assert auto_order(mpc, xt) == 0 and probe(mpc)[0] is None
        assert np.array_equal(probe(mpc)[1], np.array(O.NEVER_REFRESHED))
    # set_order(None) after an auto order; the probe leaves perm_out alone when there is no order
    x0 = O.nx2()
    mpc = order_handle(2, len(x0))
    assert auto_order(mpc, dev(x0)) == 0
    check_order(mpc, x0, O.refresh_state(x0))
    mpc.set_order(None)
    assert probe(mpc)[0] is None
    out = torch.full((len(x0),), -7, dtype=torch.int32, device="cuda")
    assert mpc.lib.mpcrl_debug_get_order(mpc._h, _ptr(out), None, mpc._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert np.array_equal(probe(mpc)[1], np.array(O.refresh_state(x0)))      # the remembered range stays


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. every solve kernel under explicit permutations
# ---------------------------------------------------------------------------------------------------------------------------------
def flags(cold, extra=0):
    from mpc4rl_amd import _lib
    return _lib.SENS_V | _lib.SENS_PI | (_lib.COLD if cold else 0) | extra


def solve_handle(c, mode, monkeypatch, env=None):
    from mpc4rl_amd import MPCBatch
    for name in ("MPCRL_GENERIC_ROWS", "MPCRL_LINEAR_SPL", "MPCRL_TIME_SLICE"):
        monkeypatch.delenv(name, raising=False)
    if env is not None:
        monkeypatch.setenv(env, "1")
    mpc = MPCBatch(c.ocp, c.B)
    if env is not None:
        monkeypatch.delenv(env, raising=False)
    if mode is not None:
        mpc.set_launch_mode(mode)
    if c.model == "cartpole":      # the launch shape, as test_gpu_small_modes expects it for the horizon
        expect = 1 if (mode == 1 and c.N not in SLICING_ILLEGAL) else 0
        assert mpc.lib.mpcrl_query_time_sliced(mpc._h, flags(True), mpc._stream()) == expect
        assert mpc.lib.mpcrl_query_box_rows(mpc._h) == (0 if env == "MPCRL_GENERIC_ROWS" else 1)
    return mpc


def call_sequence(c, w, mpc, orders, start):
    """The calls of one handle, call j under orders[(start + j) % 3] (orders = None: the identity throughout).  Returns the snapshot of
    every call: cold V with shared parameters; cold V with per-instance parameters; warm Q at x1 with u_0 pinned per instance; warm V
    at x1 with a cold mask on every third instance; cold V that leaves the bound planes alone; warm V after it."""
    from mpc4rl_amd import _lib
    from mpc4rl_amd.batch import _ptr
    mask = dev(O.cold_mask(c.B).astype(np.int32), torch.int32)
    theta = dev(O.theta_rows(c.ocp, c.model, c.B))
    calls = [
        dict(x0=c.x0, fl=flags(True)),
        dict(x0=c.x0, fl=flags(True), theta=theta),
        dict(x0=w.x1, fl=flags(False), u0=c.u0),
        dict(x0=w.x1, fl=flags(False), mask=mask),
        dict(x0=c.x0, fl=flags(True, _lib.NO_BND_STORE)),
        dict(x0=w.x1, fl=flags(False)),
    ]
    snaps = []
    for j, k in enumerate(calls):
        if orders is not None:
            p = orders[(start + j) % 3]
            mpc.set_order(dev(p, torch.int32))
            assert np.array_equal(probe(mpc)[0], p)
        else:
            assert probe(mpc)[0] is None
        if "theta" in k:
            mpc.set_theta(k["theta"])
        if "mask" in k:
            assert mpc.lib.mpcrl_set_cold_mask(mpc._h, _ptr(k["mask"]), mpc._stream()) == 0
        snaps.append(snapshot(mpc, raw_solve(mpc, k["x0"], k.get("u0"), flags=k["fl"])))
    return snaps


WORST = {}      # largest port error per family, printed with -s


def under_orders(oracle_port, monkeypatch, model, N, mode, env=None):
    c, w = C.case(oracle_port, model, N), C.warm_case(oracle_port, model, N)
    orders = O.explicit_orders(c.B)
    assert all(O.is_permutation(p, c.B) and not O.is_identity(p) for p in orders)
    what = f"{model} N {N}" + ("" if mode is None else f" mode {mode:+d}") + ("" if env is None else f" {env}=1")
    ident = solve_handle(c, mode, monkeypatch, env)
    base = call_sequence(c, w, ident, None, 0)
    # the identity run's first call against the port; its later calls did something else than the first
    r0 = base[0][0]
    got = {"status": r0.status, "iters": r0.iters, "u0": r0.u0, "V": r0.V, "dV": r0.dV_dp, "dpi": r0.dpi_dp, "X": base[0][1][0], "U": base[0][1][1],
           "PI": base[0][1][2]}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    same_statuses(got, c.ref_v)
    err, _ = compare(got, c.ref_v, c.lq and env != "MPCRL_LINEAR_SPL", tag=what + ": identity order, cold V", suite="order")
    fam = model + ("" if env is None else " " + env)
    WORST[fam] = max(WORST.get(fam, 0.0), err)
    print(f"[order] largest port error so far, {fam}: {WORST[fam]:.3e}")
    V = [s[0].V for s in base]
    scale = torch.clamp(V[0].abs(), min=1.0)
    assert float(((V[1] - V[0]).abs() / scale).min()) > C.RTOL       # per-instance parameters move every instance's V
    assert float(((V[2] - V[3]).abs() / scale).max()) > C.RTOL       # Q mode is another problem than V mode at the same x1
    assert bool((base[2][0].dpi_dp == 0.0).all())
    for j in range(1, 6):
        assert bool((base[j][0].status == 0).all()), (what, j, base[j][0].status)
    for start in range(3):
        snaps = call_sequence(c, w, solve_handle(c, mode, monkeypatch, env), orders, start)
        for j, (a, b) in enumerate(zip(snaps, base)):
            try:
                same_bits(a, b)
            except AssertionError as e:
                raise AssertionError(f"{what}: call {j} under order {(start + j) % 3} differs from the identity run in {e}") from e
    # two instances given the same x0: the parameter rows alone move V, so a row read at another index cannot go unseen
    same = raw_solve(ident, np.tile(c.x0[:1], (c.B, 1)))
    assert float((same.V[1:] - same.V[0]).abs().min()) > C.RTOL * max(1.0, abs(float(same.V[0])))
    return base


@pytest.mark.parametrize("N", O.ORDER_CP_N)
def test_cartpole_solves_under_orders(oracle_port, monkeypatch, N):
    plain = under_orders(oracle_port, monkeypatch, "cartpole", N, -1)
    sliced = under_orders(oracle_port, monkeypatch, "cartpole", N, 1)
    for a, b in zip(plain, sliced):
        same_bits(a, b)


@pytest.mark.parametrize("mode", (-1, 1))
def test_cartpole_generic_rows_under_orders(oracle_port, monkeypatch, mode):
    under_orders(oracle_port, monkeypatch, "cartpole", O.ORDER_GENERIC_N, mode, env="MPCRL_GENERIC_ROWS")


@pytest.mark.parametrize("N", O.ORDER_LIN_N)
def test_linear_solves_under_orders(oracle_port, monkeypatch, N):
    under_orders(oracle_port, monkeypatch, "linear", N, None)


def test_linear_one_stage_per_lane_under_orders(oracle_port, monkeypatch):
    under_orders(oracle_port, monkeypatch, "linear", O.ORDER_SPL1_N, None, env="MPCRL_LINEAR_SPL")


def test_chain_ignores_an_order():
    """The chain kernels have a wavefront per instance and do not read the order: a reversal changes nothing."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    B = 5
    ocp = chain_mass_ocp(n_mass=3, N=10)
    M = (ocp.nx // 3 - 1) // 2
    x0 = np.tile(ocp.x0, (B, 1))
    x0[:, 3 * (M + 1):] += np.random.default_rng(67).normal(0.0, 1e-2, (B, 3 * M))
    snaps = []
    for p in (None, O.explicit_orders(B)[0]):
        mpc = MPCBatch(ocp, B)
        mpc.set_order(None if p is None else dev(p, torch.int32))
        assert (probe(mpc)[0] is None) == (p is None)
        snaps.append(snapshot(mpc, raw_solve(mpc, x0)))
    assert bool((snaps[0][0].status == 0).all()) and len(torch.unique(snaps[0][0].V)) == B
    same_bits(snaps[0], snaps[1])


@pytest.mark.parametrize("mode", (-1, 1))
def test_statuses_under_an_order(oracle_port, monkeypatch, mode):
    """max_iter = 2: status 2 and the iteration counts of every instance, bit for bit the identity run's, and not one row repeated; on
    a warm call under that cap statuses 0 and 2 side by side, the port's."""
    c = C.case(oracle_port, "cartpole", O.ORDER_STATUS_N)
    runs = []
    for p in (None,) + O.explicit_orders(c.B):
        mpc = solve_handle(c, mode, monkeypatch)
        mpc.set_options(max_iter=O.MAX_ITER)
        mpc.set_order(None if p is None else dev(p, torch.int32))
        runs.append(snapshot(mpc, raw_solve(mpc, c.x0)))
    r = runs[0][0]
    assert bool((r.status == 2).all()) and bool((r.iters[:, 0] == O.MAX_ITER).all())
    rows = torch.cat([r.status[:, None], r.iters], 1)
    assert len(torch.unique(rows, dim=0)) > 1, rows
    for other in runs[1:]:
        assert torch.equal(other[0].status, r.status) and torch.equal(other[0].iters, r.iters)
        same_bits(other, runs[0])
    # the same cap on a warm call at x1: two SQP iterations are enough for some instances and not for others (the port's statuses)
    w = C.warm_case(oracle_port, "cartpole", O.ORDER_STATUS_N)
    ref = oracle_port.solve(c.P, w.x1, warm=c.ref_v, max_iter=O.MAX_ITER)
    orders = O.explicit_orders(c.B)
    runs = []
    for i in range(4):
        mpc = solve_handle(c, mode, monkeypatch)
        mpc.set_order(None if i == 0 else dev(orders[i - 1], torch.int32))
        raw_solve(mpc, c.x0)
        mpc.set_options(max_iter=O.MAX_ITER)
        mpc.set_order(None if i == 0 else dev(orders[i % 3], torch.int32))
        runs.append(snapshot(mpc, raw_solve(mpc, w.x1, flags=flags(False))))
    r = runs[0][0]
    assert np.array_equal(r.status.cpu().numpy(), ref.status) and sorted(set(r.status.tolist())) == [0, 2]
    for other in runs[1:]:
        assert torch.equal(other[0].status, r.status) and torch.equal(other[0].iters, r.iters)
        same_bits(other, runs[0])


@pytest.mark.parametrize("model,N", [("cartpole", 16), ("linear", 8)])
def test_row_tables_under_an_order(oracle_port, monkeypatch, model, N):
    """mpcrl_get_iterate_rows after a solve under the shuffle: table row index[i] is instance i's stored iterate."""
    c = C.case(oracle_port, model, N)
    mpc = solve_handle(c, -1 if model == "cartpole" else None, monkeypatch)
    mpc.set_order(dev(O.explicit_orders(c.B)[2], torch.int32))
    raw_solve(mpc, c.x0)
    x, u, pi, bnd, _ = mpc.get_iterate()
    picked = [0, 4, 7, c.B - 1]
    index = torch.full((c.B,), -1, dtype=torch.int64, device="cuda")
    for row, inst in enumerate(picked):
        index[inst] = len(picked) - 1 - row
    tables = [torch.full((len(picked),) + tuple(t.shape[1:]), np.nan, dtype=torch.float64, device="cuda") for t in (x, u, pi, bnd)]
    mpc.get_iterate_rows(*tables, index)
    torch.cuda.synchronize()
    sel = torch.as_tensor(picked[::-1], device="cuda")
    for t, full in zip(tables, (x, u, pi, bnd)):
        assert torch.equal(t, full[sel])
    assert len(torch.unique(x[sel][:, 0, 0])) == len(picked)      # four different instances


@pytest.mark.parametrize("mode", (-1, 1))
def test_nan_instance_under_an_order(oracle_port, monkeypatch, mode):
    """The NaN row of test_nan_instance_leaves_its_neighbours_alone moved among other neighbours: every other row keeps its bits."""
    c = C.case(oracle_port, "cartpole", O.ORDER_NAN_N)
    ipw = 64 // (c.N + 1)
    x0 = c.x0.copy()
    x0[1] = np.nan
    others = torch.arange(c.B, device="cuda") != 1
    ident = solve_handle(c, mode, monkeypatch)
    base = snapshot(ident, raw_solve(ident, x0))
    assert base[0].status.tolist() == [0, 1] + [0] * (c.B - 2)
    for p in O.explicit_orders(c.B):
        slot = int(np.flatnonzero(p == 1)[0])
        mates = set(p[slot // ipw * ipw: slot // ipw * ipw + ipw].tolist())
        assert mates != set(range(ipw))      # (plain launch) another wavefront's worth of neighbours than under the identity
        mpc = solve_handle(c, mode, monkeypatch)
        mpc.set_order(dev(p, torch.int32))
        snap = snapshot(mpc, raw_solve(mpc, x0))
        assert torch.equal(snap[0].status, base[0].status)
        same_bits(snap, base, rows=others)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the order as the learners use it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [("cartpole", 20), ("linear", 8)])
def test_warm_sequence_with_auto_order(model, N):
    """34 consecutive solves of a slowly moving batch of 130, a tenth of it cold at every step: reorder=True returns the bits of
    reorder=False at every step, and the handle held the reference's order of that step's batch — built from scratch at steps 1 and 33."""
    from mpc4rl_amd import MPCBatch
    ocp = C.problem(model, N)[0]
    a, b = MPCBatch(ocp, O.SEQ_B), MPCBatch(ocp, O.SEQ_B)
    a.set_launch_mode(-1), b.set_launch_mode(-1)
    states, moved = [np.array(O.NEVER_REFRESHED)], 0
    for t in range(O.SEQ_STEPS):
        x0, mask = O.sequence_inputs(model, t)
        xt, mt = dev(x0), dev(mask.astype(np.int32), torch.int32)
        assert a.lib.mpcrl_query_time_sliced(a._h, flags(False), a._stream()) == 0
        ra = a.solve(xt, sens_v=True, sens_pi=True, cold_mask=mt, reorder=True)
        rb = b.solve(xt, sens_v=True, sens_pi=True, cold_mask=mt, reorder=False)
        bit_equal(ra, rb)
        assert bool((ra.status == 0).all()), (t, ra.status)
        perm, state = probe(a)
        assert perm is not None and O.is_permutation(perm, O.SEQ_B) and probe(b)[0] is None
        moved += not O.is_identity(perm)
        ref_state = O.refresh_state(O.sequence_inputs(model, 0 if t < 32 else 32)[0])
        assert np.array_equal(state, np.array(ref_state)), (t, state, ref_state)
        assert np.array_equal(perm, O.order(x0, ref_state)), t
        states.append(state)
    changed = [t for t in range(O.SEQ_STEPS) if not np.array_equal(states[t], states[t + 1])]
    assert changed == [0, 32], changed      # steps 1 and 33
    assert moved >= 1
    same_bits(snapshot(a, ra), snapshot(b, rb))


def test_argsort_path_above_8192():
    """MPCBatch._pack_order for more instances than order_kernel takes: a torch.argsort through mpcrl_set_order."""
    from mpc4rl_amd import MPCBatch
    x0 = O.uniform(O.ARGSORT_B)
    ocp = C.problem("cartpole", 3)[0]
    a, b = MPCBatch(ocp, O.ARGSORT_B), MPCBatch(ocp, O.ARGSORT_B)
    a.set_launch_mode(-1), b.set_launch_mode(-1)
    ra = a.solve(dev(x0), sens_v=True, sens_pi=True, cold=True, reorder=True)
    rb = b.solve(dev(x0), sens_v=True, sens_pi=True, cold=True, reorder=False)
    perm = probe(a)[0]
    assert perm is not None and O.is_permutation(perm, O.ARGSORT_B) and not O.is_identity(perm) and probe(b)[0] is None
    d = int(O.refresh_state(x0)[2])
    assert np.all(np.diff(x0[perm, d]) >= 0.0)
    assert bool((ra.status == 0).all())
    same_bits(snapshot(a, ra), snapshot(b, rb))
