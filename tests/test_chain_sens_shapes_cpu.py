"""The fixture G17 (tests/golden/make_chain_sens_shapes.py) without a GPU: it holds what its generator promises — every instance of
every set, the shapes that put the flattened (instance, stage) kernels past one 64-lane workgroup and the horizons up to 63, both
gates, the active rows where they are required — and it is consistent with itself: the directions and the cotangents contract the
same dense Jacobians (<G, dW> = g_x0 . vx + g_theta . vp), row 0 of dX is the direction, the u_0 rows of dU are du0*/dp and du0*/dx0
applied to the directions, and the neighbouring instance's rows are far enough away for the
negative control of tests/test_gpu_chain_sens_shapes.py to see an instance index that is off by one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# (n_mass, N, base, B, stage lanes B N, instances that come from the act recipe)
SETS = ((3, 10, "mix", 13, 130, (0, 3, 6, 12)), (3, 16, "ss", 8, 128, ()), (3, 40, "mix", 3, 120, (0,)), (3, 63, "ss", 2, 126, ()),
        (5, 40, "ss", 2, 80, ()), (7, 33, "ss", 2, 66, ()))
GATE, R, C = 1e-6, 3, 2      # the gate, the directions, the stored cotangents (the third of the gate, the unit one, is not stored)


@pytest.fixture(scope="module")
def g17():
    return np.load(os.path.join(GOLD, "g17_chain_sens_shapes.npz"))


@pytest.fixture(scope="module")
def generator():
    sys.path.insert(0, GOLD)
    try:
        import make_chain_sens_shapes
    finally:
        sys.path.remove(GOLD)
    return make_chain_sens_shapes


def dims(n_mass):
    nx = (2 * (n_mass - 2) + 1) * 3
    return nx, 3, 10 * (n_mass - 1) + nx * nx + 9 + 3 * (n_mass - 2)


def w_of(fx, k):
    """dW [B, R, nw] in the mirror's order [U; X]."""
    B = len(fx[k + "x0"])
    return np.concatenate([fx[k + "dU"].reshape(B, R, -1), fx[k + "dX"].reshape(B, R, -1)], 2)


def rows_apart(v):
    """Per instance: the distance of its row from the next instance's, scaled by max(|that row|, 1) — what the GPU test's negative
    control measures when the library returns the right numbers."""
    v = v.reshape(len(v), -1)
    nb = np.roll(v, -1, 0)
    return np.abs(v - nb).max(1) / np.maximum(np.abs(nb).max(1), 1.0)


def test_the_sets_are_the_generators_and_the_file_is_no_larger_than_the_largest_fixture(g17, generator):
    assert tuple(s[:4] for s in SETS) == generator.SETS and generator.ACT_AT == {(3, 10): (0, 3, 6, 12), (3, 40): (0,)}
    assert generator.g16.GATE == generator.g12.GATE == generator.GATE == GATE == float(g17["gate"])
    assert generator.g16.TOL == generator.g12.TOL == generator.TOL == 1e-10 == float(g17["tol"])
    assert generator.g16.R == generator.g12.R == R and float(g17["sigma"]) == 0.01 and float(g17["sigma_act"]) == generator.g12.SIGMA_ACT == 0.2
    names = {f"m{s[0]}_N{s[1]}_{s[2]}_{k}" for s in SETS for k in generator.KEYS + ("act",)} | {"tol", "gate", "sigma", "sigma_act"}
    assert set(g17.files) == names
    size = os.path.getsize(os.path.join(GOLD, "g17_chain_sens_shapes.npz"))
    assert size <= max(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if f.endswith(".npz") and not f.startswith("g17_"))


@pytest.mark.parametrize("n_mass,N,base,B,lanes,act_at", SETS)
def test_fixture_shapes_gates_and_workgroup_geometry(g17, generator, n_mass, N, base, B, lanes, act_at):
    from oracle.problems import make_chain_mass
    nx, nu, n_p = dims(n_mass)
    nw = N * nu + (N + 1) * nx
    k = f"m{n_mass}_N{N}_{base}_"
    shapes = dict(x0=(B, nx), vx=(B, R, nx), vp=(B, R, n_p), dX=(B, R, N + 1, nx), dU=(B, R, N, nu), G=(B, C, nw), g_theta=(B, C, n_p),
                  g_x0=(B, C, nx), g_lb=(B, C, N, nu), g_ub=(B, C, N, nu), dpi_dp=(B, nu, n_p), dpi_dx0=(B, nu, nx), dV_dx0=(B, nx),
                  agree=(B, 2), draw=(B, 2), active=(B, N, nu), act=(B,))
    for name, shape in shapes.items():
        assert g17[k + name].shape == shape, name
        assert np.isfinite(g17[k + name]).all(), name
    assert np.all(g17[k + "agree"] <= GATE) and np.all(g17[k + "draw"] >= 0) and np.all(g17[k + "draw"] < generator.g16.DRAWS)
    # the geometry the set is there for: lanes gid = inst N + k in workgroups of 64
    assert B * N == lanes
    groups, tail = -(-lanes // 64), lanes % 64
    straddlers = [i for i in range(B) if (i * N) // 64 != (i * N + N - 1) // 64]
    want = {(3, 10): (3, 2, [6, 12]), (3, 16): (2, 0, []), (3, 40): (2, 56, [1]), (3, 63): (2, 62, [1]), (5, 40): (2, 16, [1]), (7, 33): (2, 2, [1])}
    assert (groups, tail, straddlers) == want[n_mass, N]
    # where the instances come from
    assert np.flatnonzero(g17[k + "act"]).tolist() == list(act_at)
    # candidates of the generator's two draws, in draw order; the first draw of the directions is G16's seed rule on the candidate
    ss, cand = generator.draw_x0(make_chain_mass(n_mass=n_mass, N=N), n_mass, N, base, B)
    assert generator.SPARE == 4 and len(ss) == 4 * (B - len(act_at)) and len(cand) == 4 * len(act_at)
    for pool, slots, tail in ((ss, np.flatnonzero(~g17[k + "act"]), 0), (cand, np.flatnonzero(g17[k + "act"]), 100)):
        which = [next(j for j, c in enumerate(pool) if np.array_equal(g17[k + "x0"][i], c)) for i in slots]
        assert which == sorted(set(which))
        for i, c in zip(slots, which):
            if g17[k + "draw"][i, 0] == 0:
                rng = np.random.default_rng([17100 + 100 * n_mass + N, tail + c])
                assert np.array_equal(rng.standard_normal((R, nx))[0], g17[k + "vx"][i, 0])
    assert np.all(g17[k + "active"][g17[k + "act"]][:, 1:].sum((1, 2)) >= 1)      # a control row on its bound inside the sweep
    assert not g17[k + "active"][~g17[k + "act"]][:, 1:].any()                    # near x_ss nothing is active past stage 0
    # direction 0 moves x0 and every entry of p; direction 1 the dynamics block and w only; direction 2 x0 only
    vx, vp = g17[k + "vx"], g17[k + "vp"]
    off_q, off_w = 10 * (n_mass - 1), 10 * (n_mass - 1) + nx * nx + nu * nu
    assert np.all(vx[:, 0] != 0) and np.all(vp[:, 0] != 0)
    assert np.all(vx[:, 1] == 0) and np.all(vp[:, 1, off_q:off_w] == 0) and np.all(vp[:, 1, :off_q] != 0) and np.all(vp[:, 1, off_w:] != 0)
    assert np.all(vx[:, 2] != 0) and np.all(vp[:, 2] == 0)
    assert np.all(g17[k + "G"] != 0) and generator.COTANGENT_KEYS == ("G", "g_theta", "g_x0", "g_lb", "g_ub")


@pytest.mark.parametrize("n_mass,N,base,B,lanes,act_at", SETS)
def test_fixture_is_consistent_with_itself(g17, n_mass, N, base, B, lanes, act_at):
    k = f"m{n_mass}_N{N}_{base}_"
    dW, G, vx, vp = w_of(g17, k), g17[k + "G"], g17[k + "vx"], g17[k + "vp"]
    # <G, dW> = g_x0 . vx + g_theta . vp: the directions and the cotangents contract the same dense Jacobians
    lhs = np.einsum("bcw,brw->bcr", G, dW)
    rhs = np.einsum("bcx,brx->bcr", g17[k + "g_x0"], vx) + np.einsum("bcp,brp->bcr", g17[k + "g_theta"], vp)
    scale = np.maximum(np.einsum("bcw,brw->bcr", np.abs(G), np.abs(dW)), 1.0)
    assert (np.abs(lhs - rhs) / scale).max() <= 1e-9
    # x_0 = x0: row 0 of dX is the direction itself — to the gate in the gate's own scale: the mirror pins x_0 by a pair of bound rows
    # of finite stiffness
    assert (np.abs(g17[k + "dX"][:, :, 0] - vx).max(2) / np.maximum(np.abs(g17[k + "dX"]).max((2, 3)), 1.0)).max() <= GATE
    # the u_0 rows of dU are the policy sensitivities applied to the directions
    u0 = np.einsum("bup,brp->bru", g17[k + "dpi_dp"], vp) + np.einsum("bux,brx->bru", g17[k + "dpi_dx0"], vx)
    assert (np.abs(g17[k + "dU"][:, :, 0] - u0).max(2) / np.maximum(np.abs(u0).max(2), 1.0)).max() <= 1e-9
    # the bound gradients are on the rows that exist; where nothing is active they are of the barrier's size
    if not g17[k + "active"].any():
        assert max(np.abs(g17[k + "g_lb"]).max(), np.abs(g17[k + "g_ub"]).max()) <= GATE


@pytest.mark.parametrize("n_mass,N,base,B,lanes,act_at", SETS)
def test_the_neighbours_rows_are_far_enough_for_the_negative_control(g17, n_mass, N, base, B, lanes, act_at):
    """Every instance, not only the worst: 10 gates between an instance's reference rows and the next instance's, for each quantity the
    GPU test holds against the neighbour's rows.  The bound gradients take part on the mix sets, through the instances with an active
    row (an inactive row's gradient is about tau / t^2: nothing to tell apart near x_ss)."""
    k = f"m{n_mass}_N{N}_{base}_"
    dW = w_of(g17, k)
    for r in range(R):
        assert rows_apart(dW[:, r]).min() >= 10 * GATE
    for c in range(C):
        assert rows_apart(g17[k + "g_theta"][:, c]).min() >= 10 * GATE and rows_apart(g17[k + "g_x0"][:, c]).min() >= 10 * GATE
    assert rows_apart(g17[k + "dpi_dx0"]).min() >= 10 * GATE and rows_apart(g17[k + "dV_dx0"]).min() >= 10 * GATE
    if base == "mix":
        for c in range(C):
            assert rows_apart(np.stack([g17[k + "g_lb"][:, c], g17[k + "g_ub"][:, c]], 1)).max() >= 10 * GATE
