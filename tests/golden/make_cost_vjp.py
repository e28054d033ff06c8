"""G14 — derivatives of the cartpole's planned trajectory w* = [u_0 .. u_{N-1}; x_0 .. x_N] and of its value V with respect to the
tracking cost, the 80 entries W_0, W, W_e, yref_0, yref, yref_e of p (entries 3 .. 82), each an independent variable, from the mirror
of the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.  Writes tests/golden/g14_cost_vjp.npz.  CPU only:

    python tests/golden/make_cost_vjp.py          (two and a half minutes on eight cores)

The recipe is G13's (make_bound_vjp.py), imported from there and from make_traj_vjp.py where it is code.  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``solution_from_iterate`` and ``nlp_mirror.evaluate`` on the problem with a PARAMETERISED cost: ``parameterised`` replaces the two
     cost closures of oracle/problems.py by the same expressions without the ``detach`` (``dataclasses.replace``; nothing under
     oracle/ changes), so that the mirror's dR_dp and dL_dp have a cost block.  l = 1/2 r' W r with W as it stands in p: its Hessian
     is 1/2 (W + W'), what the solve uses;
  3. J = solve(dR_dz, -dR_dp)[:nw];
  4. R = 3 cotangents G on w as in G11 / G13: two standard-normal draws over all of w and the unit cotangent on component 0 of u_0;
  5. stored: ``x0``, ``p`` [83], ``G`` [R, nw], ``g_cost`` [R, 83] = G J on the cost block and exactly 0 on entries 0 .. 2,
     ``dV_dcost`` [83] = dL_dp likewise, the mirror's du0*/dp on the dynamics block (``dpi_dp`` [nu, 3]: the bar of the GPU test is
     relative to the error of the solve's own du0*/dp), G13's class flags and masks (``interior, act_u, act_u0, act_x, act_lb,
     act_ub``), ``agree``, ``agree_V``, and per set the bounds (``lb0, ub0, lb, ub, lbe, ube``: G13's tightened boxes).
     The mirror's gradients with respect to W[a, b] and W[b, a] are the same number up to rounding (1/2 r_a r_b; 1/2 (y_a r_b + y_b r_a));
     the stored blocks are symmetrised, 1/2 (g + g'), so that they are the same bits, as the library's are.
Gate: extrapolated central differences (h = 2e-4 and 1e-4, (4 f(h/2) - f(h)) / 3) of the port's whole (U, X) and of V over the 80
entries, against G J and dL_dp, rows scaled by max(|row|, 1) (G11's ``scaled``): 1e-6 for both.  That is wider than G13's 1e-7:
there are 80 directions, some of scale 0.01 (W_uu), and gradients up to 1e3 on a normal cotangent.  An instance also enters only if
every row is active or clearly not (G13's ``classify``) and if the port's default mode (the product's twin) solves it at tol 1e-9.

Set A (``A_N{N}_``): G13's cartpole instances — their x0, bounds and classes — at the nominal p0, horizons 2, 15, 20, 31, 32, 63.
Set B (``B_N{N}_``): a per-instance p, horizons 2, 15, 20, 32, on fresh draws of x0 in G13's range and G13's bounds.  Every weight is
W + L L' + (K - K'), L ~ 0.1 N(0, 1) of shape n x 2, K ~ 0.01 N(0, 1): positive definite in its symmetric part, NOT symmetric, not
diagonal; every reference ~ 0.1 N(0, 1).  Up to DRAWS_B candidates per horizon are tried in rounds, in draw order, until PER_B of them
have passed with ACTIVE_B of them on an active control row.
The generator fails rather than deliver fewer than REQUIRED_A of G13's instances per horizon, an ``act_x`` instance at N = 15, 20, 32
or 63, or fewer than REQUIRED_B instances (one with an active control row) per horizon of set B.

FOUND (the run that wrote the committed file; what it printed):
  A N 2: 5 of G13's 5 instances pass; turned away: []
  A_N2_: 5 instances, per class {interior: 2, act_u: 3, act_u0: 3, act_x: 0}, agreement w 7.3e-07 V 2.0e-10, largest |g_cost| on a normal cotangent 6.44e+01
  A N 15: 7 of G13's 7 instances pass; turned away: []
  A_N15_: 7 instances, per class {interior: 2, act_u: 4, act_u0: 4, act_x: 2}, agreement w 1.3e-07 V 8.3e-09, largest |g_cost| on a normal cotangent 9.11e+02
  A N 20: 5 of G13's 6 instances pass; turned away: ['difference unsolved']
  A_N20_: 5 instances, per class {interior: 2, act_u: 3, act_u0: 3, act_x: 1}, agreement w 7.7e-07 V 3.9e-09, largest |g_cost| on a normal cotangent 5.52e+02
  A N 31: 5 of G13's 5 instances pass; turned away: []
  A_N31_: 5 instances, per class {interior: 2, act_u: 3, act_u0: 3, act_x: 2}, agreement w 4.8e-07 V 1.2e-09, largest |g_cost| on a normal cotangent 5.59e+02
  A N 32: 5 of G13's 6 instances pass; turned away: ['difference unsolved']
  A_N32_: 5 instances, per class {interior: 2, act_u: 3, act_u0: 3, act_x: 1}, agreement w 4.3e-07 V 4.3e-09, largest |g_cost| on a normal cotangent 8.15e+02
  A N 63: 6 of G13's 7 instances pass; turned away: ['difference unsolved']
  A_N63_: 6 instances, per class {interior: 2, act_u: 4, act_u0: 4, act_x: 2}, agreement w 2.9e-07 V 5.5e-09, largest |g_cost| on a normal cotangent 1.43e+03
  B N 2: of 64 draws 0 not solved, 4 unclear, 33 solved ones on an active control row; gate run on 4, turned away []
  B_N2_: 4 instances, per class {interior: 1, act_u: 0, act_u0: 3, act_x: 0}, agreement w 4.4e-08 V 6.6e-11, largest |g_cost| on a normal cotangent 4.76e+01
  B N 15: of 64 draws 12 not solved, 0 unclear, 5 solved ones on an active control row; gate run on 5, turned away ['24: gate 1.3e-06 6.6e-09']
  B_N15_: 4 instances, per class {interior: 2, act_u: 2, act_u0: 1, act_x: 1}, agreement w 2.4e-07 V 5.7e-10, largest |g_cost| on a normal cotangent 2.07e+02
  B N 20: of 64 draws 15 not solved, 2 unclear, 8 solved ones on an active control row; gate run on 4, turned away []
  B_N20_: 4 instances, per class {interior: 2, act_u: 2, act_u0: 2, act_x: 0}, agreement w 4.8e-08 V 7.8e-10, largest |g_cost| on a normal cotangent 3.72e+02
  B N 32: of 64 draws 24 not solved, 2 unclear, 14 solved ones on an active control row; gate run on 4, turned away []
  B_N32_: 4 instances, per class {interior: 2, act_u: 2, act_u0: 2, act_x: 1}, agreement w 7.2e-07 V 4.6e-09, largest |g_cost| on a normal cotangent 1.71e+02
In set A the instances turned away are those where one of the 320 perturbed exact-QP solves does not reach tol 1e-10; none misses the
gate itself.  In set B between a fifth and a third of the draws at N >= 15 do not solve in one of the two modes (the full-step SQP
ends with status 2 or 4 on these weights), and instances on an active control row are scarce at N = 15: the stream SEED_B = 14100 holds
three there, of which one misses the gate at 1.2e-6 and two have a perturbed solve that does not converge, so the committed stream is
14101, where three of five pass and one misses at 1.3e-6.  The gate was not moved.
"""
import dataclasses
import os
import sys
from multiprocessing import Pool

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import cpu_port, nlp_mirror  # noqa: E402
from oracle.from_iterate import solution_from_iterate  # noqa: E402
from make_traj_vjp import R, TOL, scaled, w_of  # noqa: E402
from make_bound_vjp import CLASSES, X0_SCALE, bounded, classify, groups  # noqa: E402

GATE = 1e-6
NP, NDYN = 83, 3
COST = np.arange(NDYN, NP)
HORIZONS_A, HORIZONS_B = (2, 15, 20, 31, 32, 63), (2, 15, 20, 32)
REQUIRED_A, ACT_X_AT = 5, (15, 20, 32, 63)
DRAWS_B, PER_B, ACTIVE_B, REQUIRED_B = 64, 4, 2, 3
SEED_B = 14101      # (the stream 14100 holds three solved candidates on an active control row at N = 15 and none passes, see FOUND)
BLOCKS = ((3, 5), (28, 5), (53, 4))          # (offset, side) of W_0, W, W_e in p, each column-major
REFS = ((69, 5), (74, 5), (79, 4))           # yref_0, yref, yref_e
KEYS = ("x0", "p", "G", "g_cost", "dV_dcost", "dpi_dp", "act_lb", "act_ub", "agree", "agree_V") + CLASSES


def parameterised(P):
    """The cartpole problem with the cost block of p as variables: the closures of oracle/problems.py without their ``detach``."""
    def stage_cost(k, x, u, p):
        Wk = (p[3:28] if k == 0 else p[28:53]).reshape(5, 5).T
        y = torch.cat([x, u]) - (p[69:74] if k == 0 else p[74:79])
        return 0.5 * y @ (Wk @ y)

    def terminal_cost(x, p):
        y = x - p[79:83]
        return 0.5 * y @ (p[53:69].reshape(4, 4).T @ y)

    return dataclasses.replace(P, stage_cost=stage_cost, terminal_cost=terminal_cost)


def perturbed_p(p0, rng):
    """Set B's parameter vector: every weight W + L L' + (K - K'), every reference 0.1 N(0, 1)."""
    p = p0.copy()
    for o, n in BLOCKS:
        L, K = 0.1 * rng.standard_normal((n, 2)), 0.01 * rng.standard_normal((n, n))
        W = p[o:o + n * n].reshape(n, n).T + L @ L.T + (K - K.T)
        p[o:o + n * n] = W.flatten("F")
    for o, n in REFS:
        p[o:o + n] = 0.1 * rng.standard_normal(n)
    return p


def symmetrised(g):
    """[..., 83] with every W block replaced by 1/2 (g + g')."""
    g = g.copy()
    for o, n in BLOCKS:
        b = g[..., o:o + n * n].reshape(g.shape[:-1] + (n, n))
        g[..., o:o + n * n] = (0.5 * (b + np.swapaxes(b, -1, -2))).reshape(g.shape[:-1] + (n * n,))
    return g


def differences(P, x0, p):
    """(d w* / d p[COST] [nw, 80], dV / d p[COST] [80]) by extrapolated central differences, all solves in one call; None where one of
    them is not solved."""
    xs, ps = [], []
    for h in (2e-4, 1e-4):
        for sgn in (1.0, -1.0):
            for j in COST:
                pv = p.copy()
                pv[j] += sgn * h
                xs.append(x0), ps.append(pv)
    r = cpu_port.solve(P, np.array(xs), p=np.array(ps), flags=0, tol=TOL, exact=True, nthreads=1)
    if (r.status != 0).any():
        return None
    w, V = w_of(r).reshape(2, 2, len(COST), -1), r.V.reshape(2, 2, len(COST))
    d_w = [(w[i, 0] - w[i, 1]) / (2 * h) for i, h in enumerate((2e-4, 1e-4))]
    d_V = [(V[i, 0] - V[i, 1]) / (2 * h) for i, h in enumerate((2e-4, 1e-4))]
    return ((4 * d_w[1] - d_w[0]) / 3).T, (4 * d_V[1] - d_V[0]) / 3


def instance(job):
    """The stored record of one instance, or a string saying why it does not enter."""
    N, x0, p, seed = job      # (a problem holds closures: the worker builds its own)
    torch.set_num_threads(1)
    P = bounded("cartpole", N)
    nx, nu = P.nx, P.nu
    r = cpu_port.solve(P, x0[None], p=p[None], flags=0, tol=TOL, exact=True, nthreads=1)
    if r.status[0] != 0 or cpu_port.solve(P, x0[None], p=p[None], flags=0, tol=1e-9, nthreads=1).status[0] != 0:
        return "unsolved"
    c = classify(P, r.BND[0])
    if c is None:
        return "unclear"
    flags, soft, act = c
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0], p=p, u0fix=None)
    mr = nlp_mirror.evaluate(parameterised(P), sol, x0, p=p, u0fix=None)
    nw = N * nu + (N + 1) * nx
    J = np.linalg.solve(mr.dR_dz, -mr.dR_dp)[:nw]
    G = np.random.default_rng(seed).standard_normal((R, nw))
    G[R - 1] = 0.0
    G[R - 1, 0] = 1.0
    g_cost, dV = np.zeros((R, NP)), np.zeros(NP)
    g_cost[:, COST], dV[COST] = (G @ J)[:, COST], mr.dL_dp[0, COST]
    fd = differences(P, x0, p)
    if fd is None:
        return "difference unsolved"
    agree, agree_V = scaled(g_cost[:, COST], G @ fd[0]), scaled(dV[COST], fd[1])
    if not max(agree, agree_V) <= GATE:
        return f"gate {agree:.1e} {agree_V:.1e}"
    return dict(x0=x0, p=p, G=G, g_cost=symmetrised(g_cost), dV_dcost=symmetrised(dV), dpi_dp=mr.dpi_dp[:, :NDYN], act_lb=act[0],
                act_ub=act[1], agree=agree, agree_V=agree_V, **flags)


def store(fx, tag, N, got):
    for k in KEYS:
        fx[tag + k] = np.stack([np.asarray(o[k]) for o in got])
    for k, v in groups(bounded("cartpole", N)).items():
        fx[tag + k] = v
    big = max(np.abs(o["g_cost"][:R - 1]).max() for o in got)
    print(f"{tag}: {len(got)} instances, per class {{{', '.join(f'{c}: {int(fx[tag + c].sum())}' for c in CLASSES)}}}, "
          f"agreement w {fx[tag + 'agree'].max():.1e} V {fx[tag + 'agree_V'].max():.1e}, largest |g_cost| on a normal cotangent {big:.2e}",
          flush=True)


def set_a(pool, g13, N, fx):
    P = bounded("cartpole", N)
    x0 = g13[f"cartpole_N{N}_x0"]
    res = pool.map(instance, [(N, x0[i], P.p0.copy(), [14000, N, i]) for i in range(len(x0))], chunksize=1)
    got = [o for o in res if isinstance(o, dict)]
    print(f"A N {N}: {len(got)} of G13's {len(x0)} instances pass; turned away: {[o for o in res if not isinstance(o, dict)]}", flush=True)
    if len(got) < REQUIRED_A:
        raise SystemExit(f"set A, N {N}: only {len(got)} of G13's instances pass the gate")
    for i, o in enumerate(res):      # the classes are G13's own
        if isinstance(o, dict):
            assert all(bool(o[c]) == bool(g13[f"cartpole_N{N}_{c}"][i]) for c in CLASSES)
    if N in ACT_X_AT and not any(o["act_x"] for o in got):
        raise SystemExit(f"set A, N {N}: no instance with an active hard state row passes the gate")
    store(fx, f"A_N{N}_", N, got)


def set_b(pool, N, fx):
    P = bounded("cartpole", N)
    rng = np.random.default_rng([SEED_B, N])
    x0 = rng.uniform(-1.0, 1.0, (DRAWS_B, 4)) * X0_SCALE
    p = np.stack([perturbed_p(P.p0, rng) for _ in range(DRAWS_B)])
    # the candidates' KKT points, all in one call each: which are solved (in both modes), clear, and on an active control row
    r, rd = cpu_port.solve(P, x0, p=p, flags=0, tol=TOL, exact=True), cpu_port.solve(P, x0, p=p, flags=0, tol=1e-9)
    cls = [classify(P, r.BND[i]) if r.status[i] == 0 and rd.status[i] == 0 else None for i in range(DRAWS_B)]
    on_u = [c is not None and bool(c[0]["act_u"] or c[0]["act_u0"]) for c in cls]
    unsolved = int(((r.status != 0) | (rd.status != 0)).sum())
    active = lambda o: bool(o["act_u"] or o["act_u0"])      # noqa: E731
    got, why, tried = {}, [], set()
    while True:      # rounds, in draw order: the active ones still missing first, then whatever fills the set
        left = [i for i in range(DRAWS_B) if cls[i] is not None and i not in tried]
        need_active = max(0, ACTIVE_B - sum(map(active, got.values())))
        pick = [i for i in left if on_u[i]][:need_active]
        pick += [i for i in left if i not in pick][:max(0, PER_B - len(got) - len(pick))]
        if not pick:
            break
        res = pool.map(instance, [(N, x0[i], p[i], [14200, N, i]) for i in sorted(pick)], chunksize=1)
        got.update({i: o for i, o in zip(sorted(pick), res) if isinstance(o, dict)})
        why += [f"{i}: {o}" for i, o in zip(sorted(pick), res) if not isinstance(o, dict)]
        tried.update(pick)
    got = [got[i] for i in sorted(got)]
    print(f"B N {N}: of {DRAWS_B} draws {unsolved} not solved, {sum(c is None for c in cls) - unsolved} unclear, "
          f"{sum(on_u)} solved ones on an active control row; gate run on {len(tried)}, turned away {why}", flush=True)
    if len(got) < REQUIRED_B or not any(map(active, got)):
        raise SystemExit(f"set B, N {N}: {len(got)} instances pass the gate, {sum(map(active, got))} with an active control row")
    store(fx, f"B_N{N}_", N, got)


def main():
    g13 = np.load(os.path.join(HERE, "g13_bound_vjp.npz"))
    fx = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for N in HORIZONS_A:
            set_a(pool, g13, N, fx)
        for N in HORIZONS_B:
            set_b(pool, N, fx)
    fx["tol"], fx["gate"] = np.array(TOL), np.array(GATE)
    out = os.path.join(HERE, "g14_cost_vjp.npz")
    np.savez_compressed(out, **fx)
    print("wrote g14_cost_vjp.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
