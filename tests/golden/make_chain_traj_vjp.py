"""G12 — vector-Jacobian products of the whole planned trajectory w* = [u_0 .. u_{N-1}; x_0 .. x_N] of the chain-of-masses OCP with
respect to x0 and to p, from the mirror of the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.  Writes
tests/golden/g12_chain_traj_vjp.npz.  CPU only:

    python tests/golden/make_chain_traj_vjp.py          (several minutes on eight cores)

The recipe is the one of make_traj_vjp.py (G11), on the chain.  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``solution_from_iterate`` and ``nlp_mirror.evaluate`` on it;
  3. J_p = solve(dR_dz, -dR_dp)[:nw] and J_x = solve(dR_dz, -E)[:nw], E = dR/dx0 from the lbx0 / ubx0 rows — the two calls G10 made
     (its dpi_dp and dpi_dx0 are their first nu rows), so that the unit cotangent on u_0 reproduces G10;
  4. R = 3 cotangents G on w: two standard-normal draws over all of w (x_0 included) and the unit cotangent on component 0 of u_0;
     the references g_theta = G J_p and g_x0 = G J_x.
Gate 1e-6 (G10's gate, RTOL of tests/small_mode_cases.py): central differences of the port's whole (U, X) over x0 and over DIFF_P —
a fixed subset of p with entries of every block m, D, L, C, Q, R (and w) — at h = 2e-4 and 1e-4, extrapolated (4 f(h/2) - f(h)) / 3;
G J and G . differences must agree, rows scaled by max(|row|, 1).  An instance also enters only if the port's default mode (the
product's twin) solves it at tol 1e-9.  The differences carry the solves' own noise, tol / h = 1e-6 per entry of w at worst, and a
standard-normal cotangent sums it over all of w: measured 2e-7 .. 1e-6 here, so a draw of G can miss the gate on an instance whose
Jacobians are right.  The two normal cotangents of an instance are therefore drawn up to DRAWS = 3 times (``draw``: which one
entered); the KKT point, the Jacobians, the differences and the gate are the same for every draw.

Sets, four instances each.
  * The eight sets of G10 on G10's own x0 (``idx``: the row of G10 an instance is; all four must pass).
  * m3_N10_act: n_mass 3, N 10, x0 = x0_default + N(0, 0.2): every instance has at least one control row active (slack < 1e-8) at a
    stage >= 1 and no control row with a slack between 1e-8 and 1e-6 (``active`` [B, N, nu] marks the rows) — the only place a
    barrier term meets a non-zero right-hand side inside the adjoint sweep; none of G10's instances has such a row.
The generator fails rather than deliver a short set.  Also stored per set: ``agree`` [B] and ``nb_theta`` / ``nb_x0`` [B], the scaled
distance of each instance's g_theta / g_x0 from the next instance's (the negative control of the GPU test).
"""
import os
import sys
from multiprocessing import Pool

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import cpu_port, nlp_mirror  # noqa: E402
from oracle.from_iterate import solution_from_iterate  # noqa: E402
from oracle.problems import make_chain_mass  # noqa: E402

TOL, GATE, ACTIVE, SIGMA_ACT, B, R, DRAWS = 1e-10, 1e-6, 1e-8, 0.2, 4, 3, 3
G10_SETS = ((3, 1, "ss"), (3, 2, "ss"), (3, 10, "ss"), (3, 10, "x0"), (4, 3, "ss"), (5, 8, "ss"), (6, 3, "ss"), (7, 5, "ss"))
ACT_SET = (3, 10, "act")
KEYS = ("x0", "G", "g_theta", "g_x0", "agree", "active", "draw")


def set_name(n_mass, N, base):
    return f"m{n_mass}_N{N}_{base}_"


def diff_p(n_mass):
    """Entries of p the differences run over: m_0, D_0[0], L_0[1], C_0[2], Q[0, 0], Q[nx-1, nx-1], R[0, 0], R[1, 1], w[0]."""
    nl, nx, nu = n_mass - 1, (2 * (n_mass - 2) + 1) * 3, 3
    off_q = 10 * nl
    off_r = off_q + nx * nx
    return np.array([0, nl, 4 * nl + 1, 7 * nl + 2, off_q, off_q + nx * nx - 1, off_r, off_r + nu + 1, off_r + nu * nu])


def scaled(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)).max())


def w_of(r):
    """[B, nw] in the mirror's order."""
    return np.concatenate([r.U.reshape(len(r.U), -1), r.X.reshape(len(r.X), -1)], 1)


def differences(P, x0, dp):
    """d w* / d [x0; p[dp]] [nw, nx + len(dp)] by extrapolated central differences, all solves in one call; None where one of them
    is not solved."""
    nx = P.nx
    nz = nx + len(dp)
    xs, ps = [], []
    for h in (2e-4, 1e-4):
        for sgn in (1.0, -1.0):
            for j in range(nz):
                xv, pv = x0.copy(), P.p0.copy()
                if j < nx:
                    xv[j] += sgn * h
                else:
                    pv[dp[j - nx]] += sgn * h
                xs.append(xv), ps.append(pv)
    r = cpu_port.solve(P, np.array(xs), p=np.array(ps), flags=0, tol=TOL, exact=True, nthreads=1)
    if (r.status != 0).any():
        return None
    w = w_of(r).reshape(2, 2, nz, -1)
    d = [(w[i, 0] - w[i, 1]) / (2 * h) for i, h in enumerate((2e-4, 1e-4))]
    return ((4 * d[1] - d[0]) / 3).T


def instance(job):
    n_mass, N, x0, seed = job
    torch.set_num_threads(1)
    P = make_chain_mass(n_mass=n_mass, N=N)
    nx, nu = P.nx, P.nu
    r = cpu_port.solve(P, x0[None], flags=0, tol=TOL, exact=True, nthreads=1)
    if r.status[0] != 0 or cpu_port.solve(P, x0[None], flags=0, tol=1e-9, nthreads=1).status[0] != 0:
        return None
    tu = np.minimum(r.BND[0, 2, :N, :nu], r.BND[0, 3, :N, :nu])      # slacks of the control rows [N, nu]
    if not ((tu < ACTIVE) | (tu > 1e-6)).all():                      # (nothing in between: a row is active or clearly not)
        return None
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0])
    mr = nlp_mirror.evaluate(P, sol, x0)
    nw = N * nu + (N + 1) * nx
    E = np.zeros((mr.dR_dz.shape[0], nx))
    for i, (k, kind, idx, sgn, bnd, sv) in enumerate(nlp_mirror.mirror_rows(P)):
        if bnd in ("lbx0", "ubx0"):
            E[nw + N * nx + i, idx] = -sgn
    Jp = np.linalg.solve(mr.dR_dz, -mr.dR_dp)[:nw]
    Jx = np.linalg.solve(mr.dR_dz, -E)[:nw]
    dp = diff_p(n_mass)
    fd = differences(P, x0, dp)
    if fd is None:
        return None
    for draw in range(DRAWS):
        G = np.random.default_rng(list(seed) + [draw]).standard_normal((R, nw))
        G[R - 1] = 0.0
        G[R - 1, 0] = 1.0
        out = dict(x0=x0, G=G, g_theta=G @ Jp, g_x0=G @ Jx, active=tu < ACTIVE, draw=draw)
        out["agree"] = max(scaled(out["g_x0"], G @ fd[:, :nx]), scaled(out["g_theta"][:, dp], G @ fd[:, nx:]))
        if out["agree"] <= GATE:
            return out
    return None


def finish(fx, tag, got):
    for k in KEYS:
        fx[tag + k] = np.stack([np.asarray(o[k]) for o in got])
    for k in ("g_theta", "g_x0"):
        v = fx[tag + k]
        fx[tag + "nb_" + k[2:]] = np.array([scaled(v[i], v[(i + 1) % len(v)]) for i in range(len(v))])
    print(f"{tag}: agreement {fx[tag + 'agree'].max():.1e}, active rows at stages >= 1 {fx[tag + 'active'][:, 1:].sum((1, 2)).tolist()}, "
          f"neighbours theta {fx[tag + 'nb_theta'].min():.1e} x0 {fx[tag + 'nb_x0'].min():.1e}", flush=True)


def main():
    g10 = np.load(os.path.join(HERE, "g10_chain_state_sens.npz"))
    fx = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        jobs = []
        for n_mass, N, base in G10_SETS:
            x0 = g10[set_name(n_mass, N, base) + "x0"]
            jobs += [(n_mass, N, x0[i], [12000 + 100 * n_mass + N + (base == "x0"), i]) for i in range(B)]
        res = pool.map(instance, jobs, chunksize=1)
        for s, (n_mass, N, base) in enumerate(G10_SETS):
            tag, got = set_name(n_mass, N, base), res[B * s:B * (s + 1)]
            if any(o is None for o in got):
                raise SystemExit(f"{tag}: instances {[i for i, o in enumerate(got) if o is None]} of G10 do not pass the gate")
            finish(fx, tag, got)
            fx[tag + "idx"] = np.arange(B)
            unit = max(scaled(fx[tag + "g_theta"][:, R - 1], g10[tag + "dpi_dp"][:, 0]), scaled(fx[tag + "g_x0"][:, R - 1], g10[tag + "dpi_dx0"][:, 0]))
            if not unit <= 1e-12:
                raise SystemExit(f"{tag}: the unit cotangent is {unit:.1e} from G10")
        n_mass, N, base = ACT_SET
        P = make_chain_mass(n_mass=n_mass, N=N)
        rng = np.random.default_rng(12020)
        tag, got = set_name(n_mass, N, base), []
        for draw in range(3):
            x0 = P.x0_default + rng.normal(0.0, SIGMA_ACT, (2 * B, P.nx))
            got += [o for o in pool.map(instance, [(n_mass, N, x, [12900, draw, i]) for i, x in enumerate(x0)], chunksize=1)
                    if o is not None and o["active"][1:].any()]
            if len(got) >= B:
                break
        if len(got) < B:
            raise SystemExit(f"{tag}: only {len(got)} of {B} instances with an active control row at a stage >= 1 pass the gate")
        finish(fx, tag, got[:B])
    fx["tol"], fx["gate"], fx["sigma_act"] = np.array(TOL), np.array(GATE), np.array(SIGMA_ACT)
    for n_mass in sorted({s[0] for s in G10_SETS}):
        fx[f"diff_p_m{n_mass}"] = diff_p(n_mass)
    out = os.path.join(HERE, "g12_chain_traj_vjp.npz")
    np.savez_compressed(out, **fx)
    print("wrote g12_chain_traj_vjp.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
