"""G16 — Jacobian-vector products of the whole planned trajectory w* = [u_0 .. u_{N-1}; x_0 .. x_N] of the chain-of-masses OCP along
directions in x0 and in p, from the mirror of the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.  Writes
tests/golden/g16_chain_traj_jvp.npz.  CPU only:

    python tests/golden/make_chain_traj_jvp.py          (a few minutes on eight cores, about 36 s per instance at n_mass 7)

The recipe is the one of make_traj_jvp.py (G15), on the instances of G12 (g12_chain_traj_vjp.npz: the x0 of its nine sets; ``idx``
holds the row of G12 an instance is).  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``solution_from_iterate`` and ``nlp_mirror.evaluate`` on it;
  3. J_p = solve(dR_dz, -dR_dp)[:nw] and J_x = solve(dR_dz, -E)[:nw], E = dR/dx0 from the lbx0 / ubx0 rows — the two dense solves
     G12 contracted with its cotangents, so that <G, dW> of this file equals g_x0 . vx + g_theta . vp of that one;
  4. R = 3 directions from rng = default_rng(seed): vx = standard_normal((R, nx)), then vp = standard_normal((R, n_p)) over EVERY
     entry of p (m, D, L, C, Q, R, w); direction 1 moves the dynamics block and w only (vp[1] zero on Q and R, vx[1] = 0), direction
     2 moves x0 only (vp[2] = 0);
  5. the reference dW = vx J_x' + vp J_p', stored split into dU [R, N, nu] and dX [R, N + 1, nx].
Gate 1e-6 (G12's), per direction over the whole of dW scaled by max(|dW[r]|_inf, 1), against *directional* central differences of the
port's whole (U, X) along (vx[r], vp[r]) at h = 2e-4 and 1e-4, extrapolated (4 d(h/2) - d(h)) / 3: twelve solves an instance.
Seed of instance i of a set: [16000 + 100 n_mass + N, i] for the first draw, the same list with d appended for redraw d = 1, 2
(DRAWS = 3; ``draw``: which one entered).  The KKT point and the Jacobians are the same for every draw.

The generator fails rather than deliver less than: all four instances of each of the eight G10-derived sets, and at least three of
the four of m3_N10_act (x0 next to an active-set change there: a direction that moves x0 can cross it inside the difference step).
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

TOL, GATE, B, R, DRAWS = 1e-10, 1e-6, 4, 3, 3
SETS = ((3, 1, "ss"), (3, 2, "ss"), (3, 10, "ss"), (3, 10, "x0"), (4, 3, "ss"), (5, 8, "ss"), (6, 3, "ss"), (7, 5, "ss"), (3, 10, "act"))
REQUIRED = {"act": 3}      # base -> instances that must pass (every other set: all B)
KEYS = ("x0", "vx", "vp", "dX", "dU", "agree", "draw")


def set_name(n_mass, N, base):
    return f"m{n_mass}_N{N}_{base}_"


def scaled(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)).max())


def w_of(r):
    """[B, nw] in the mirror's order."""
    return np.concatenate([r.U.reshape(len(r.U), -1), r.X.reshape(len(r.X), -1)], 1)


def differences(P, x0, vx, vp):
    """d w* along (vx[r], vp[r]) [R, nw] by extrapolated central differences, all solves in one call; None where one of them is
    not solved."""
    xs, ps = [], []
    for h in (2e-4, 1e-4):
        for sgn in (1.0, -1.0):
            for r in range(len(vx)):
                xs.append(x0 + sgn * h * vx[r]), ps.append(P.p0 + sgn * h * vp[r])
    r = cpu_port.solve(P, np.array(xs), p=np.array(ps), flags=0, tol=TOL, exact=True, nthreads=1)
    if (r.status != 0).any():
        return None
    w = w_of(r).reshape(2, 2, len(vx), -1)
    d = [(w[i, 0] - w[i, 1]) / (2 * h) for i, h in enumerate((2e-4, 1e-4))]
    return (4 * d[1] - d[0]) / 3


def instance(job):
    n_mass, N, x0, seed = job
    torch.set_num_threads(1)
    P = make_chain_mass(n_mass=n_mass, N=N)
    nx, nu, n_p = P.nx, P.nu, len(P.p0)
    r = cpu_port.solve(P, x0[None], flags=0, tol=TOL, exact=True, nthreads=1)
    if r.status[0] != 0:
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
    off_q = 10 * (n_mass - 1)
    worst = []
    for draw in range(DRAWS):
        rng = np.random.default_rng(list(seed) + ([draw] if draw else []))
        vx = rng.standard_normal((R, nx))
        vp = rng.standard_normal((R, n_p))
        vp[1, off_q:off_q + nx * nx + nu * nu] = 0.0
        vx[1] = 0.0
        vp[2] = 0.0
        dW = vx @ Jx.T + vp @ Jp.T
        fd = differences(P, x0, vx, vp)
        if fd is None:
            continue
        agree = scaled(dW, fd)
        worst.append(agree)
        if agree <= GATE:
            return dict(x0=x0, vx=vx, vp=vp, dU=dW[:, :N * nu].reshape(R, N, nu), dX=dW[:, N * nu:].reshape(R, N + 1, nx), agree=agree,
                        draw=draw)
    print(f"  dropped: n_mass {n_mass} N {N} seed {seed}: agreement {worst}", flush=True)
    return None


def main():
    g12 = np.load(os.path.join(HERE, "g12_chain_traj_vjp.npz"))
    fx = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        jobs = []
        for n_mass, N, base in SETS:
            x0 = g12[set_name(n_mass, N, base) + "x0"]
            jobs += [(n_mass, N, x0[i], [16000 + 100 * n_mass + N, i]) for i in range(B)]
        res = pool.map(instance, jobs, chunksize=1)
    for s, (n_mass, N, base) in enumerate(SETS):
        tag, got = set_name(n_mass, N, base), res[B * s:B * (s + 1)]
        idx = [i for i, o in enumerate(got) if o is not None]
        if len(idx) < REQUIRED.get(base, B):
            raise SystemExit(f"{tag}: only instances {idx} of G12 pass the gate, {REQUIRED.get(base, B)} are required")
        for k in KEYS:
            fx[tag + k] = np.stack([np.asarray(got[i][k]) for i in idx])
        fx[tag + "idx"] = np.array(idx)
        print(f"{tag}: instances {idx}, agreement {fx[tag + 'agree'].max():.1e}, draws {fx[tag + 'draw'].tolist()}", flush=True)
    fx["tol"], fx["gate"] = np.array(TOL), np.array(GATE)
    out = os.path.join(HERE, "g16_chain_traj_jvp.npz")
    np.savez_compressed(out, **fx)
    print("wrote g16_chain_traj_jvp.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
