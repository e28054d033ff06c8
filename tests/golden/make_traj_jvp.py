"""G15 — Jacobian-vector products of the whole planned trajectory w* = [u_0 .. u_{N-1}; x_0 .. x_N] of the cartpole and the
linear-system OCP along directions in x0 and in p, from the mirror of the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.
Writes tests/golden/g15_traj_jvp.npz.  CPU only:

    python tests/golden/make_traj_jvp.py          (about five minutes on eight cores)

Instances: exactly those of G11 (g11_traj_vjp.npz: same x0, cls, soft and horizons; ``idx`` holds the row of G11 an instance came
from) and its per-instance-theta set.  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``nlp_mirror.evaluate`` on it (``solution_from_iterate``);
  3. J_p = solve(dR_dz, -dR_dp)[:nw] and J_x = solve(dR_dz, -E)[:nw], E = dR/dx0 as make_traj_vjp.py builds it — the two dense
     solves G11 contracted with its cotangents, so that <G, dW> of this file equals g_x0 . vx + g_theta . vp of that one;
  4. R = 3 directions (vx [nx], vp [np]): standard-normal draws on x0 and on the entries of p the sensitivity pass differentiates
     (DIFF_P; the rest of vp is 0), then direction 1 with vx = 0 (theta only) and direction 2 with vp = 0 (x0 only); the reference
     dW = vx J_x' + vp J_p', stored split into dU [R, N, nu] and dX [R, N + 1, nx].
Gate: G11's, 1e-7 with rows scaled by max(|row|, 1), against *directional* central differences of the port's whole (U, X) along
(vx[r], vp[r]) at h = 2e-4 and 1e-4, extrapolated (4 d(h/2) - d(h)) / 3: twelve solves an instance.  Where a soft slack is positive
the mirror holds the slacks constant (quirk q1): it is the definition, the instance is kept, marked ``soft`` and not compared
(``agree`` NaN).  Other instances above the gate are dropped.
The generator fails rather than deliver fewer than REQUIRED instances of class 0 (interior) and class 1 (a control bound active at
a stage >= 1) per (model, N), counted as G11 counts them; none of class 0 at the linear system's N = 31, 32 and 63, where G11 has
none (see make_traj_vjp.py); and both instances of each per-instance-theta set.

What the recipe gives: 96 of the 99 compared instances pass (92 of 95 at the nominal parameters, the 4 with a theta of their own),
the largest passing value 9.8e-8.  Dropped are cartpole N 15 row 9
(class 1, 1.08e-7) and linear N 20 rows 2 and 3 (class 0, 1.88e-7 and 1.12e-7): the differences' own error at these step sizes.
That leaves 3 class-1 instances at cartpole N 15 and 2 class-0 instances at linear N 20, the required counts with nothing to spare.
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
from oracle.problems import make_cartpole, make_linear_system  # noqa: E402

TOL, GATE, GAMMA, R = 1e-10, 1e-7, 0.99, 3
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
DIFF_P = {"cartpole": np.arange(3), "linear": np.arange(12)}      # m, M, l (the mirror's cost has no parameters); A, B, b, V_0, f
REQUIRED = {0: 2, 1: 3}      # class -> instances per (model, N), at least
REQUIRED_AT = {("linear", N): {0: 0} for N in (31, 32, 63)}      # (model, N) -> {class: count} where G11 has none of a class
TH_N = 20                    # per-instance theta: G11's two instances at N = 20, both required


def problem(model, N):
    return make_cartpole(N=N, tf=0.1 * N) if model == "cartpole" else make_linear_system(gamma=GAMMA, N=N)


def scaled(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)).max())


def w_of(r):
    """[B, nw] in the mirror's order."""
    return np.concatenate([r.U.reshape(len(r.U), -1), r.X.reshape(len(r.X), -1)], 1)


def differences(P, x0, p, vx, vp):
    """d w* along (vx[r], vp[r]) [R, nw] by extrapolated central differences, all solves in one call; None where one of them is
    not solved."""
    xs, ps = [], []
    for h in (2e-4, 1e-4):
        for sgn in (1.0, -1.0):
            for r in range(len(vx)):
                xs.append(x0 + sgn * h * vx[r]), ps.append(p + sgn * h * vp[r])
    r = cpu_port.solve(P, np.array(xs), p=np.array(ps), flags=0, tol=TOL, exact=True, nthreads=1)
    if (r.status != 0).any():
        return None
    w = w_of(r).reshape(2, 2, len(vx), -1)
    d = [(w[i, 0] - w[i, 1]) / (2 * h) for i, h in enumerate((2e-4, 1e-4))]
    return (4 * d[1] - d[0]) / 3


def instance(job):
    model, N, x0, p, soft, seed = job
    torch.set_num_threads(1)
    P = problem(model, N)
    nx, nu = P.nx, P.nu
    pv = P.p0.copy() if p is None else p
    r = cpu_port.solve(P, x0[None], p=None if p is None else p[None], flags=0, tol=TOL, exact=True, nthreads=1)
    if r.status[0] != 0:
        return None
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0], p=p, u0fix=None)
    mr = nlp_mirror.evaluate(P, sol, x0, p=p, u0fix=None)
    nw = N * nu + (N + 1) * nx
    E = np.zeros((mr.dR_dz.shape[0], nx))
    for i, (k, kind, idx, sgn, bnd, sv) in enumerate(nlp_mirror.mirror_rows(P)):
        if bnd in ("lbx0", "ubx0"):
            E[nw + N * nx + i, idx] = -sgn
    Jp = np.linalg.solve(mr.dR_dz, -mr.dR_dp)[:nw]
    Jx = np.linalg.solve(mr.dR_dz, -E)[:nw]
    rng = np.random.default_rng(seed)
    dp = DIFF_P[model]
    vx = rng.standard_normal((R, nx))
    vp = np.zeros((R, len(pv)))
    vp[:, dp] = rng.standard_normal((R, len(dp)))
    vx[1] = 0.0
    vp[2] = 0.0
    dW = vx @ Jx.T + vp @ Jp.T
    out = dict(x0=x0, vx=vx, vp=vp, dU=dW[:, :N * nu].reshape(R, N, nu), dX=dW[:, N * nu:].reshape(R, N + 1, nx), soft=soft,
               agree=np.nan)
    if not soft:
        fd = differences(P, x0, pv, vx, vp)
        if fd is None:
            return None
        out["agree"] = scaled(dW, fd)
        if not out["agree"] <= GATE:
            print(f"  dropped: {model} N {N} seed {seed}: agreement {out['agree']:.2e}", flush=True)
            return None
    return out


def stack(out, keys):
    return {k: np.stack([np.asarray(o[k]) for o in out]) for k in keys}


KEYS = ("x0", "vx", "vp", "dX", "dU", "agree")


def compute(models=tuple(HORIZONS), procs=8):
    g11 = np.load(os.path.join(HERE, "g11_traj_vjp.npz"))
    fx = {}
    with Pool(min(procs, os.cpu_count() or 1)) as pool:
        for model, horizons in ((m, HORIZONS[m]) for m in models):
            for N in horizons:
                key = f"{model}_N{N}_"
                x0, soft = g11[key + "x0"], g11[key + "soft"]
                res = pool.map(instance, [(model, N, x0[i], None, bool(soft[i]), [15000 + N, i]) for i in range(len(x0))], chunksize=1)
                idx = [i for i, o in enumerate(res) if o is not None]
                for k, v in stack([res[i] for i in idx], KEYS + ("soft",)).items():
                    fx[key + k] = v
                fx[key + "idx"], fx[key + "cls"] = np.array(idx), g11[key + "cls"][idx]
                worst = fx[key + "agree"][~fx[key + "soft"]].max(initial=0.0)      # (0 where every instance has a positive slack)
                print(f"{model} N {N}: {len(idx)} of {len(x0)} instances, per class {np.bincount(fx[key + 'cls'], minlength=4).tolist()}, "
                      f"{int(fx[key + 'soft'].sum())} soft, agreement {worst:.1e}", flush=True)
            key = f"{model}_th_"
            x0, th = g11[key + "x0"], g11[key + "theta"]
            res = pool.map(instance, [(model, TH_N, x0[i], th[i], False, [15900, i]) for i in range(len(x0))], chunksize=1)
            idx = [i for i, o in enumerate(res) if o is not None]
            if len(idx) < len(x0):
                raise SystemExit(f"{model} per-instance theta: only {len(idx)} of G11's {len(x0)} instances pass the gate")
            for k, v in stack([res[i] for i in idx], KEYS).items():
                fx[key + k] = v
            fx[key + "theta"], fx[key + "idx"] = th[idx], np.array(idx)
            print(f"{model} per-instance theta: {len(idx)} of {len(x0)} instances, agreement {fx[key + 'agree'].tolist()}", flush=True)
    fx["gamma"], fx["tol"], fx["gate"] = np.array(GAMMA), np.array(TOL), np.array(GATE)
    return fx


def shortfalls(fx):
    out = []
    for model, horizons in HORIZONS.items():
        for N in horizons:
            cls = fx[f"{model}_N{N}_cls"]
            for c, need in {**REQUIRED, **REQUIRED_AT.get((model, N), {})}.items():
                have = int((cls == c).sum())      # (counted as G11 counts them: a class-1 instance with a positive slack is one)
                if have < need:
                    out.append(f"{model} N {N}: {have} of {need} instances of class {c} in the fixture")
    return out


def main():
    fx = compute()
    short = shortfalls(fx)
    if short:
        raise SystemExit("\n".join(short))
    np.savez_compressed(os.path.join(HERE, "g15_traj_jvp.npz"), **fx)
    print("wrote g15_traj_jvp.npz:", os.path.getsize(os.path.join(HERE, "g15_traj_jvp.npz")), "bytes")


if __name__ == "__main__":
    main()
