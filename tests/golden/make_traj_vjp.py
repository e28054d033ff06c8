"""G11 — vector-Jacobian products of the whole planned trajectory w* = [u_0 .. u_{N-1}; x_0 .. x_N] of the cartpole and the
linear-system OCP with respect to x0 and to p, from the mirror of the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.
Writes tests/golden/g11_traj_vjp.npz.  CPU only:

    python tests/golden/make_traj_vjp.py          (about ten minutes on eight cores)

Instances: those of G9 (g9_state_sens.npz: same x0, cls, soft and horizons; ``idx`` holds the row of G9 an instance came from) and
its per-instance-theta set.  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``nlp_mirror.evaluate`` on it (``solution_from_iterate``);
  3. J_p = solve(dR_dz, -dR_dp)[:nw] and J_x = solve(dR_dz, -E)[:nw], E = dR/dx0 built as make_state_sens.py builds it — the two
     calls G9 made (its dpi_dp and dpi_dx0_mirror are their first nu rows), so that the unit cotangent on u_0 reproduces G9;
  4. R = 3 cotangents G on w: two standard-normal draws over all of w (x_0 included) and the unit cotangent on component 0 of u_0;
     the references g_theta = G J_p and g_x0 = G J_x.
Gate: central differences of the port's whole (U, X) over x0 and over the entries of p the sensitivity pass differentiates (DIFF_P)
at h = 2e-4 and 1e-4, extrapolated (4 f(h/2) - f(h)) / 3.  An instance without a positive slack enters only if G J and
G . differences agree to 1e-7, rows scaled by max(|row|, 1).  Where a soft slack is positive the mirror holds the slacks constant
(quirk q1): it is the definition, the instance is kept, marked ``soft`` and not compared (``agree`` NaN).
The generator fails rather than deliver fewer than REQUIRED instances of class 0 (interior) and class 1 (a control bound active at
a stage >= 1) per (model, N); the classes are G9's, counted as G9 counts them (a class-1 instance with a positive slack is one).

Lowered counts (REQUIRED_AT), the gate left as it is.  Linear system, N = 31, 32 and 63: no interior instance of G9 passes, so the
fixture holds instances with a positive slack only there and nothing at these horizons is compared with differences.  The nominal
parameters put the equilibrium x = 0 exactly on the softened bound lbx = 0, and by stage ~30 the plan has converged onto it: the
differences over b and f (and, less, A and B) straddle the kink where that bound row switches (0.02 ... 0.4 off the mirror at
h = 1e-4, against 2e-10 ... 4e-8 at N <= 20), and several perturbed solves stop at a residual of 1.3e-10 ... 2e-10, short of
tol 1e-10.  du0*/dx0 alone (G9) does not see the tail.  Per-instance theta: two of G9's three instances pass for each model (TH_MIN).
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
REQUIRED = {0: 4, 1: 3}      # class -> instances per (model, N), at least
REQUIRED_AT = {("linear", N): {0: 0} for N in (31, 32, 63)}      # (model, N) -> {class: count} where a horizon cannot reach REQUIRED
TH_N, TH_MIN = 20, 2         # per-instance theta: G9's three instances at N = 20, of which at least TH_MIN must pass


def problem(model, N):
    return make_cartpole(N=N, tf=0.1 * N) if model == "cartpole" else make_linear_system(gamma=GAMMA, N=N)


def scaled(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)).max())


def w_of(r):
    """[B, nw] in the mirror's order."""
    return np.concatenate([r.U.reshape(len(r.U), -1), r.X.reshape(len(r.X), -1)], 1)


def differences(P, model, x0, p):
    """d w* / d [x0; p[DIFF_P]] [nw, nx + len(DIFF_P)] by extrapolated central differences, all solves in one call; None where one
    of them is not solved."""
    nx, dp = P.nx, DIFF_P[model]
    nz = nx + len(dp)
    xs, ps = [], []
    for h in (2e-4, 1e-4):
        for sgn in (1.0, -1.0):
            for j in range(nz):
                xv, pv = x0.copy(), p.copy()
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
    G = np.random.default_rng(seed).standard_normal((R, nw))
    G[R - 1] = 0.0
    G[R - 1, 0] = 1.0
    out = dict(x0=x0, G=G, g_theta=G @ Jp, g_x0=G @ Jx, soft=soft, agree=np.nan)
    if not soft:
        fd = differences(P, model, x0, pv)
        if fd is None:
            return None
        dp = DIFF_P[model]
        out["agree"] = max(scaled(out["g_x0"], G @ fd[:, :nx]), scaled(out["g_theta"][:, dp], G @ fd[:, nx:]))
        if not out["agree"] <= GATE:
            return None
    return out


def stack(out, keys):
    return {k: np.stack([np.asarray(o[k]) for o in out]) for k in keys}


def compute(models=tuple(HORIZONS), procs=8):
    g9 = np.load(os.path.join(HERE, "g9_state_sens.npz"))
    fx = {}
    with Pool(min(procs, os.cpu_count() or 1)) as pool:
        for model, horizons in ((m, HORIZONS[m]) for m in models):
            for N in horizons:
                key = f"{model}_N{N}_"
                x0, soft = g9[key + "x0"], g9[key + "soft"]
                seed0 = 11000 + 1000 * (model == "linear") + 10 * N
                res = pool.map(instance, [(model, N, x0[i], None, bool(soft[i]), [seed0, i]) for i in range(len(x0))], chunksize=1)
                idx = [i for i, o in enumerate(res) if o is not None]
                for k, v in stack([res[i] for i in idx], ("x0", "G", "g_theta", "g_x0", "soft", "agree")).items():
                    fx[key + k] = v
                fx[key + "idx"], fx[key + "cls"] = np.array(idx), g9[key + "cls"][idx]
                print(f"{model} N {N}: {len(idx)} of {len(x0)} instances, per class {np.bincount(fx[key + 'cls'], minlength=4).tolist()}, "
                      f"{int(fx[key + 'soft'].sum())} soft, agreement {np.nanmax(fx[key + 'agree']):.1e}", flush=True)
            key = f"{model}_th_"
            x0, th = g9[key + "x0"], g9[key + "theta"]
            res = pool.map(instance, [(model, TH_N, x0[i], th[i], False, [11900 + (model == "linear"), i]) for i in range(len(x0))], chunksize=1)
            idx = [i for i, o in enumerate(res) if o is not None]
            if len(idx) < TH_MIN:
                raise SystemExit(f"{model} per-instance theta: only {len(idx)} of G9's {len(x0)} instances pass the gate")
            for k, v in stack([res[i] for i in idx], ("x0", "G", "g_theta", "g_x0", "agree")).items():
                fx[key + k] = v
            fx[key + "theta"], fx[key + "idx"] = th[idx], np.array(idx)
            print(f"{model} per-instance theta: {len(idx)} of {len(x0)} instances, agreement {np.nanmax(fx[key + 'agree']):.1e}", flush=True)
    fx["gamma"], fx["tol"], fx["gate"] = np.array(GAMMA), np.array(TOL), np.array(GATE)
    return fx


def shortfalls(fx):
    out = []
    for model, horizons in HORIZONS.items():
        for N in horizons:
            cls = fx[f"{model}_N{N}_cls"]
            for c, need in {**REQUIRED, **REQUIRED_AT.get((model, N), {})}.items():
                have = int((cls == c).sum())      # (counted as G9 counts them: a class-1 instance with a positive slack is one)
                if have < need:
                    out.append(f"{model} N {N}: {have} of {need} instances of class {c} in the fixture")
    return out


def main():
    fx = compute()
    short = shortfalls(fx)
    if short:
        raise SystemExit("\n".join(short))
    np.savez_compressed(os.path.join(HERE, "g11_traj_vjp.npz"), **fx)
    print("wrote g11_traj_vjp.npz:", os.path.getsize(os.path.join(HERE, "g11_traj_vjp.npz")), "bytes")


if __name__ == "__main__":
    main()
