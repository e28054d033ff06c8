"""G9 — state sensitivities dV/dx0, dQ/dx0, dQ/du0, du0*/dx0 of the cartpole and the linear-system OCP, from the mirror of the
reference's NLP (oracle/nlp_mirror.py) at tight KKT points.  Writes tests/golden/g9_state_sens.npz.  CPU only:

    python tests/golden/make_state_sens.py          (about a quarter of an hour on eight cores)

Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``nlp_mirror.evaluate`` on it (``solution_from_iterate``);
  3. du0*/dx0 = solve(dR_dz, -E)[:nu], E = dR/dx0: x0 is the bound value of the lbx0 / ubx0 rows, whose h + t row has -sgn in the
     column of its state;
  4. dV/dx0 = -pi0 (minus the multiplier of x_0 = x0);
  5. Q mode (u0 fixed): the same for dQ/dx0, and dQ/du0 = grad_u [c_0 l_0 + pi_1' F](x0, u0) by autograd;
  6. the mirror's dpi_dp and dL_dp.
Cross-check: central differences of u0* and V (Q) over x0 (and u0) at h = 2e-4 and 1e-4, extrapolated (4 f(h/2) - f(h)) / 3.  An
instance enters the fixture only if mirror and differences agree to 1e-7, rows scaled by max(|row|, 1).  Two exceptions: where a
soft slack is positive the mirror holds the slacks constant (quirk q1) — it is the definition and the differences are not compared;
where u_0 sits on its bound the expected du0*/dx0 is exactly 0 (``dpi_dx0`` holds that zero; the dense solve there carries noise).
The generator fails rather than deliver fewer instances or classes than REQUIRED below.

Classes (``cls``): 0 interior (no control row, no hard state row active, no slack positive), 1 a control bound active at a stage
>= 1 with u_0 free, 2 u_0 on its bound, 3 anything else (an active state row, u_0 free).  ``soft`` marks a positive slack.
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

TOL, GATE, ACTIVE, GAMMA = 1e-10, 1e-7, 1e-8, 0.99
HORIZONS = {"cartpole": (2, 15, 20, 31, 32, 63), "linear": (2, 7, 20, 31, 32, 63)}
BATCH = {"cartpole": 13, "linear": 25}
REQUIRED = {0: 4, 1: 3, 2: 1}      # class -> instances per (model, N), at least
Q_N, TH_N, TH_B = 20, 20, 3


def problem(model, N):
    return make_cartpole(N=N, tf=0.1 * N) if model == "cartpole" else make_linear_system(gamma=GAMMA, N=N)


def port(P, x0, p=None, u0fix=None):
    return cpu_port.solve(P, np.atleast_2d(x0), p=p, u0fix=u0fix, flags=0, tol=TOL, exact=True, nthreads=1)


def classify(P, r):
    """(cls [n], soft [n]) of the port's solutions; -1 = not solved."""
    N, nu = P.N, P.nu
    B = r.BND
    tu = np.minimum(B[:, 2, :N, :nu], B[:, 3, :N, :nu]).min(2)      # smallest slack of the control rows per stage
    soft = (B[:, 4:6] > ACTIVE).any((1, 2, 3))
    xact = (B[:, 2:4, 1:, nu:] < ACTIVE).any((1, 2, 3))
    if len(P.idxsbx):      # rows of a softened coordinate are active where the slack is positive; the tail x -> 0 = lbx is not
        hard = [nu + int(ix) for j, ix in enumerate(P.idxbx) if j not in set(int(s) for s in P.idxsbx)]
        xact = (B[:, 2:4, 1:, hard] < ACTIVE).any((1, 2, 3))
    cls = np.full(len(r.status), 3)
    cls[(tu[:, 1:] < ACTIVE).any(1) & (tu[:, 0] > 1e-6)] = 1
    cls[(tu > 1e-6).all(1) & ~xact & ~soft] = 0
    cls[tu[:, 0] < ACTIVE] = 2
    keep = (r.status == 0) & ((tu < ACTIVE) | (tu > 1e-6)).all(1)      # (nothing in between: a row is active or clearly not)
    cls[~keep] = -1
    return cls, soft


def extrapolated_differences(f, z, nout):
    """d f / d z by central differences at h = 2e-4 and 1e-4, extrapolated."""
    J = np.zeros((nout, len(z)))
    for j in range(len(z)):
        d = []
        for h in (2e-4, 1e-4):
            e = np.zeros(len(z))
            e[j] = h
            d.append((f(z + e) - f(z - e)) / (2 * h))
        J[:, j] = (4 * d[1] - d[0]) / 3
    return J


def scaled(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1.0)).max())


def mirror_instance(job):
    """One instance: the mirror's quantities and their agreement with the differences (NaN = not compared)."""
    model, N, x0, p, u0fix, cls, soft = job
    torch.set_num_threads(1)
    P = problem(model, N)
    nx, nu = P.nx, P.nu
    r = port(P, x0, p=p, u0fix=None if u0fix is None else u0fix[None])
    if r.status[0] != 0:
        return None
    # the product's own iteration (the port's default mode is its twin) must solve the instance too, at the tolerance of the GPU test
    if cpu_port.solve(P, np.atleast_2d(x0), p=p, u0fix=None if u0fix is None else u0fix[None], flags=0, tol=1e-9, nthreads=1).status[0] != 0:
        return None
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0], p=p, u0fix=u0fix)
    mr = nlp_mirror.evaluate(P, sol, x0, p=p, u0fix=u0fix)
    rows = nlp_mirror.mirror_rows(P)
    nw = N * nu + (N + 1) * nx
    E = np.zeros((mr.dR_dz.shape[0], nx))
    for i, (k, kind, idx, sgn, bnd, sv) in enumerate(rows):
        if bnd in ("lbx0", "ubx0"):
            E[nw + N * nx + i, idx] = -sgn
    out = dict(x0=x0, u0=r.u0[0], V=r.V[0], dV_dx0=-sol.pi0, dL_dp=mr.dL_dp[0], dpi_dp=mr.dpi_dp,
               dpi_dx0_mirror=np.linalg.solve(mr.dR_dz, -E)[:nu], soft=soft, agree_du=np.nan, agree_dV=np.nan, agree_dQ=np.nan)
    out["dpi_dx0"] = np.zeros((nu, nx)) if (cls == 2 or u0fix is not None) else out["dpi_dx0_mirror"]
    pp = None if p is None else p[None]
    if u0fix is not None:
        ut = torch.tensor(u0fix, requires_grad=True)
        pt = torch.tensor(P.p0 if p is None else p)
        c0 = float(P.cost_scaling()[0])
        l0 = c0 * P.stage_cost(0, torch.tensor(x0), ut, pt) + torch.tensor(r.PI[0, 0]) @ P.F(torch.tensor(x0), ut, pt)
        out["dQ_du0"] = torch.autograd.grad(l0, ut)[0].numpy()
        if not soft:
            fd = extrapolated_differences(lambda z: port(P, z[:nx], p=pp, u0fix=z[None, nx:]).V, np.concatenate([x0, u0fix]), 1)
            out["agree_dV"], out["agree_dQ"] = scaled(out["dV_dx0"], fd[0, :nx]), scaled(out["dQ_du0"], fd[0, nx:])
    elif not soft:
        def f(z):
            rr = port(P, z, p=pp)
            return np.concatenate([rr.u0[0], rr.V])
        fd = extrapolated_differences(f, x0, nu + 1)
        out["agree_dV"] = scaled(out["dV_dx0"], fd[nu])
        if cls != 2:
            out["agree_du"] = scaled(out["dpi_dx0"], fd[:nu])
    ok = all(not (v > GATE) for v in (out["agree_du"], out["agree_dV"], out["agree_dQ"]))
    return out if ok else None


def candidates(model, N, rng):
    n = 40000 if N == 2 else 6000
    if model == "cartpole":
        x0 = np.concatenate([rng.uniform(-1, 1, (n // 2, 4)) * np.array([1.5, 3.0, 1.0, 5.0]),
                             rng.uniform(-1, 1, (n // 2, 4)) * np.array([2.0, 9.0, 3.0, 9.0])])
    else:
        x0 = np.concatenate([np.column_stack([rng.uniform(0.02, 0.98, n // 2), rng.uniform(-0.9, 0.9, n // 2)]),
                             np.column_stack([rng.uniform(-1.0, 2.0, n // 2), rng.uniform(-2.0, 2.0, n // 2)])])
    return x0[rng.permutation(len(x0))]


def collect(pool, model, N, jobs_of_class, want, tag):
    """Takes candidates class by class (round robin once the REQUIRED ones are in) until ``want`` instances passed the gate."""
    got = {c: [] for c in jobs_of_class}
    cursor = {c: 0 for c in jobs_of_class}

    def draw(c, k):
        lst = jobs_of_class[c][cursor[c]: cursor[c] + k]
        cursor[c] += len(lst)
        res = [o for o in pool.map(mirror_instance, lst) if o is not None]
        for o in res:
            o["cls"] = c
        got[c] += res
        return len(lst)

    for c, need in REQUIRED.items():
        while len(got[c]) < need:
            if not draw(c, 2 * (need - len(got[c])) + 2):
                raise SystemExit(f"{tag}: only {len(got[c])} of {need} instances of class {c} pass the gate")
        got[c] = got[c][:need]
    order, i = [0, 1, 3, 2], 0
    while sum(len(v) for v in got.values()) < want:
        c = order[i % len(order)]
        i += 1
        before = len(got[c])
        if draw(c, 1) == 0 and all(cursor[k] >= len(jobs_of_class[k]) for k in got):
            raise SystemExit(f"{tag}: candidates exhausted at {sum(len(v) for v in got.values())} of {want} instances")
        got[c] = got[c][: before + 1]
    out = [o for c in sorted(got) for o in got[c]]
    print(f"{tag}: {[len(got[c]) for c in sorted(got)]} instances per class, "
          f"agreement du {np.nanmax([o['agree_du'] for o in out]):.1e} dV {np.nanmax([o['agree_dV'] for o in out]):.1e}", flush=True)
    return out[:want]


def stack(out, keys):
    return {k: np.stack([np.asarray(o[k]) for o in out]) for k in keys}


def q_mode_set(pool, model, x0v, u0v, n_interior):
    """Q mode at N = Q_N, BATCH[model] instances: rows 0..3 are four of the first n_interior (interior) rows of the V-mode set with
    their own u0* pinned (``vrow`` says which; -1 elsewhere); the others take the x0 of the V-mode set in its order with a random
    pinned control, an x0 at which six draws of the control all fail the gate (an active set that switches inside the difference
    stencil) being passed over."""
    P = problem(model, Q_N)
    rng = np.random.default_rng(9500 + (model == "linear"))
    B = len(x0v)
    own = pool.map(mirror_instance, [(model, Q_N, x0v[i], None, u0v[i], 0, False) for i in range(n_interior)])
    rows = [i for i, o in enumerate(own) if o is not None][:4]      # (a pinned solve that stops short of tol 1e-10 is passed over)
    if len(rows) < 4:
        raise SystemExit(f"{model} Q mode: only {len(rows)} of 4 rows that pin their own u0* pass the gate")
    res, us = [own[i] for i in rows], [u0v[i] for i in rows]
    i = 4
    while len(res) < B:
        if i >= 3 * B:
            raise SystemExit(f"{model} Q mode: only {len(res)} of {B} instances pass the gate")
        x0 = x0v[i % B]
        i += 1
        u0fix = rng.uniform(0.9 * P.lbu, 0.9 * P.ubu, (6, P.nu))
        rq = cpu_port.solve(P, np.tile(x0, (6, 1)), u0fix=u0fix, flags=0, tol=TOL, exact=True)
        softq = (rq.BND[:, 4:6] > ACTIVE).any((1, 2, 3))
        for o, u in zip(pool.map(mirror_instance, [(model, Q_N, x0, None, u0fix[j], 0, bool(softq[j])) for j in range(6)]), u0fix):
            if o is not None:
                res.append(o), us.append(u)
                break
    for j, (o, u) in enumerate(zip(res, us)):
        o["u0fix"], o["vrow"] = u, rows[j] if j < 4 else -1
    out = {f"{model}_q_{k}": v for k, v in stack(res, ("x0", "u0fix", "vrow", "V", "dV_dx0", "dQ_du0", "dL_dp", "soft", "agree_dV", "agree_dQ")).items()}
    print(f"{model} Q mode: agreement dQ/dx0 {np.nanmax(out[f'{model}_q_agree_dV']):.1e} dQ/du0 {np.nanmax(out[f'{model}_q_agree_dQ']):.1e}, "
          f"{int(out[f'{model}_q_soft'].sum())} with a positive slack", flush=True)
    return out


def main():
    fx = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for model, horizons in HORIZONS.items():
            for N in sorted(horizons, key=lambda n: n != Q_N):      # (the horizon of the Q-mode and theta sets first)
                P = problem(model, N)
                rng = np.random.default_rng(9000 + 100 * (model == "linear") + N)
                x0 = candidates(model, N, rng)
                cls, soft = classify(P, cpu_port.solve(P, x0, flags=0, tol=TOL, exact=True))
                jobs = {c: [(model, N, x0[i], None, None, c, bool(soft[i])) for i in np.where(cls == c)[0][:60]] for c in (0, 1, 2, 3)}
                out = collect(pool, model, N, jobs, BATCH[model], f"{model} N {N}")
                for k, v in stack(out, ("x0", "u0", "V", "dV_dx0", "dpi_dx0", "dpi_dx0_mirror", "dpi_dp", "dL_dp", "cls", "soft",
                                        "agree_du", "agree_dV")).items():
                    fx[f"{model}_N{N}_{k}"] = v
                if N != Q_N:
                    continue
                fx.update(q_mode_set(pool, model, fx[f"{model}_N{Q_N}_x0"], fx[f"{model}_N{Q_N}_u0"], int((fx[f"{model}_N{Q_N}_cls"] == 0).sum())))
                # per-instance theta (+-5 % of p0) at N = TH_N: interior instances of the V-mode set
                P = problem(model, TH_N)
                rng = np.random.default_rng(9700 + (model == "linear"))
                res = []
                for i in range(BATCH[model]):
                    th = P.p0 * (1.0 + 0.05 * rng.uniform(-1, 1, P.n_p))
                    o = mirror_instance((model, TH_N, fx[f"{model}_N{TH_N}_x0"][i], th, None, 0, False))
                    if o is not None:
                        o["theta"] = th
                        res.append(o)
                    if len(res) == TH_B:
                        break
                if len(res) < TH_B:
                    raise SystemExit(f"{model} per-instance theta: only {len(res)} of {TH_B} instances pass the gate")
                for k, v in stack(res, ("x0", "theta", "u0", "V", "dV_dx0", "dpi_dx0", "dpi_dp", "dL_dp", "agree_du", "agree_dV")).items():
                    fx[f"{model}_th_{k}"] = v
                print(f"{model} per-instance theta: agreement du {np.nanmax(fx[f'{model}_th_agree_du']):.1e} dV {np.nanmax(fx[f'{model}_th_agree_dV']):.1e}")
    fx["gamma"], fx["tol"], fx["gate"] = np.array(GAMMA), np.array(TOL), np.array(GATE)
    np.savez_compressed(os.path.join(HERE, "g9_state_sens.npz"), **fx)
    print("wrote g9_state_sens.npz:", os.path.getsize(os.path.join(HERE, "g9_state_sens.npz")), "bytes")


if __name__ == "__main__":
    main()
