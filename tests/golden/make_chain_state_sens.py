"""G10 — du0*/dx0 and dV/dx0 of the chain-of-masses OCP, from the mirror of the reference's NLP (oracle/nlp_mirror.py) at tight KKT
points.  Writes tests/golden/g10_chain_state_sens.npz.  CPU only:

    python tests/golden/make_chain_state_sens.py          (a few minutes on eight cores)

The recipe is the one of make_state_sens.py (G9).  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``solution_from_iterate`` and ``nlp_mirror.evaluate`` on it;
  3. du0*/dx0 = solve(dR_dz, -E)[:nu], E = dR/dx0 from the lbx0 / ubx0 rows;
  4. dV/dx0 = -pi0;
  5. the mirror's dpi_dp and dL_dp.
Cross-check: central differences of the port's u0* and V over x0 at h = 2e-4 and 1e-4, extrapolated.  An instance enters only if the
port's default mode (the product's twin) solves it too at tol 1e-9, and if mirror and differences agree to GATE = 1e-6 (RTOL of
tests/small_mode_cases.py, the bar the GPU test holds), rows scaled by max(|row|, 1).

Sets (SETS below), four instances each, x0 = base + N(0, 0.01) on every coordinate.  Around x_ss every instance is interior (class 0);
from the problem's default x0 one component of u_0 sits on its bound (class 2: ``active`` [B, nu] marks it, the mirror's row there
is ~1e-9 and is kept as the mirror gives it; the differences are compared on the free rows).  The generator fails rather than deliver
a set without its class.
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

TOL, GATE, ACTIVE, SIGMA, B = 1e-10, 1e-6, 1e-8, 0.01, 4
# (n_mass, N, base, class)
SETS = ((3, 1, "ss", 0), (3, 2, "ss", 0), (3, 10, "ss", 0), (3, 10, "x0", 2), (4, 3, "ss", 0), (5, 8, "ss", 0), (6, 3, "ss", 0),
        (7, 5, "ss", 0))
KEYS = ("x0", "u0", "V", "dV_dx0", "dpi_dx0", "dpi_dp", "dL_dp", "cls", "active", "agree_du", "agree_dV", "active_row")


def set_name(n_mass, N, base):
    return f"m{n_mass}_N{N}_{base}_"


def port(P, x0):
    return cpu_port.solve(P, np.atleast_2d(x0), flags=0, tol=TOL, exact=True, nthreads=1)


def extrapolated_differences(f, z, nout):
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
    n_mass, N, x0 = job
    torch.set_num_threads(1)
    P = make_chain_mass(n_mass=n_mass, N=N)
    nx, nu = P.nx, P.nu
    r = port(P, x0)
    if r.status[0] != 0 or cpu_port.solve(P, np.atleast_2d(x0), flags=0, tol=1e-9, nthreads=1).status[0] != 0:
        return None
    tu = np.minimum(r.BND[0, 2, :N, :nu], r.BND[0, 3, :N, :nu])      # slacks of the control rows [N, nu]
    if not ((tu < ACTIVE) | (tu > 1e-6)).all():                      # (nothing in between: a row is active or clearly not)
        return None
    active = tu[0] < ACTIVE
    cls = 2 if active.any() else (0 if (tu > 1e-6).all() else 1)
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0])
    mr = nlp_mirror.evaluate(P, sol, x0)
    rows = nlp_mirror.mirror_rows(P)
    nw = N * nu + (N + 1) * nx
    E = np.zeros((mr.dR_dz.shape[0], nx))
    for i, (k, kind, idx, sgn, bnd, sv) in enumerate(rows):
        if bnd in ("lbx0", "ubx0"):
            E[nw + N * nx + i, idx] = -sgn
    dpi_dx0 = np.linalg.solve(mr.dR_dz, -E)[:nu]

    def f(z):
        rr = port(P, z)
        return np.concatenate([rr.u0[0], rr.V])
    fd = extrapolated_differences(f, x0, nu + 1)
    out = dict(x0=x0, u0=r.u0[0], V=r.V[0], dV_dx0=-sol.pi0, dpi_dx0=dpi_dx0, dpi_dp=mr.dpi_dp, dL_dp=mr.dL_dp[0], cls=cls, active=active,
               agree_dV=scaled(-sol.pi0, fd[nu]), agree_du=scaled(dpi_dx0[~active], fd[:nu][~active]),
               active_row=float(np.abs(dpi_dx0[active]).max()) if active.any() else 0.0)
    return out if out["agree_du"] <= GATE and out["agree_dV"] <= GATE and out["active_row"] <= GATE else None


def main():
    fx = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for n_mass, N, base, want in SETS:
            P = make_chain_mass(n_mass=n_mass, N=N)
            rng = np.random.default_rng(10000 + 100 * n_mass + N + (base == "x0"))
            centre = P.extra["x_ss"] if base == "ss" else P.x0_default
            tag = set_name(n_mass, N, base)
            got = []
            for _ in range(3):
                x0 = centre + rng.normal(0.0, SIGMA, (B, P.nx))
                got += [o for o in pool.map(mirror_instance, [(n_mass, N, x) for x in x0], chunksize=1) if o is not None and o["cls"] == want]
                if len(got) >= B:
                    break
            if len(got) < B:
                raise SystemExit(f"{tag}: only {len(got)} of {B} instances of class {want} pass the gate")
            got = got[:B]
            for k in KEYS:
                fx[tag + k] = np.stack([np.asarray(o[k]) for o in got])
            print(f"{tag}: class {want}, agreement du {fx[tag + 'agree_du'].max():.1e} dV {fx[tag + 'agree_dV'].max():.1e} "
                  f"active row {fx[tag + 'active_row'].max():.1e}", flush=True)
    fx["tol"], fx["gate"], fx["sigma"] = np.array(TOL), np.array(GATE), np.array(SIGMA)
    out = os.path.join(HERE, "g10_chain_state_sens.npz")
    np.savez_compressed(out, **fx)
    print("wrote g10_chain_state_sens.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
