"""G13 — derivatives of the planned trajectory w* = [u_0 .. u_{N-1}; x_0 .. x_N] and of the value V with respect to the box bounds,
row by row, from the mirror of the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.  Writes
tests/golden/g13_bound_vjp.npz.  CPU only:

    python tests/golden/make_bound_vjp.py          (about six minutes on eight cores)

The recipe is the one of make_traj_vjp.py (G11) and make_chain_traj_vjp.py (G12), imported from there where it is code.  Per instance
  1. the KKT point: the C++ port of the dense oracle, exact-QP mode, tol 1e-10 (cold);
  2. ``solution_from_iterate`` and ``nlp_mirror.evaluate`` on it;
  3. J_b = solve(dR_dz, -E)[:nw] with one column of E per bound row of the mirror: -sgn in the row h + t of that bound (h = sgn (v - b)
     [- s]: dR/db = -sgn there and nothing elsewhere).  The rows lbx0 / ubx0 (x_0 = x0: that is g_x0) and the slack rows have none;
  4. R = 3 cotangents G on w as in G11: two standard-normal draws over all of w and the unit cotangent on component 0 of u_0;
  5. stored: g_lb, g_ub [R, N + 1, nu + nx] = G J_b, one entry per stage and coordinate of v = [u; x], exactly 0 where the mirror has
     no row; dV_dlb = lam_l and dV_dub = -lam_u in the same layout; the mirror's du0*/dp (``dpi_dp``: the bar of the GPU test is
     relative to the error of the solve's own du0*/dp); x0; the bounds used (``lb0, ub0, lb, ub, lbe, ube``, the three groups of
     mpcrl_set_bounds, +-1e30 = absent); the masks ``act_lb, act_ub`` (slack < 1e-8) and the classes below; ``soft``; ``agree``,
     ``agree_V``; ``fd_u0`` [nb, nu] and ``fd_V`` [nb], the gate's differences of u_0* and of V over the shared vectors (``shared_vectors``).
Gate: central differences of the port's whole (U, X) and of V over the SHARED bound vectors — lbu, ubu (stages 0 .. N - 1), lbx, ubx
(stages 1 .. N - 1), lbx_e, ubx_e (stage N), each entry moved with ``dataclasses.replace`` — at h = 2e-4 and 1e-4, extrapolated
(4 f(h/2) - f(h)) / 3, against the mirror's rows summed over the stages that share the vector: 1e-7 on the small models (G11's gate),
1e-6 on the chain (G12's, with its DRAWS rule: the normal cotangents of an instance are drawn up to three times).  An instance also
enters only if it is solved, has no bound row with a slack between 1e-8 and 1e-6 (a row is active or clearly not), and if the port's
default mode (the product's twin) solves it at tol 1e-9.  Where a soft slack is positive the mirror holds the slacks constant (quirk
q1): that is the definition; such an instance is marked ``soft``, is not compared with differences (``agree`` NaN) and counts for
nothing below.  An instance without one is "firm".

Bounds of the sets (the default ones leave almost nothing to assert: an inactive row's gradient is about tau / t^2).
  * linear system, horizons of G11: lbx = (-1, -1), |u| <= 0.3, x0 in [0.1, 0.9] x [-0.4, 0.4];
  * cartpole, horizons of G11: |x| <= (0.6, 1.0, 0.4, 1.5) on the stages and at the end, |u| <= 8 — at N = 2 (a plan of 0.2 s) nothing
    is active at 8 and the control bound is U_BOUND_AT[("cartpole", 2)] — x0 = U(-1, 1) . (0.5, 0.3, 0.3, 0.5);
  * chain: G12's sets m3_N10_act, m3_N10_x0 and m5_N8_ss on their own x0, default bounds |u| <= 1.
Classes (flags, an instance can carry several): ``interior`` (no active row), ``act_u`` (an active control row at a stage >= 1),
``act_u0`` (u_0 on a bound), ``act_x`` (an active hard state row).  DRAWS_X0 candidates are drawn per (model, N), classified from
their KKT points, and the gate runs, in rounds, on the fewest that cover TARGET (greedily, in draw order) until the instances that
passed cover it or no candidate is left, so that the file stays small.  Cartpole, N = 15: the active state rows there are runs of 4 to
11 stages on the cart position, where the differences carry more of the solves' noise (agreement 1.2e-7 .. 1e-5 on most candidates),
and one candidate in ten passes the gate: DRAWS_AT draws 640 there, the gate left as it is.
The generator fails rather than deliver fewer firm instances than REQUIRED per (model, N) (REQUIRED_AT: none lowered), fewer than
CHAIN_ACTIVE instances with an active row in the chain sets, or a set with an active class in which no instance has
max(|g_lb|, |g_ub|) >= 0.1 on a normal cotangent.
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
from oracle.problems import make_chain_mass  # noqa: E402
from make_traj_vjp import GAMMA, HORIZONS, R, TOL, problem, scaled, w_of  # noqa: E402
from make_chain_traj_vjp import DRAWS, set_name  # noqa: E402

GATE = {"small": 1e-7, "chain": 1e-6}
ACTIVE, CLEAR, DRAWS_X0, MAGNITUDE = 1e-8, 1e-6, 64, 0.1
U_BOUND, U_BOUND_AT = {"cartpole": 8.0, "linear": 0.3}, {("cartpole", 2): 1.0}
DRAWS_AT = {("cartpole", 15): 640}      # (model, N) -> candidates where DRAWS_X0 do not hold enough that pass the gate
X_BOUND = np.array([0.6, 1.0, 0.4, 1.5])
X0_SCALE = np.array([0.5, 0.3, 0.3, 0.5])
CLASSES = ("interior", "act_u", "act_u0", "act_x")
REQUIRED = {"interior": 2, "act_u": 3, "act_u0": 1}
REQUIRED_X = {"act_x": 1}         # cartpole at N >= 15
REQUIRED_AT = {}                  # (model, N) -> {class: count} where a horizon cannot reach REQUIRED
TARGET = {"interior": 2, "act_u": 3, "act_u0": 1, "act_x": 2}      # what the instances that passed must cover: REQUIRED, and a second active state row
CHAIN_SETS = ((3, 10, "act"), (3, 10, "x0"), (5, 8, "ss"))
CHAIN_ACTIVE = {(3, 10, "act"): 4, (3, 10, "x0"): 1}
KEYS = ("x0", "G", "g_lb", "g_ub", "dV_dlb", "dV_dub", "dpi_dp", "act_lb", "act_ub", "soft", "agree", "agree_V", "fd_u0", "fd_V") + CLASSES


def bounded(model, N):
    """The problem of G11 at this horizon with the bounds of this fixture."""
    P = problem(model, N)
    ub = U_BOUND_AT.get((model, N), U_BOUND[model])
    if model == "linear":
        return dataclasses.replace(P, lbu=np.array([-ub]), ubu=np.array([ub]), lbx=np.array([-1.0, -1.0]))
    return dataclasses.replace(P, lbu=np.array([-ub]), ubu=np.array([ub]), lbx=-X_BOUND, ubx=X_BOUND.copy(), lbx_e=-X_BOUND, ubx_e=X_BOUND.copy())


def draw_x0(model, N):
    rng, n = np.random.default_rng([13000, int(model == "linear"), N]), DRAWS_AT.get((model, N), DRAWS_X0)
    if model == "linear":
        return np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(-0.4, 0.4, n)], 1)
    return rng.uniform(-1.0, 1.0, (n, 4)) * X0_SCALE


def groups(P):
    """The three groups of mpcrl_set_bounds for this problem, +-1e30 = absent."""
    lb, ub, lbe, ube = cpu_port.stage_bounds(P)[:4]
    return dict(lb0=lb[:P.nu].copy(), ub0=ub[:P.nu].copy(), lb=lb, ub=ub, lbe=lbe, ube=ube)


def row_mask(P):
    """[2, N + 1, nu + nx]: the bound rows the OCP has (stage-0 states and terminal controls have none)."""
    g = groups(P)
    m = np.zeros((2, P.N + 1, P.nu + P.nx), bool)
    m[0, :P.N, :P.nu], m[1, :P.N, :P.nu] = g["lb"][:P.nu] > -1e29, g["ub"][:P.nu] < 1e29
    m[0, 1:P.N, P.nu:], m[1, 1:P.N, P.nu:] = g["lb"][P.nu:] > -1e29, g["ub"][P.nu:] < 1e29
    m[0, P.N, P.nu:], m[1, P.N, P.nu:] = g["lbe"] > -1e29, g["ube"] < 1e29
    return m


def classify(P, bnd):
    """(flags {class: bool}, soft, act [2, N + 1, nw]) of one KKT point, or None where a row is neither active nor clearly not."""
    nu = P.nu
    m = row_mask(P)
    t = np.where(m, bnd[2:4], 1.0)
    if ((t >= ACTIVE) & (t <= CLEAR)).any():
        return None
    act = m & (t < ACTIVE)
    soft = bool((bnd[4:6] > ACTIVE).any())
    softc = np.zeros(P.nu + P.nx, bool)
    softc[[nu + int(P.idxbx[j]) for j in P.idxsbx]] = True
    flags = dict(interior=not act.any(), act_u=bool(act[:, 1:, :nu].any()), act_u0=bool(act[:, 0, :nu].any()),
                 act_x=bool(act[:, :, nu:][:, :, ~softc[nu:]].any()))
    return flags, soft, act


def shared_vectors(P):
    """[(field of the problem, entry, side, stages, coordinate of v)] — the bound vectors the port shares over stages."""
    N, nu, out = P.N, P.nu, []
    for i in range(nu):
        out += [("lbu", i, 0, range(0, N), i), ("ubu", i, 1, range(0, N), i)]
    for j, ix in enumerate(P.idxbx):
        out += [("lbx", j, 0, range(1, N), nu + int(ix)), ("ubx", j, 1, range(1, N), nu + int(ix))]
    for j, ix in enumerate(P.idxbx_e):
        out += [("lbx_e", j, 0, range(N, N + 1), nu + int(ix)), ("ubx_e", j, 1, range(N, N + 1), nu + int(ix))]
    return out


def differences(P, x0):
    """(d w* / d b [nw, nb], dV / d b [nb]) over the shared vectors by extrapolated central differences; None where a solve fails."""
    vec = shared_vectors(P)
    d_w, d_V = [], []
    for h in (2e-4, 1e-4):
        w, V = [], []
        for sgn in (1.0, -1.0):
            for name, j, _, _, _ in vec:
                b = getattr(P, name).copy()
                b[j] += sgn * h
                r = cpu_port.solve(dataclasses.replace(P, **{name: b}), x0[None], flags=0, tol=TOL, exact=True, nthreads=1)
                if r.status[0] != 0:
                    return None
                w.append(w_of(r)[0]), V.append(r.V[0])
        w, V = np.array(w).reshape(2, len(vec), -1), np.array(V).reshape(2, len(vec))
        d_w.append((w[0] - w[1]) / (2 * h)), d_V.append((V[0] - V[1]) / (2 * h))
    return ((4 * d_w[1] - d_w[0]) / 3).T, (4 * d_V[1] - d_V[0]) / 3


def instance(job):
    kind, spec, x0, seed = job      # (a problem holds closures: the worker builds its own)
    torch.set_num_threads(1)
    P = make_chain_mass(n_mass=spec[0], N=spec[1]) if kind == "chain" else bounded(*spec)
    N, nx, nu = P.N, P.nx, P.nu
    r = cpu_port.solve(P, x0[None], flags=0, tol=TOL, exact=True, nthreads=1)
    if r.status[0] != 0 or cpu_port.solve(P, x0[None], flags=0, tol=1e-9, nthreads=1).status[0] != 0:
        return None
    c = classify(P, r.BND[0])
    if c is None:
        return None
    flags, soft, act = c
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0])
    mr = nlp_mirror.evaluate(P, sol, x0)
    nw, nv = N * nu + (N + 1) * nx, nu + nx
    rows = [(i, k, (idx if vk == "u" else nu + idx), 0 if sgn < 0 else 1, sgn)
            for i, (k, vk, idx, sgn, bnd, sv) in enumerate(nlp_mirror.mirror_rows(P)) if vk != "s" and bnd not in ("lbx0", "ubx0")]
    E = np.zeros((mr.dR_dz.shape[0], len(rows)))
    for col, (i, k, cv, side, sgn) in enumerate(rows):
        E[nw + N * nx + i, col] = -sgn
    Jb = np.linalg.solve(mr.dR_dz, -E)[:nw]
    J = np.zeros((2, nw, N + 1, nv))      # [side, w, stage, coordinate]: zero where the mirror has no row
    dV = np.zeros((2, N + 1, nv))
    for col, (i, k, cv, side, sgn) in enumerate(rows):
        J[side, :, k, cv] = Jb[:, col]
        dV[side, k, cv] = -sgn * mr.lam[i]
    if not (row_mask(P) == (J != 0).any(1)).all():      # (a row without any effect on w would be a surprise worth hearing of)
        return None
    out = dict(x0=x0, dV_dlb=dV[0], dV_dub=dV[1], dpi_dp=mr.dpi_dp, act_lb=act[0], act_ub=act[1], soft=soft, agree=np.nan, agree_V=np.nan,
               **flags)
    fd = None if soft else differences(P, x0)
    if fd is None and not soft:
        return None
    vec = shared_vectors(P)
    out["fd_u0"] = np.full((len(vec), nu), np.nan) if soft else fd[0][:nu].T      # the differences of u_0* and of V themselves
    out["fd_V"] = np.full(len(vec), np.nan) if soft else fd[1]
    for draw in range(DRAWS if kind == "chain" else 1):
        G = np.random.default_rng(list(seed) + [draw]).standard_normal((R, nw))
        G[R - 1] = 0.0
        G[R - 1, 0] = 1.0
        g = np.einsum("rw,swkc->srkc", G, J)
        out.update(G=G, g_lb=g[0], g_ub=g[1])
        if soft:
            return out
        summed = np.stack([g[side][:, list(stages), cv].sum(1) for _, _, side, stages, cv in vec], 1)
        out["agree"] = scaled(summed, G @ fd[0])
        out["agree_V"] = scaled(np.array([dV[side, list(stages), cv].sum() for _, _, side, stages, cv in vec]), fd[1])
        if max(out["agree"], out["agree_V"]) <= GATE[kind]:
            return out
    return None


def cover(cands, have, target, skip):
    """The fewest candidates not in ``skip``, greedily in draw order, that bring ``have[c]`` up to target[c] for every class c (or all
    there are)."""
    picked = []
    for c in target:
        for i, (flags, soft) in enumerate(cands):
            if target[c] <= have[c] + sum(cands[j][0][c] for j in picked):
                break
            if flags is not None and not soft and flags[c] and i not in picked and i not in skip:
                picked.append(i)
    return sorted(picked)


def small_set(pool, model, N):
    P = bounded(model, N)
    x0 = draw_x0(model, N)
    r = cpu_port.solve(P, x0, flags=0, tol=TOL, exact=True)
    cands = []
    for i in range(len(x0)):
        c = classify(P, r.BND[i]) if r.status[i] == 0 else None
        cands.append((None, False) if c is None else (c[0], c[1]))
    counts = {c: sum(1 for f, s in cands if f is not None and not s and f[c]) for c in CLASSES}
    target = {c: n for c, n in TARGET.items() if c != "act_x" or (model == "cartpole" and N >= 15)}
    got, tried = {}, set()
    if model == "linear":      # one instance with a positive slack: the definition (quirk q1), not compared with differences
        tried.update([i for i, (f, s) in enumerate(cands) if f is not None and s][:1])
    picked = sorted(tried)
    while True:      # the gate turns a third of the candidates away: rounds, until the passed ones cover the target or none are left
        have = {c: sum(1 for o in got.values() if o[c] and not o["soft"]) for c in CLASSES}
        picked += cover(cands, have, target, tried | set(picked))
        if not picked:
            break
        res = pool.map(instance, [("small", (model, N), x0[i], [13100 + int(model == "linear"), N, i]) for i in picked], chunksize=1)
        got.update({i: o for i, o in zip(picked, res) if o is not None})
        tried.update(picked)
        picked = []
    print(f"{model} N {N}: firm candidates per class {counts} of {len(x0)} draws, gate run on {len(tried)}, passed {len(got)}", flush=True)
    return P, [got[i] for i in sorted(got)]


def chain_set(pool, g12, n_mass, N, base):
    P = make_chain_mass(n_mass=n_mass, N=N)
    x0 = g12[set_name(n_mass, N, base) + "x0"]
    got = pool.map(instance, [("chain", (n_mass, N), x0[i], [13900 + 100 * n_mass + N + (base == "x0"), i]) for i in range(len(x0))], chunksize=1)
    return P, [o for o in got if o is not None]


def store(fx, tag, P, got):
    for k in KEYS:
        fx[tag + k] = np.stack([np.asarray(o[k]) for o in got])
    for k, v in groups(P).items():
        fx[tag + k] = v
    firm = ~fx[tag + "soft"]
    big = max((max(np.abs(o["g_lb"][:R - 1]).max(), np.abs(o["g_ub"][:R - 1]).max()) for o in got if not o["soft"]), default=0.0)
    print(f"{tag}: {len(got)} instances, firm per class {{{', '.join(f'{c}: {int((fx[tag + c] & firm).sum())}' for c in CLASSES)}}}, "
          f"{int((~firm).sum())} soft, agreement w {np.nanmax(fx[tag + 'agree']):.1e} V {np.nanmax(fx[tag + 'agree_V']):.1e}, "
          f"largest |g| on a normal cotangent {big:.2e}", flush=True)


def shortfalls(fx):
    out = []

    def magnitude(tag):
        firm = ~fx[tag + "soft"]
        if (fx[tag + "act_lb"][firm].any() or fx[tag + "act_ub"][firm].any()) and \
                not max(np.abs(fx[tag + "g_lb"][firm][:, :R - 1]).max(), np.abs(fx[tag + "g_ub"][firm][:, :R - 1]).max()) >= MAGNITUDE:
            out.append(f"{tag}: no instance with a bound gradient of {MAGNITUDE} on a normal cotangent")

    for model, horizons in HORIZONS.items():
        for N in horizons:
            tag = f"{model}_N{N}_"
            need = {**REQUIRED, **(REQUIRED_X if model == "cartpole" and N >= 15 else {}), **REQUIRED_AT.get((model, N), {})}
            for c, n in need.items():
                have = int((fx[tag + c] & ~fx[tag + "soft"]).sum())
                if have < n:
                    out.append(f"{tag}: {have} of {n} firm instances of class {c}")
            magnitude(tag)
    for s in CHAIN_SETS:
        tag = set_name(*s)
        have = int((fx[tag + "act_lb"] | fx[tag + "act_ub"]).any((1, 2)).sum())
        if have < CHAIN_ACTIVE.get(s, 0):
            out.append(f"{tag}: {have} of {CHAIN_ACTIVE[s]} instances with an active row")
        magnitude(tag)
    return out


def main():
    g12 = np.load(os.path.join(HERE, "g12_chain_traj_vjp.npz"))
    fx = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for s in CHAIN_SETS:
            P, got = chain_set(pool, g12, *s)
            if len(got) < len(g12[set_name(*s) + "x0"]):
                raise SystemExit(f"{set_name(*s)}: only {len(got)} of G12's instances pass the gate")
            store(fx, set_name(*s), P, got)
        for model, horizons in HORIZONS.items():
            for N in horizons:
                P, got = small_set(pool, model, N)
                if not got:
                    raise SystemExit(f"{model} N {N}: no instance passes the gate")
                store(fx, f"{model}_N{N}_", P, got)
    short = shortfalls(fx)
    if short:
        raise SystemExit("\n".join(short))
    fx["gamma"], fx["tol"], fx["gate_small"], fx["gate_chain"] = np.array(GAMMA), np.array(TOL), np.array(GATE["small"]), np.array(GATE["chain"])
    out = os.path.join(HERE, "g13_bound_vjp.npz")
    np.savez_compressed(out, **fx)
    print("wrote g13_bound_vjp.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
