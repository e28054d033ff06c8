"""G17 — the four derivative calls of the chain-of-masses plan (trajectory JVP, trajectory VJP, bound VJP, du0*/dx0 and dV/dx0) at
shapes where the batch is more than one 64-lane workgroup of (instance, stage) lanes and where the horizon is long, from the mirror of
the reference's NLP (oracle/nlp_mirror.py) at tight KKT points.  Writes tests/golden/g17_chain_sens_shapes.npz.  CPU only:

    python tests/golden/make_chain_sens_shapes.py          (several minutes on eight cores)

The recipe is the one of make_chain_traj_jvp.py (G16) and make_chain_traj_vjp.py (G12), and it is their code: per instance
``instance`` of G16 (the KKT point from the port in exact-QP mode at tol 1e-10, ``solution_from_iterate``, ``nlp_mirror.evaluate``,
J_p = solve(dR_dz, -dR_dp)[:nw], J_x = solve(dR_dz, -E)[:nw], three directions, G16's gate) and ``instance`` of G12 (the same point
and Jacobians, three cotangents, G12's gate) are called as they are.  What neither of them returns is computed here from the same
point, and ``extras`` refuses an instance whose G J_p is not G12's g_theta to 1e-12:
  * g_lb, g_ub [R, N, nu] = G J_b on the control rows, J_b as make_bound_vjp.py (G13) builds it: one column of E per bound row of the
    mirror, -sgn in that row.  The chain has no state bounds and stage N has no controls: those columns of the library's
    [N + 1, nu + nx] output are exact zeros and are not stored;
  * dpi_dp = J_p[:nu], dpi_dx0 = J_x[:nu]; dV_dx0 = -pi0, as make_chain_state_sens.py (G10).
Of G12's three cotangents the two standard-normal ones are stored, with their rows (G, g_theta, g_x0, g_lb, g_ub: [B, 2, ...]).  The
third, the unit cotangent on component 0 of u_0, takes part in G12's gate and is then left out, to keep the file no larger than the
largest fixture there was (773 618 bytes; with it: 817 708): its g_theta and g_x0 are row 0 of dpi_dp and dpi_dx0, which the generator
checks to 1e-12 before it drops them.

Sets: (n_mass, N, base, B), stage lanes B N.
  m3_N10_mix  13 instances, 130 lanes: three workgroups, a tail of 2 lanes, instances 6 and 12 straddle a workgroup boundary
  m3_N16_ss    8 instances, 128 lanes: exactly two full workgroups
  m3_N40_mix   3 instances, 120 lanes: the default horizon, instance 1 straddles
  m3_N63_ss    2 instances, 126 lanes: the longest horizon mpcrl_create accepts
  m5_N40_ss    2 instances,  80 lanes: the benchmark's shape
  m7_N33_ss    2 instances,  66 lanes: a second workgroup of 2 lanes
``ss``: x0 = x_ss + N(0, 0.01) from default_rng([17000 + 100 n_mass + N]), as x0_near_ss of the GPU tests draws it.  ``mix``: the
instances at ACT_AT (0, 3, 6 and 12 of m3_N10_mix — both straddlers among them; 0 of m3_N40_mix) come from G12's ``act`` recipe,
x0 = x0_default + N(0, 0.2) from default_rng([17900 + N]), kept only with a control row active (slack < 1e-8) at a stage >= 1 and no
slack between 1e-8 and 1e-6 (``act`` [B] marks them).  The other instances of a mix set are ``ss``.  Of either kind SPARE = 4 x the
needed number of candidates are drawn and the first that pass both gates enter, in draw order — G10's and G12's rule: a draw of the
normal cotangents can miss G12's gate on an instance whose Jacobians are right (its docstring), and with nw = 1221 entries of w summed at
n_mass 7, N 33 it does so more often than on G12's own shapes (measured there: 2e-6 .. 4e-6 on three draws of one candidate, all of it
from the differences over m_0).  The ss candidates are gated as they are needed, the act candidates all at once.
Seeds of candidate c: [17100 + 100 n_mass + N, c] for G16's directions, [17500 + 100 n_mass + N, c] for G12's cotangents; an act
candidate takes 100 + c.  ``agree`` and ``draw`` [B, 2]: column 0 G16's gate, column 1 G12's.

The generator fails rather than deliver fewer than every instance of every set.
"""
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
import make_chain_traj_jvp as g16  # noqa: E402
import make_chain_traj_vjp as g12  # noqa: E402
from make_chain_traj_vjp import GATE, R, SIGMA_ACT, TOL, scaled  # noqa: E402

SIGMA, SPARE = 0.01, 4
SETS = ((3, 10, "mix", 13), (3, 16, "ss", 8), (3, 40, "mix", 3), (3, 63, "ss", 2), (5, 40, "ss", 2), (7, 33, "ss", 2))
ACT_AT = {(3, 10): (0, 3, 6, 12), (3, 40): (0,)}
KEYS = ("x0", "vx", "vp", "dX", "dU", "G", "g_theta", "g_x0", "g_lb", "g_ub", "dpi_dp", "dpi_dx0", "dV_dx0", "agree", "draw", "active")
COTANGENT_KEYS = ("G", "g_theta", "g_x0", "g_lb", "g_ub")


def set_name(n_mass, N, base):
    return f"m{n_mass}_N{N}_{base}_"


def gates(job):
    """('jvp' | 'vjp', n_mass, N, x0, seed) -> what that generator's ``instance`` returns."""
    which, rest = job[0], job[1:]
    return (g16 if which == "jvp" else g12).instance(rest)


def extras(job):
    n_mass, N, x0, G, g_theta = job
    torch.set_num_threads(1)
    P = make_chain_mass(n_mass=n_mass, N=N)
    nx, nu = P.nx, P.nu
    r = cpu_port.solve(P, x0[None], flags=0, tol=TOL, exact=True, nthreads=1)
    sol = solution_from_iterate(P, r.X[0], r.U[0], r.PI[0], r.BND[0])
    mr = nlp_mirror.evaluate(P, sol, x0)
    nw = N * nu + (N + 1) * nx
    rows = list(enumerate(nlp_mirror.mirror_rows(P)))
    Ex = np.zeros((mr.dR_dz.shape[0], nx))
    for i, (k, kind, idx, sgn, bnd, sv) in rows:
        if bnd in ("lbx0", "ubx0"):
            Ex[nw + N * nx + i, idx] = -sgn
    bound = [(i, k, idx, 0 if sgn < 0 else 1, sgn) for i, (k, kind, idx, sgn, bnd, sv) in rows if kind != "s" and bnd not in ("lbx0", "ubx0")]
    if any(kind != "u" for i, (k, kind, idx, sgn, bnd, sv) in rows if kind != "s" and bnd not in ("lbx0", "ubx0")) or len(bound) != 2 * N * nu:
        raise SystemExit("the chain has bound rows on its controls only")
    Eb = np.zeros((mr.dR_dz.shape[0], len(bound)))
    for col, (i, k, idx, side, sgn) in enumerate(bound):
        Eb[nw + N * nx + i, col] = -sgn
    Jp = np.linalg.solve(mr.dR_dz, -mr.dR_dp)[:nw]
    Jx = np.linalg.solve(mr.dR_dz, -Ex)[:nw]
    Jb = np.linalg.solve(mr.dR_dz, -Eb)[:nw]
    if not scaled(G @ Jp, g_theta) <= 1e-12:
        raise SystemExit(f"n_mass {n_mass} N {N}: G J_p is {scaled(G @ Jp, g_theta):.1e} from G12's g_theta")
    g = np.zeros((2, R, N, nu))
    for col, (i, k, idx, side, sgn) in enumerate(bound):
        g[side, :, k, idx] = G @ Jb[:, col]
    return dict(g_lb=g[0], g_ub=g[1], dpi_dp=Jp[:nu], dpi_dx0=Jx[:nu], dV_dx0=-sol.pi0)


def draw_x0(P, n_mass, N, base, B):
    """The candidates (of the ss instances [SPARE (B - n_act), nx], of the act instances [SPARE n_act, nx]), each in draw order."""
    n_act = len(ACT_AT.get((n_mass, N), ())) if base == "mix" else 0
    ss = P.extra["x_ss"] + np.random.default_rng([17000 + 100 * n_mass + N]).normal(0.0, SIGMA, (SPARE * (B - n_act), P.nx))
    act = P.x0_default + np.random.default_rng([17900 + N]).normal(0.0, SIGMA_ACT, (SPARE * n_act, P.nx))
    return ss, act


def main():
    # a pool: the candidates of one kind of one set, the slots (instances of the set) they fill in draw order, what passed so far
    pools = []
    for s, (n_mass, N, base, B) in enumerate(SETS):
        ss, act = draw_x0(make_chain_mass(n_mass=n_mass, N=N), n_mass, N, base, B)
        at = list(ACT_AT.get((n_mass, N), ())) if base == "mix" else []
        pools.append(dict(s=s, kind="ss", x0=ss, slots=[i for i in range(B) if i not in at], tail=0, tried=0, got=[]))
        if at:
            pools.append(dict(s=s, kind="act", x0=act, slots=at, tail=100, tried=0, got=[]))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        while True:
            # the ss candidates as they are needed, the act candidates (most of them next to an active-set change) all at once
            todo = []
            for p in pools:
                short = len(p["slots"]) - len(p["got"])
                take = min(len(p["x0"]) - p["tried"], short if p["kind"] == "ss" else (len(p["x0"]) if short else 0))
                todo += [(p, c) for c in range(p["tried"], p["tried"] + take)]
                p["tried"] += take
            if not todo:
                break
            jobs = []
            for p, c in todo:
                n_mass, N = SETS[p["s"]][:2]
                jobs += [("jvp", n_mass, N, p["x0"][c], [17100 + 100 * n_mass + N, p["tail"] + c]),
                         ("vjp", n_mass, N, p["x0"][c], [17500 + 100 * n_mass + N, p["tail"] + c])]
            order = sorted(range(len(jobs)), key=lambda j: -jobs[j][1] ** 3 * jobs[j][2])      # the long ones first
            res = dict(zip(order, pool.map(gates, [jobs[j] for j in order], chunksize=1)))
            for n, (p, c) in enumerate(todo):
                a, b = res[2 * n], res[2 * n + 1]
                tag = set_name(*SETS[p["s"]][:3])
                if a is None or b is None or (p["kind"] == "act" and not b["active"][1:].any()):
                    print(f"  {tag}: {p['kind']} candidate {c} does not enter (jvp {a is not None}, vjp {b is not None})", flush=True)
                    continue
                p["got"].append(dict(x0=p["x0"][c], vx=a["vx"], vp=a["vp"], dX=a["dX"], dU=a["dU"], G=b["G"], g_theta=b["g_theta"],
                                     g_x0=b["g_x0"], active=b["active"], agree=np.array([a["agree"], b["agree"]]),
                                     draw=np.array([a["draw"], b["draw"]])))
        kept = {}      # (set, instance) -> record
        for p in pools:
            if len(p["got"]) < len(p["slots"]):
                raise SystemExit(f"{set_name(*SETS[p['s']][:3])}: only {len(p['got'])} of {len(p['slots'])} {p['kind']} instances pass the gates")
            kept.update({(p["s"], i): o for i, o in zip(p["slots"], p["got"])})      # the first that passed, in draw order
        keys = sorted(kept)
        more = pool.map(extras, [(SETS[s][0], SETS[s][1], kept[s, i]["x0"], kept[s, i]["G"], kept[s, i]["g_theta"]) for s, i in keys], chunksize=1)
    for key, m in zip(keys, more):
        kept[key].update(m)
    fx = {}
    for s, (n_mass, N, base, B) in enumerate(SETS):
        tag = set_name(n_mass, N, base)
        for k in KEYS:
            fx[tag + k] = np.stack([np.asarray(kept[s, i][k]) for i in range(B)])
        unit = max(scaled(fx[tag + "g_theta"][:, R - 1], fx[tag + "dpi_dp"][:, 0]), scaled(fx[tag + "g_x0"][:, R - 1], fx[tag + "dpi_dx0"][:, 0]))
        if not unit <= 1e-12:
            raise SystemExit(f"{tag}: the unit cotangent is {unit:.1e} from row 0 of dpi_dp / dpi_dx0")
        for k in COTANGENT_KEYS:      # the unit cotangent is not stored
            fx[tag + k] = fx[tag + k][:, :R - 1]
        fx[tag + "act"] = np.array([base == "mix" and i in ACT_AT.get((n_mass, N), ()) for i in range(B)])
        print(f"{tag}: {B} instances, agreement jvp {fx[tag + 'agree'][:, 0].max():.1e} vjp {fx[tag + 'agree'][:, 1].max():.1e}, draws "
              f"{fx[tag + 'draw'].T.tolist()}, active rows at stages >= 1 {fx[tag + 'active'][:, 1:].sum((1, 2)).tolist()}", flush=True)
    fx["tol"], fx["gate"], fx["sigma"], fx["sigma_act"] = np.array(TOL), np.array(GATE), np.array(SIGMA), np.array(SIGMA_ACT)
    out = os.path.join(HERE, "g17_chain_sens_shapes.npz")
    np.savez_compressed(out, **fx)
    print("wrote g17_chain_sens_shapes.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
