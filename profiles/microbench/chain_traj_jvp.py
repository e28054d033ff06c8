"""What mpcrl_chain_traj_jvp (include/mpcrl_chain_traj_jvp_ext.h) costs beside a chain solve and mpcrl_chain_traj_vjp on the same
handle, on both of its routes and at one and eight directions.

    timeout -k 10 600 python profiles/microbench/chain_traj_jvp.py [--out FILE] [--repeats 20] [--commit NAME]

Chain of masses n_mass 5 and n_mass 7 at N 40, B 1024, one process, HIP events around one eager call (its launch overhead is inside
every figure), the calls alternating repeat by repeat after warm-up; median (min) in microseconds.  Per repeat, in this order:
  solve                 mpcrl_solve, cold, no sensitivities
  jvp 1 (4 launches)    mpcrl_chain_traj_jvp after it, one direction: point pass, exact Hessians, right-hand side, Riccati solve
  jvp 8 (18)            the same with eight directions: 2 + 2 x 8 launches
  jvp 8 dx0 (10)        eight directions in x0 alone: no right-hand-side launch
  vjp (5 launches)      mpcrl_chain_traj_vjp after it (profiles/microbench/chain_traj_vjp.py)
  solve+dp              mpcrl_solve, cold, MPCRL_SENS_V | MPCRL_SENS_PI
  jvp 1 (2 launches)    mpcrl_chain_traj_jvp after it, one direction: right-hand side, Riccati solve
  jvp 8 (16)            eight directions
  jvp 8 dx0 (8)         eight directions in x0 alone
  vjp (3 launches)      mpcrl_chain_traj_vjp after it
Random directions over all of x0 and p, one random cotangent over all of (X, U).  Nothing is asserted about the times."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # microseconds


def ab(fns, repeats, warmup=3):
    t = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, f in fns.items():      # (in the order given: the calls on the workspace follow their solve)
            torch.cuda.synchronize()
            us = timed(f)
            if i >= warmup:
                t[k].append(us)
    return {k: (statistics.median(v), min(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--commit", default="the working tree", help="what the figures are labelled as measured on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chain_traj_jvp.py measures on the GPU; none found")
    from mpc4rl_amd import MPCBatch, _lib, chain_mass_ocp
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    B, N, R = 1024, 40, 8
    rng = np.random.default_rng(0)
    for n_mass in (5, 7):
        ocp = chain_mass_ocp(n_mass=n_mass, N=N)
        mpc = MPCBatch(ocp, B, device=dev)
        kw = dict(dtype=torch.float64, device=dev)
        x0 = torch.tensor(np.tile(ocp.consts, (B, 1)) + rng.normal(0.0, 0.05, (B, ocp.nx)), **kw)
        u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
        dVp, dpip = torch.empty((B, ocp.n_p), **kw), torch.empty((B, ocp.nu, ocp.n_p), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        g_x0, g_th = torch.empty((B, ocp.nx), **kw), torch.empty((B, ocp.n_p), **kw)
        gX = torch.tensor(rng.standard_normal((B, N + 1, ocp.nx)), **kw)
        gU = torch.tensor(rng.standard_normal((B, N, ocp.nu)), **kw)
        vx = torch.tensor(rng.standard_normal((B, R, ocp.nx)), **kw)
        vp = torch.tensor(rng.standard_normal((B, R, ocp.n_p)), **kw)
        vx1, vp1 = vx[:, :1].contiguous(), vp[:, :1].contiguous()
        dX, dU = torch.empty((B, R, N + 1, ocp.nx), **kw), torch.empty((B, R, N, ocp.nu), **kw)

        def solve(flags):
            mpc._call("mpcrl_solve", x0, None, flags | _lib.COLD, u0, V, dVp if flags else None, dpip if flags else None, status, iters)

        def jvp(ndir, theta=True):
            mpc._call("mpcrl_chain_traj_jvp", 0, status, ndir, vx1 if ndir == 1 else vx, (vp1 if ndir == 1 else vp) if theta else None, dX, dU)

        def vjp():
            mpc._call("mpcrl_chain_traj_vjp", 0, status, gX, gU, g_x0, g_th)

        r = ab({"solve": lambda: solve(0), "jvp 1 (4 launches)": lambda: jvp(1), "jvp 8 (18)": lambda: jvp(R),
                "jvp 8 dx0 (10)": lambda: jvp(R, False), "vjp (5 launches)": vjp,
                "solve+dp": lambda: solve(_lib.SENS_V | _lib.SENS_PI), "jvp 1 (2 launches)": lambda: jvp(1), "jvp 8 (16)": lambda: jvp(R),
                "jvp 8 dx0 (8)": lambda: jvp(R, False), "vjp (3 launches)": vjp}, args.repeats)
        jvp(R)
        torch.cuda.synchronize()
        say(f"chain n_mass {n_mass} N {N}, B {B} ({int((status == 0).sum())} solved, dX finite on {int(torch.isfinite(dX).all(-1).all(-1).all(-1).sum())}): "
            + ", ".join(f"{k} {med:9.1f} ({mn:9.1f}) us" for k, (med, mn) in r.items()))
        per = (r["jvp 8 (16)"][0] - r["jvp 1 (2 launches)"][0]) / (R - 1)
        say(f"chain n_mass {n_mass}: a further direction {per:9.1f} us, of which the right-hand side "
            f"{(r['jvp 8 (16)'][0] - r['jvp 8 dx0 (8)'][0]) / R:9.1f} us; jvp 1 (2 launches) / vjp (3 launches) "
            f"{r['jvp 1 (2 launches)'][0] / r['vjp (3 launches)'][0]:5.2f}; jvp 1 (2 launches) / solve {r['jvp 1 (2 launches)'][0] / r['solve'][0]:5.3f}; "
            f"the VJP route to the same column takes (N + 1) nx + N nu = {(N + 1) * ocp.nx + N * ocp.nu} cotangents")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
