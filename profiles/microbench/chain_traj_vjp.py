"""What mpcrl_chain_traj_vjp (include/mpcrl_chain_traj_ext.h) costs beside a chain solve, its sensitivity tail and
mpcrl_chain_policy_state_sens, on both of its routes.

    timeout -k 10 600 python profiles/microbench/chain_traj_vjp.py [--out FILE] [--repeats 20] [--commit NAME]

Chain of masses n_mass 5 and n_mass 7 at N 40, B 1024, one process, HIP events around one eager call (its launch overhead is inside
every figure), the calls alternating repeat by repeat after warm-up; median (min) in microseconds.  Per repeat, in this order:
  solve                 mpcrl_solve, cold, no sensitivities
  vjp (5 launches)      mpcrl_chain_traj_vjp after it: point pass, exact Hessians, adjoint solve, mixed term, outputs
  vjp g_x0 (4)          the same without g_theta: no mixed term
  policy (4 launches)   mpcrl_chain_policy_state_sens after it: point pass, exact Hessians, NU adjoint solves, contraction
  solve+dp              mpcrl_solve, cold, MPCRL_SENS_V | MPCRL_SENS_PI (the difference to `solve` is the solve's own sensitivity tail)
  vjp (3 launches)      mpcrl_chain_traj_vjp after it: adjoint solve, mixed term, outputs
  vjp g_x0 (2)          the same without g_theta
  policy (1 launch)     mpcrl_chain_policy_state_sens after it: the contraction alone
One random cotangent over all of (X, U).  Nothing is asserted about the times."""
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
        sys.exit("chain_traj_vjp.py measures on the GPU; none found")
    from mpc4rl_amd import MPCBatch, _lib, chain_mass_ocp
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    B, N = 1024, 40
    rng = np.random.default_rng(0)
    for n_mass in (5, 7):
        ocp = chain_mass_ocp(n_mass=n_mass, N=N)
        mpc = MPCBatch(ocp, B, device=dev)
        kw = dict(dtype=torch.float64, device=dev)
        x0 = torch.tensor(np.tile(ocp.consts, (B, 1)) + rng.normal(0.0, 0.05, (B, ocp.nx)), **kw)
        u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
        dVp, dpip = torch.empty((B, ocp.n_p), **kw), torch.empty((B, ocp.nu, ocp.n_p), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        dpi, g_x0, g_th = torch.empty((B, ocp.nu, ocp.nx), **kw), torch.empty((B, ocp.nx), **kw), torch.empty((B, ocp.n_p), **kw)
        gX = torch.tensor(rng.standard_normal((B, N + 1, ocp.nx)), **kw)
        gU = torch.tensor(rng.standard_normal((B, N, ocp.nu)), **kw)

        def solve(flags):
            mpc._call("mpcrl_solve", x0, None, flags | _lib.COLD, u0, V, dVp if flags else None, dpip if flags else None, status, iters)

        def vjp(theta):
            mpc._call("mpcrl_chain_traj_vjp", 0, status, gX, gU, g_x0, g_th if theta else None)

        def policy():
            mpc._call("mpcrl_chain_policy_state_sens", 0, status, dpi)

        r = ab({"solve": lambda: solve(0), "vjp (5 launches)": lambda: vjp(True), "vjp g_x0 (4)": lambda: vjp(False),
                "policy (4 launches)": policy, "solve+dp": lambda: solve(_lib.SENS_V | _lib.SENS_PI),
                "vjp (3 launches)": lambda: vjp(True), "vjp g_x0 (2)": lambda: vjp(False), "policy (1 launch)": policy}, args.repeats)
        vjp(True)
        torch.cuda.synchronize()
        say(f"chain n_mass {n_mass} N {N}, B {B} ({int((status == 0).sum())} solved, g_theta finite on {int(torch.isfinite(g_th).all(-1).sum())}): "
            + ", ".join(f"{k} {med:9.1f} ({mn:9.1f}) us" for k, (med, mn) in r.items()))
        tail = r["solve+dp"][0] - r["solve"][0]
        say(f"chain n_mass {n_mass}: tail {tail:9.1f} us; vjp (3 launches) / tail {r['vjp (3 launches)'][0] / tail:5.2f}; vjp (5 launches) / tail "
            f"{r['vjp (5 launches)'][0] / tail:5.2f}; vjp (3 launches) / solve {r['vjp (3 launches)'][0] / r['solve'][0]:5.3f}; "
            f"(N + 1) nx + N nu = {(N + 1) * ocp.nx + N * ocp.nu} solves by du0*/dp-style passes")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
