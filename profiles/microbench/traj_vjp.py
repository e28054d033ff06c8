"""What mpcrl_traj_vjp (include/mpcrl_traj_ext.h) costs beside a solve, its parameter-sensitivity tail and mpcrl_state_sens.

    timeout -k 10 300 python profiles/microbench/traj_vjp.py [--out FILE] [--repeats 30] [--commit NAME]

Cartpole N 20 and linear system N 40, B 4096, one process, HIP events around one eager call (its launch overhead is inside every
figure), the calls alternating repeat by repeat after warm-up; median (min) in microseconds.  Per repeat, in this order:
  solve              mpcrl_solve, cold, no sensitivities
  vjp                mpcrl_traj_vjp after it, one random cotangent over all of (X, U), g_x0 and g_theta
  vjp (g_x0 alone)   the same without g_theta: loads, linearisation and the adjoint solve, no Jet2 parameter pass
  state_sens         mpcrl_state_sens with dpi_dx0 alone (the adjoint solve for -e_{u_0} and the stage-0 contraction)
  solve+dp           mpcrl_solve, cold, MPCRL_SENS_V | MPCRL_SENS_PI (the difference to `solve` is the solve's own sensitivity tail)
The line `tail` is median(solve+dp) - median(solve); `vjp / tail` is the ratio the pass was expected to keep below 1.5.
Nothing is asserted about the times."""
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


def ab(fns, repeats, warmup=5):
    t = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, f in fns.items():      # (in the order given: the calls on the stored iterate follow the plain solve)
            torch.cuda.synchronize()
            us = timed(f)
            if i >= warmup:
                t[k].append(us)
    return {k: (statistics.median(v), min(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--commit", default="the working tree", help="what the figures are labelled as measured on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("traj_vjp.py measures on the GPU; none found")
    from mpc4rl_amd import MPCBatch, _lib, cartpole_ocp, linear_system_ocp
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    B = 4096
    rng = np.random.default_rng(0)
    cases = (("cartpole N 20", cartpole_ocp(N=20, tf=2.0), rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 1.0, 0.3, 1.0])),
             ("linear N 40", linear_system_ocp(N=40), np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.2, 0.5, B)])))
    for name, ocp, x0n in cases:
        mpc = MPCBatch(ocp, B, device=dev)
        kw = dict(dtype=torch.float64, device=dev)
        x0 = torch.tensor(x0n, **kw)
        u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
        dVp, dpip = torch.empty((B, ocp.n_p), **kw), torch.empty((B, ocp.nu, ocp.n_p), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        dpi, g_x0, g_th = torch.empty((B, ocp.nu, ocp.nx), **kw), torch.empty((B, ocp.nx), **kw), torch.empty((B, ocp.n_p), **kw)
        gX = torch.tensor(rng.standard_normal((B, ocp.N + 1, ocp.nx)), **kw)
        gU = torch.tensor(rng.standard_normal((B, ocp.N, ocp.nu)), **kw)

        def solve(flags):
            mpc._call("mpcrl_solve", x0, None, flags | _lib.COLD, u0, V, dVp if flags else None, dpip if flags else None, status, iters)

        r = ab({"solve": lambda: solve(0),
                "vjp": lambda: mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th),
                "vjp (g_x0 alone)": lambda: mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, None),
                "state_sens": lambda: mpc._call("mpcrl_state_sens", 0, None, None, dpi),
                "solve+dp": lambda: solve(_lib.SENS_V | _lib.SENS_PI)}, args.repeats)
        mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th)
        torch.cuda.synchronize()
        ok = int((status == 0).sum())
        say(f"{name}, B {B} ({ok} solved, g_theta finite on {int(torch.isfinite(g_th).all(-1).sum())}): "
            + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
        tail = r["solve+dp"][0] - r["solve"][0]
        say(f"{name}: tail {tail:8.1f} us; vjp / tail {r['vjp'][0] / tail:5.2f}; Jet2 parameter pass (vjp - vjp without g_theta) "
            f"{r['vjp'][0] - r['vjp (g_x0 alone)'][0]:8.1f} us; the rest against state_sens {r['vjp (g_x0 alone)'][0] - r['state_sens'][0]:+8.1f} us")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
