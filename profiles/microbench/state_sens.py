"""What mpcrl_state_sens costs beside the solve and the parameter-sensitivity pass of the same handle.

    python profiles/microbench/state_sens.py [--out FILE] [--repeats 30] [--commit NAME]

Cartpole N 20 and linear system N 40, B 4096 each, one process, HIP events around one eager call (its launch overhead is inside every
figure), the calls alternating repeat by repeat after warm-up; median (min) in microseconds:
  solve            mpcrl_solve, cold, no sensitivities
  solve+dp         mpcrl_solve, cold, MPCRL_SENS_V | MPCRL_SENS_PI (the difference to `solve` is small_sens_kernel; the linear system at
                   N 40 runs lq_solve_kernel, which computes them inside the solve launch)
  state: value     mpcrl_state_sens, dV/dx0 alone (stage0_grad_kernel)
  state: policy    mpcrl_state_sens, du0*/dx0 alone (small_state_sens_kernel: linearisation, one adjoint solve, no parameter jets)
  state: both      mpcrl_state_sens, both
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
        for k, f in fns.items():
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
        sys.exit("state_sens.py measures on the GPU; none found")
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
    cases = (("cartpole N 20", cartpole_ocp(), rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.5])),
             ("linear N 40", linear_system_ocp(N=40), np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.2, 0.5, B)])))
    for name, ocp, x0 in cases:
        mpc = MPCBatch(ocp, B, device=dev)
        x0 = torch.tensor(x0, device=dev)
        kw = dict(dtype=torch.float64, device=dev)
        u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
        dVp, dpip = torch.empty((B, ocp.n_p), **kw), torch.empty((B, ocp.nu, ocp.n_p), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        dV, dpi = torch.empty((B, ocp.nx), **kw), torch.empty((B, ocp.nu, ocp.nx), **kw)
        mpc.solve(x0, cold=True)      # (the packing order of the batch, once; the timed calls below keep it)

        def solve(flags):
            mpc._call("mpcrl_solve", x0, None, flags | _lib.COLD, u0, V, dVp if flags else None, dpip if flags else None, status, iters)

        r = ab({"solve": lambda: solve(0), "solve+dp": lambda: solve(_lib.SENS_V | _lib.SENS_PI),
                "state: value": lambda: mpc._call("mpcrl_state_sens", 0, dV, None, None),
                "state: policy": lambda: mpc._call("mpcrl_state_sens", 0, None, None, dpi),
                "state: both": lambda: mpc._call("mpcrl_state_sens", 0, dV, None, dpi)}, args.repeats)
        torch.cuda.synchronize()
        ok = int(((status == 0) | (status == 2)).sum())
        say(f"{name}, B {B} ({ok} solved, du0*/dx0 finite on {int(torch.isfinite(dpi).all(-1).all(-1).sum())}): "
            + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
