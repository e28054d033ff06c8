"""What mpcrl_chain_policy_state_sens (include/mpcrl_chain_ext.h) costs beside the chain solve and its parameter-sensitivity pass.

    python profiles/microbench/chain_state_sens.py [--out FILE] [--repeats 30] [--commit NAME]

Chain of masses n_mass 5 and 7, N 40, B 1024, one process, HIP events around one eager call (its launch overhead is inside every
figure), the calls alternating repeat by repeat after warm-up; median (min) in microseconds.  Per repeat, in this order:
  solve            mpcrl_solve, cold, no sensitivities
  du0*/dx0 (4)     mpcrl_chain_policy_state_sens after it: second-order point pass, exact Hessians, adjoint Riccati solve, contraction
  solve+dp         mpcrl_solve, cold, MPCRL_SENS_V | MPCRL_SENS_PI (the difference to `solve` is the six-launch sensitivity tail)
  du0*/dx0 (1)     mpcrl_chain_policy_state_sens after it: the contraction alone
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
        for k, f in fns.items():      # (in the order given: each du0*/dx0 call follows its solve)
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
        sys.exit("chain_state_sens.py measures on the GPU; none found")
    from mpc4rl_amd import MPCBatch, _lib, chain_mass_ocp
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    B = 1024
    for n_mass in (5, 7):
        ocp = chain_mass_ocp(n_mass=n_mass, N=40)
        mpc = MPCBatch(ocp, B, device=dev)
        x0 = torch.tensor(np.tile(ocp.x0, (B, 1)) + np.random.default_rng(n_mass).normal(0.0, 0.02, (B, ocp.nx)), device=dev)
        kw = dict(dtype=torch.float64, device=dev)
        u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
        dVp, dpip = torch.empty((B, ocp.n_p), **kw), torch.empty((B, ocp.nu, ocp.n_p), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        dpi = torch.empty((B, ocp.nu, ocp.nx), **kw)

        def solve(flags):
            mpc._call("mpcrl_solve", x0, None, flags | _lib.COLD, u0, V, dVp if flags else None, dpip if flags else None, status, iters)

        def state():
            mpc._call("mpcrl_chain_policy_state_sens", 0, status, dpi)

        r = ab({"solve": lambda: solve(0), "du0*/dx0 (4 launches)": state,
                "solve+dp": lambda: solve(_lib.SENS_V | _lib.SENS_PI), "du0*/dx0 (1 launch)": state}, args.repeats)
        torch.cuda.synchronize()
        ok = int(((status == 0) | (status == 2)).sum())
        say(f"chain n_mass {n_mass} N 40, B {B} ({ok} solved, du0*/dx0 finite on {int(torch.isfinite(dpi).all(-1).all(-1).sum())}): "
            + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
