"""What the cost output of include/mpcrl_cost_ext.h costs beside the bound VJP it extends.

    timeout -k 10 300 python profiles/microbench/cost_vjp.py [--out FILE] [--repeats 30] [--commit NAME]

One process, HIP events around one eager call (its launch overhead is inside every figure), the calls alternating repeat by repeat
after warm-up; median (min) in microseconds.  Cartpole N 20, B 4096, after a cold solve on the x0 of profiles/microbench/bound_vjp.py
(drawn inside the tightened box of the fixtures, so that control and state rows are active and the extrapolation runs):
mpcrl_traj_vjp (g_x0, g_theta), mpcrl_bound_vjp with its four outputs, mpcrl_cost_vjp with all five, mpcrl_cost_vjp with g_cost alone,
and mpcrl_cost_value_grad.  The first four outputs of mpcrl_cost_vjp are compared bit for bit with mpcrl_bound_vjp's.  Nothing is
asserted about the times."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bound_vjp import ab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--commit", default="the working tree", help="what the figures are labelled as measured on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cost_vjp.py measures on the GPU; none found")
    from mpc4rl_amd import MPCBatch, _lib, cartpole_ocp
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured once on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    kw = dict(dtype=torch.float64, device=dev)
    B, N = 4096, 20
    rng = np.random.default_rng(0)
    xb = [0.6, 1.0, 0.4, 1.5]
    ocp = cartpole_ocp(N=N, tf=2.0)
    mpc = MPCBatch(ocp, B, device=dev)
    mpc.set_bounds(_lib.BOUNDS_U0, [-8.0], [8.0])
    mpc.set_bounds(_lib.BOUNDS_STAGE, [-8.0] + [-v for v in xb], [8.0] + xb)
    mpc.set_bounds(_lib.BOUNDS_TERMINAL, [-v for v in xb], xb)
    x0 = torch.tensor(rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.5]), **kw)
    u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
    status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
    nb = (B, N + 1, ocp.nu + ocp.nx)
    g_x0, g_th, g_lb, g_ub, g_c = (torch.empty(s, **kw) for s in ((B, ocp.nx), (B, ocp.n_p), nb, nb, (B, ocp.n_p)))
    gX, gU = torch.tensor(rng.standard_normal((B, N + 1, ocp.nx)), **kw), torch.tensor(rng.standard_normal((B, N, ocp.nu)), **kw)
    mpc._call("mpcrl_set_launch_mode", -1)
    mpc._call("mpcrl_solve", x0, None, _lib.COLD, u0, V, None, None, status, iters)
    r = ab({"traj_vjp": lambda: mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th),
            "bound_vjp (4 outputs)": lambda: mpc._call("mpcrl_bound_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub),
            "cost_vjp (5 outputs)": lambda: mpc._call("mpcrl_cost_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub, g_c),
            "cost_vjp (g_cost)": lambda: mpc._call("mpcrl_cost_vjp", 0, gX, gU, None, None, None, None, g_c),
            "cost_value_grad": lambda: mpc._call("mpcrl_cost_value_grad", 0, g_c)}, args.repeats)
    say(f"cartpole N {N}, B {B} ({int((status == 0).sum())} solved): " + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
    say(f"cartpole N {N}: the cost output adds {r['cost_vjp (5 outputs)'][0] - r['bound_vjp (4 outputs)'][0]:+8.1f} us to bound_vjp "
        f"({r['cost_vjp (5 outputs)'][0] / r['bound_vjp (4 outputs)'][0]:5.2f} x); {ocp.n_p * 8} bytes of stores per instance")
    four = [torch.empty_like(t) for t in (g_x0, g_th, g_lb, g_ub)]
    mpc._call("mpcrl_bound_vjp", 0, gX, gU, *four)
    mpc._call("mpcrl_cost_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub, g_c)
    torch.cuda.synchronize()
    eq = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(four, (g_x0, g_th, g_lb, g_ub)))
    say(f"cartpole N {N}: g_x0, g_theta, g_lb, g_ub of cost_vjp bit-identical to bound_vjp's: {eq}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
