"""What mpcrl_traj_jvp (include/mpcrl_traj_jvp_ext.h) costs beside mpcrl_traj_vjp and a solve on the same handle.

    timeout -k 10 300 python profiles/microbench/traj_jvp.py [--out FILE] [--repeats 30] [--commit NAME]

Cartpole N 20 and linear system N 40, B 4096, one process, HIP events around one eager call (its launch overhead is inside every
figure), the calls alternating repeat by repeat after warm-up; median (min) in microseconds.  Per repeat, in this order:
  solve        mpcrl_solve, cold, no sensitivities
  jvp R=1      mpcrl_traj_jvp after it, one random direction in (x0, theta), dX and dU
  jvp R=full   the same with R = nx + n_diff directions (cartpole 7, linear system 14): what the full Jacobian costs
  vjp          mpcrl_traj_vjp, one random cotangent over all of (X, U), g_x0 and g_theta
The closing lines give R=full against R separate R=1 calls, and against the (N + 1) nx + N nu calls of mpcrl_traj_vjp the same
Jacobian costs by the backward mode (104 at cartpole N 20, 122 at linear N 40).  Nothing is asserted about the times."""
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
        sys.exit("traj_jvp.py measures on the GPU; none found")
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
        N, nx, nu, n_p = ocp.N, ocp.nx, ocp.nu, ocp.n_p
        Rf = nx + mpc.n_diff()
        x0 = torch.tensor(x0n, **kw)
        u0, V = torch.empty((B, nu), **kw), torch.empty((B,), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        g_x0, g_th = torch.empty((B, nx), **kw), torch.empty((B, n_p), **kw)
        gX, gU = torch.tensor(rng.standard_normal((B, N + 1, nx)), **kw), torch.tensor(rng.standard_normal((B, N, nu)), **kw)
        vx, vp = torch.tensor(rng.standard_normal((B, Rf, nx)), **kw), torch.zeros((B, Rf, n_p), **kw)
        vp[..., :mpc.n_diff()] = torch.tensor(rng.standard_normal((B, Rf, mpc.n_diff())), **kw)
        vx1, vp1 = vx[:, :1].contiguous(), vp[:, :1].contiguous()
        dX, dU = torch.empty((B, Rf, N + 1, nx), **kw), torch.empty((B, Rf, N, nu), **kw)
        dX1, dU1 = torch.empty((B, 1, N + 1, nx), **kw), torch.empty((B, 1, N, nu), **kw)
        r = ab({"solve": lambda: mpc._call("mpcrl_solve", x0, None, _lib.COLD, u0, V, None, None, status, iters),
                "jvp R=1": lambda: mpc._call("mpcrl_traj_jvp", 0, 1, vx1, vp1, dX1, dU1),
                f"jvp R={Rf}": lambda: mpc._call("mpcrl_traj_jvp", 0, Rf, vx, vp, dX, dU),
                "vjp": lambda: mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th)}, args.repeats)
        torch.cuda.synchronize()
        ok = int((status == 0).sum())
        say(f"{name}, B {B} ({ok} solved, dX finite on {int(torch.isfinite(dX).all(-1).all(-1).all(-1).sum())}): "
            + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
        one, full, vjp = r["jvp R=1"][0], r[f"jvp R={Rf}"][0], r["vjp"][0]
        nw = (N + 1) * nx + N * nu
        say(f"{name}: R={Rf} / ({Rf} x R=1) {full / (Rf * one):5.2f}; R=1 / vjp {one / vjp:5.2f}; the Jacobian: R={Rf} / ({nw} x vjp) "
            f"{full / (nw * vjp):6.3f}; R={Rf} / solve {full / r['solve'][0]:5.2f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
