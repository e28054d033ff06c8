"""What the bound outputs of include/mpcrl_bound_ext.h cost beside the trajectory VJP they extend.

    timeout -k 10 600 python profiles/microbench/bound_vjp.py [--out FILE] [--repeats 30] [--parent PARENT.so] [--commit NAME]

One process, HIP events around one eager call (its launch overhead is inside every figure), the calls alternating repeat by repeat
after warm-up; median (min) in microseconds.
  * cartpole N 20 and linear system N 40, B 4096, after a cold solve: mpcrl_traj_vjp (g_x0, g_theta), mpcrl_bound_vjp with all four
    outputs, mpcrl_bound_vjp with the bound outputs alone, mpcrl_bound_value_grad; the x0 are drawn inside the tightened box of the
    fixture G13, so that control and state rows are active and the cartpole's extrapolation runs.  With --parent, a library built from
    the parent commit (csrc/Makefile OUT=...) is loaded beside this one through ctypes, given the same handle set-up, solve and
    cotangent, and its mpcrl_traj_vjp alternates with the others: whether mpcrl_traj_vjp itself moved, and whether its bits did.
  * chain of masses n_mass 5 and 7, N 40, B 1024, after a solve with sens_pi: mpcrl_chain_traj_vjp against mpcrl_chain_bound_vjp with
    all four outputs.
Nothing is asserted about the times."""
import argparse
import ctypes as C
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


class OtherBuild:
    """A handle of another build of the library, called through ctypes directly (this package's binding stays on its own build)."""

    def __init__(self, path, ocp, B, dev):
        self.lib, self.dev = C.CDLL(path), dev
        spec, keep = ocp.c_spec()
        self.h = C.c_void_p()
        self.call("mpcrl_create", C.byref(spec), B, dev.index, C.byref(self.h), handle=False, stream=False)
        del keep
        self.theta = torch.as_tensor(ocp.p0, dtype=torch.float64, device=dev).contiguous()
        self.call("mpcrl_set_theta", self.theta, ocp.n_p, 0)

    def call(self, name, *args, handle=True, stream=True):
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        argv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else (C.c_void_p(None) if a is None else a) for a in args]
        if stream:
            argv.append(C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        rc = fn(*(([self.h] if handle else []) + argv))
        if rc < 0:
            raise RuntimeError(f"{name} of the other build failed with {rc}")

    def close(self):
        self.call("mpcrl_destroy", stream=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--parent", default=None, help="libmpcrl_hip.so built from the parent commit")
    ap.add_argument("--commit", default="the working tree", help="what the figures are labelled as measured on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bound_vjp.py measures on the GPU; none found")
    from mpc4rl_amd import MPCBatch, _lib, cartpole_ocp, chain_mass_ocp, linear_system_ocp
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    kw = dict(dtype=torch.float64, device=dev)
    B = 4096
    rng = np.random.default_rng(0)
    xb = [0.6, 1.0, 0.4, 1.5]
    cases = (("cartpole N 20", cartpole_ocp(N=20, tf=2.0), rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.5]),
              ([-8.0], [8.0], [-8.0] + [-v for v in xb], [8.0] + xb, [-v for v in xb], xb)),
             ("linear N 40", linear_system_ocp(N=40), np.column_stack([rng.uniform(0.1, 0.9, B), rng.uniform(-0.4, 0.4, B)]),
              ([-0.3], [0.3], [-0.3, -1.0, -1.0], [0.3, 1.0, 1.0], [-1e30] * 2, [1e30] * 2)))
    for name, ocp, x0n, bounds in cases:
        mpc = MPCBatch(ocp, B, device=dev)
        for which, (lo, hi) in zip((_lib.BOUNDS_U0, _lib.BOUNDS_STAGE, _lib.BOUNDS_TERMINAL), zip(bounds[0::2], bounds[1::2])):
            mpc.set_bounds(which, lo, hi)
        x0 = torch.tensor(x0n, **kw)
        u0, V = torch.empty((B, ocp.nu), **kw), torch.empty((B,), **kw)
        status, iters = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        nb = (B, ocp.N + 1, ocp.nu + ocp.nx)
        g_x0, g_th, g_lb, g_ub = torch.empty((B, ocp.nx), **kw), torch.empty((B, ocp.n_p), **kw), torch.empty(nb, **kw), torch.empty(nb, **kw)
        gX = torch.tensor(rng.standard_normal((B, ocp.N + 1, ocp.nx)), **kw)
        gU = torch.tensor(rng.standard_normal((B, ocp.N, ocp.nu)), **kw)
        mpc._call("mpcrl_set_launch_mode", -1)      # the plain launch on both builds: the same iterate to work on
        mpc._call("mpcrl_solve", x0, None, _lib.COLD, u0, V, None, None, status, iters)
        fns = {"traj_vjp": lambda: mpc._call("mpcrl_traj_vjp", 0, gX, gU, g_x0, g_th),
               "bound_vjp (4 outputs)": lambda: mpc._call("mpcrl_bound_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub),
               "bound_vjp (g_lb, g_ub)": lambda: mpc._call("mpcrl_bound_vjp", 0, gX, gU, None, None, g_lb, g_ub),
               "bound_value_grad": lambda: mpc._call("mpcrl_bound_value_grad", 0, g_lb, g_ub)}
        other = None
        if args.parent:
            other = OtherBuild(args.parent, ocp, B, dev)
            for which, (lo, hi) in zip((_lib.BOUNDS_U0, _lib.BOUNDS_STAGE, _lib.BOUNDS_TERMINAL), zip(bounds[0::2], bounds[1::2])):
                lo, hi = np.asarray(lo, float), np.asarray(hi, float)
                other.call("mpcrl_set_bounds", int(which), C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), stream=False)
            ou0, oV, ost, oit = torch.empty_like(u0), torch.empty_like(V), torch.empty_like(status), torch.empty_like(iters)
            p_x0, p_th = torch.empty_like(g_x0), torch.empty_like(g_th)
            other.call("mpcrl_set_launch_mode", -1, stream=False)
            other.call("mpcrl_solve", x0, None, int(_lib.COLD), ou0, oV, None, None, ost, oit)
            fns["traj_vjp of the parent build"] = lambda: other.call("mpcrl_traj_vjp", 0, gX, gU, p_x0, p_th)
        r = ab(fns, args.repeats)
        mpc._call("mpcrl_bound_vjp", 0, gX, gU, g_x0, g_th, g_lb, g_ub)
        torch.cuda.synchronize()
        bnd = mpc.get_iterate()[3]
        nz = int(((bnd[:, 2:4] < 1e-8) & (bnd[:, 0:2] > 1e-6)).any((1, 2, 3)).sum())
        capped = int((bnd[:, 0:2, :, ocp.nu:] / bnd[:, 2:4, :, ocp.nu:] > 1e9).any((1, 2, 3)).sum())
        say(f"{name}, B {B} ({int((status == 0).sum())} solved, {nz} with an active row, {capped} with a state row above the cap): "
            + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
        say(f"{name}: the bound outputs add {r['bound_vjp (4 outputs)'][0] - r['traj_vjp'][0]:+8.1f} us to traj_vjp "
            f"({r['bound_vjp (4 outputs)'][0] / r['traj_vjp'][0]:5.2f} x); {2 * nb[1] * nb[2] * 8} bytes of stores per instance")
        if other is not None:
            torch.cuda.synchronize()
            t_x0, t_th = torch.empty_like(g_x0), torch.empty_like(g_th)
            mpc._call("mpcrl_traj_vjp", 0, gX, gU, t_x0, t_th)
            torch.cuda.synchronize()
            eq = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((t_x0, p_x0), (t_th, p_th)))
            say(f"{name}: traj_vjp against the parent build {r['traj_vjp'][0] - r['traj_vjp of the parent build'][0]:+8.1f} us "
                f"({r['traj_vjp'][0] / r['traj_vjp of the parent build'][0]:5.3f} x); outputs bit-identical to the parent's: {eq}")
            other.close()
    B = 1024
    for n_mass in (5, 7):
        ocp = chain_mass_ocp(n_mass=n_mass, N=40)
        mpc = MPCBatch(ocp, B, device=dev)
        x0 = np.tile(ocp.x0, (B, 1)) + rng.normal(0.0, 0.05, (B, ocp.nx))
        res = mpc.solve(x0, sens_pi=True, cold=True)
        nb = (B, ocp.N + 1, ocp.nu + ocp.nx)
        g_x0, g_th, g_lb, g_ub = torch.empty((B, ocp.nx), **kw), torch.empty((B, ocp.n_p), **kw), torch.empty(nb, **kw), torch.empty(nb, **kw)
        gX = torch.tensor(rng.standard_normal((B, ocp.N + 1, ocp.nx)), **kw)
        gU = torch.tensor(rng.standard_normal((B, ocp.N, ocp.nu)), **kw)
        st = res.status
        r = ab({"chain_traj_vjp": lambda: mpc._call("mpcrl_chain_traj_vjp", 0, st, gX, gU, g_x0, g_th),
                "chain_bound_vjp (4 outputs)": lambda: mpc._call("mpcrl_chain_bound_vjp", 0, st, gX, gU, g_x0, g_th, g_lb, g_ub),
                "chain_bound_vjp (g_lb, g_ub)": lambda: mpc._call("mpcrl_chain_bound_vjp", 0, st, gX, gU, None, None, g_lb, g_ub)}, args.repeats)
        torch.cuda.synchronize()
        say(f"chain n_mass {n_mass} N 40, B {B} ({int((st == 0).sum())} solved), after a solve with sens_pi: "
            + ", ".join(f"{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
        say(f"chain n_mass {n_mass}: the bound outputs (one launch more) add {r['chain_bound_vjp (4 outputs)'][0] - r['chain_traj_vjp'][0]:+8.1f} us "
            f"({r['chain_bound_vjp (4 outputs)'][0] / r['chain_traj_vjp'][0]:5.2f} x)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
