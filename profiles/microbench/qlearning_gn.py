"""What the Gauss-Newton TD kernel costs beside the first-order one, and what the two parameter steps do to the TD error of the chain.

    python profiles/microbench/qlearning_gn.py [--out FILE] [--repeats 50] [--episodes 10] [--commit NAME]

(a) mpcrl_qlearning_td_gn against mpcrl_qlearning_td_grad on the same synthetic tables, one launch between two HIP events, the two
    kernels alternating repeat by repeat, after warm-up; median (min) in microseconds.  Tables: T 102, E 4096 (4096 x 100 terms) with
    n_p 12, K 12 (the linear system's shape at a large batch), and T 6, E 256 (1024 terms) with n_p 499, K 40 (the chain's, n_mass 5).
    One in ten solves of the tables has failed.  The launch overhead of an eager call is inside both figures.
(b) mpcrl_qlearning_gn_apply at K 12 and K 40, the same way.
(c) --episodes episodes of ChainQLearning at n_mass 5, N 40, E 256, T 5, plant m x 1.1 and D x 0.9, with method="gradient" (its default
    lr 1e-6) and method="gauss_newton" at (lr, damping) = (0.5, 1e-3), (0.01, 1e-3), (0.001, 1e-3) and (0.01, 1), from the same seeds: the
    mean td^2 over the valid terms per episode, the step's norm and its largest entry relative to the entry of theta it moves, and the
    wall time of an eager episode (host clock around a call that ends in a synchronise).  A step
    that leaves the region where the OCP solves shows as valid 0 and gn_info -1 from the next episode on."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


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
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--commit", default="the working tree", help="what the figures are labelled as measured on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("qlearning_gn.py measures on the GPU; none found")
    from mpc4rl_amd import BatchedChainMassEnv, ChainQLearning, _lib, chain_mass_ocp
    from mpc4rl_amd.problems import chain_param_layout
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# (a), (b): HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    for T, E, n_p, K in ((102, 4096, 12, 12), (6, 256, 499, 40)):
        g = torch.Generator(device=dev).manual_seed(T)
        M = (T - 2) * E
        q, v = torch.randn(T - 1, E, generator=g, **f64), torch.randn(T - 1, E, generator=g, **f64)
        dq = torch.randn(T - 1, E, n_p, generator=g, **f64)
        sq = (torch.rand(T - 1, E, generator=g, device=dev) < 0.1).to(torch.int32) * 2
        sv = torch.zeros(T - 1, E, dtype=torch.int32, device=dev)
        cost, live = torch.rand(T, E, generator=g, **f64), torch.ones(T, E, dtype=torch.uint8, device=dev)
        idx = torch.arange(K, dtype=torch.int32, device=dev)
        td, valid = torch.zeros(T - 2, E, **f64), torch.zeros(T - 2, E, dtype=torch.uint8, device=dev)
        ws1 = torch.zeros(lib.mpcrl_qlearning_td_workspace_bytes(T, E, n_p), dtype=torch.uint8, device=dev)
        ws2 = torch.zeros(lib.mpcrl_qlearning_gn_workspace_bytes(T, E, K), dtype=torch.uint8, device=dev)
        m1, m2 = torch.zeros(n_p + 2, **f64), torch.zeros(K * (K + 1) // 2 + K + 2, **f64)
        tab = [_p(t) for t in (q, v, dq, sq, sv, cost, live)]

        def grad():
            assert lib.mpcrl_qlearning_td_grad(*tab, T, E, n_p, 0.99, 1e-4, _p(ws1), _p(td), _p(valid), _p(m1), stream()) == 0

        def gn():
            assert lib.mpcrl_qlearning_td_gn(*tab, T, E, n_p, 0.99, _p(idx), K, _p(ws2), _p(td), _p(valid), _p(m2), stream()) == 0

        r = ab({"td_grad": grad, "td_gn": gn}, args.repeats)
        mb = (T - 1) * E * n_p * 8 / 2**20
        say(f"(a) {M} terms, n_p {n_p}, K {K} (dQ/dp table {mb:.1f} MiB, valid {int(m2[-1])}): "
            + ", ".join(f"mpcrl_qlearning_{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
        theta, step, info = torch.zeros(n_p, **f64), torch.zeros(n_p, **f64), torch.zeros(1, dtype=torch.int32, device=dev)

        def apply():
            assert lib.mpcrl_qlearning_gn_apply(_p(m2), K, _p(idx), n_p, 0.0, 1e-3, _p(theta), _p(step), _p(info), stream()) == 0

        med, mn = ab({"apply": apply}, args.repeats)["apply"]
        say(f"(b) mpcrl_qlearning_gn_apply, K {K}: {med:8.1f} ({mn:8.1f}) us, info {int(info)}")
    n_mass, N, E, T = 5, 40, 256, 5
    ocp = chain_mass_ocp(n_mass, N=N)
    off = chain_param_layout(n_mass)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1
    p[off["D"][0]: off["D"][1]] *= 0.9
    say(f"# (c) ChainQLearning, n_mass {n_mass}, N {N}, E {E}, T {T}, plant m x 1.1, D x 0.9, w_std 0.01, noise_scale 0.05, eager; "
        "mean td^2 over the valid terms, wall ms per episode")
    for kw in (dict(method="gradient"), dict(method="gauss_newton", lr=0.5, damping=1e-3), dict(method="gauss_newton", lr=0.01, damping=1e-3),
               dict(method="gauss_newton", lr=0.001, damping=1e-3), dict(method="gauss_newton", lr=0.01, damping=1.0)):
        ql = ChainQLearning(ocp, BatchedChainMassEnv(E, ocp, device=dev, p=p, w_std=0.01, seed=1), T, noise_scale=0.05, seed=2, **kw)
        for ep in range(args.episodes):
            theta0 = ql.theta.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = ql.run_episode()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            nv = max(1.0, float(ql.valid.sum()))
            moved = st.step != 0.0
            rel = float((st.step[moved] / theta0[moved]).abs().max()) if bool(moved.any()) else 0.0
            say(f"(c) {kw['method']:<12s} lr {ql.lr:g} damping {ql.damping:g} episode {ep}: mean td^2 {float((ql.td ** 2).sum()) / nv:.6e}, valid {st.converged_fraction:.4f}, "
                f"|step| {float(st.step.norm()):.3e}, max |step_a / theta_a| {rel:.3e}, gn_info {st.gn_info}, {ms:8.1f} ms")
        del ql
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
