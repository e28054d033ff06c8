"""What the box-constrained Gauss-Newton step costs beside the plain one, and what bounds and a trust region do to the chain run that the
plain step could not survive (profiles/qlearning_gn_microbench.txt, part (c)).

    python profiles/microbench/qlearning_gn_box.py [--out FILE] [--repeats 50] [--episodes 10] [--commit NAME]

(a) mpcrl_qlearning_gn_apply_box against mpcrl_qlearning_gn_apply on the same message, one launch between two HIP events, the two
    alternating repeat by repeat, after warm-up; median (min) in microseconds.  K 12, 40 and 64; G = g' g of 4 K + 3 correlated random
    terms, damping 1e-3, lr 1; at each K three trust regions (scale 1) around the unconstrained step d0: 10 max|d0| (no bound active), a
    radius found by bisection with the torch statement that leaves about K / 2 entries active, and 1e-8 (all active); `active` and
    `iterations` are what the launch reported.  theta is restored between launches outside the timed window.  The launch overhead of an eager call is inside both figures.
(b) --episodes episodes of ChainQLearning at n_mass 5, N 40, E 256, T 5, plant m x 1.1 and D x 0.9 — run (c) of qlearning_gn.py, the same
    chain, plant and seeds — with method="gauss_newton", damping 1e-3, theta_bounds = chain_theta_bounds(ocp) and (lr, trust_radius) =
    (1, 0.02), (1, 0.1), (0.5, 0.02), (0.5, 0.1): the columns of that run (max |step_a / theta_a| over the entries of theta that are not
    0), plus gn_active and gn_iterations."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
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


def ab(fns, repeats, between, warmup=5):
    t = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, f in fns.items():
            between()
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
        sys.exit("qlearning_gn_box.py measures on the GPU; none found")
    from mpc4rl_amd import BatchedChainMassEnv, ChainQLearning, _lib, chain_mass_ocp, chain_theta_bounds, qlearning_gn_box_step
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
    say(f"# (a): HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    for K in (12, 40, 64):
        rng = np.random.default_rng(K)
        M = 4 * K + 3
        g = rng.normal(size=(M, K)) @ (rng.normal(size=(K, K)) / np.sqrt(K) + np.eye(K))
        td = rng.normal(size=M)
        G, b = g.T @ g, g.T @ td
        msg = torch.as_tensor(np.concatenate([G[np.triu_indices(K)], b, [0.0], [float(M)]]))
        inf, one = np.full(K, np.inf), np.ones(K)
        d0 = qlearning_gn_box_step(msg, K, 1.0, 1e-3, -inf, inf, one, np.inf, np.zeros(K))[0].abs()
        msg_d, idx = msg.to(dev), torch.arange(K, dtype=torch.int32, device=dev)
        lo, hi, scale = torch.full((K,), -np.inf, **f64), torch.full((K,), np.inf, **f64), torch.ones(K, **f64)
        theta0 = torch.zeros(K, **f64)
        theta, step = theta0.clone(), torch.zeros(K, **f64)
        active, info = torch.zeros(K, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        n_active = lambda r: int((qlearning_gn_box_step(msg, K, 1.0, 1e-3, -inf, inf, one, r, np.zeros(K))[1] != 0).sum())
        r_lo, r_hi = 1e-8, 10.0 * float(d0.max())                  # all active ... none: bisect (on the host) for about K / 2
        for _ in range(12):
            r_mid = float(np.sqrt(r_lo * r_hi))
            r_lo, r_hi = (r_mid, r_hi) if n_active(r_mid) > K // 2 else (r_lo, r_mid)
        for what, radius in (("no bound active", 10.0 * float(d0.max())), ("about half active", r_hi), ("all active", 1e-8)):
            def plain():
                assert lib.mpcrl_qlearning_gn_apply(_p(msg_d), K, _p(idx), K, 1.0, 1e-3, _p(theta), _p(step), _p(info), stream()) == 0

            def box():
                assert lib.mpcrl_qlearning_gn_apply_box(_p(msg_d), K, _p(idx), K, 1.0, 1e-3, _p(lo), _p(hi), _p(scale), radius, _p(theta), _p(step),
                                                        _p(active), _p(info), stream()) == 0

            r = ab({"gn_apply": plain, "gn_apply_box": box}, args.repeats, lambda: theta.copy_(theta0))
            torch.cuda.synchronize()
            code, its = info.tolist()          # (the box launch is the last one)
            say(f"(a) K {K}, radius {radius:.3e} ({what}): "
                + ", ".join(f"mpcrl_qlearning_{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items())
                + f"; info {code}, active {int((active != 0).sum())} of {K}, iterations {its}")
    n_mass, N, E, T = 5, 40, 256, 5
    ocp = chain_mass_ocp(n_mass, N=N)
    off = chain_param_layout(n_mass)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1
    p[off["D"][0]: off["D"][1]] *= 0.9
    say(f"# (b) ChainQLearning, n_mass {n_mass}, N {N}, E {E}, T {T}, plant m x 1.1, D x 0.9, w_std 0.01, noise_scale 0.05, eager, "
        "theta_bounds = chain_theta_bounds(ocp); mean td^2 over the valid terms, wall ms per episode")
    for lr, radius in ((1.0, 0.02), (1.0, 0.1), (0.5, 0.02), (0.5, 0.1)):
        ql = ChainQLearning(ocp, BatchedChainMassEnv(E, ocp, device=dev, p=p, w_std=0.01, seed=1), T, noise_scale=0.05, seed=2, method="gauss_newton",
                            lr=lr, damping=1e-3, trust_radius=radius, theta_bounds=chain_theta_bounds(ocp))
        for ep in range(args.episodes):
            theta0 = ql.theta.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = ql.run_episode()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            nv = max(1.0, float(ql.valid.sum()))
            moved = (st.step != 0.0) & (theta0 != 0.0)
            rel = float((st.step[moved] / theta0[moved]).abs().max()) if bool(moved.any()) else 0.0
            say(f"(b) gauss_newton lr {ql.lr:g} damping {ql.damping:g} trust_radius {radius:g} episode {ep}: mean td^2 {float((ql.td ** 2).sum()) / nv:.6e}, "
                f"valid {st.converged_fraction:.4f}, |step| {float(st.step.norm()):.3e}, max |step_a / theta_a| {rel:.3e}, gn_info {st.gn_info}, "
                f"gn_active {st.gn_active}, gn_iterations {st.gn_iterations}, {ms:8.1f} ms")
        del ql
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
