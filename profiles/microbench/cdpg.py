"""What the deterministic policy gradient with a compatible critic costs beside Q-learning, and what it does to the closed-loop cost.

    python profiles/microbench/cdpg.py [--out FILE] [--repeats 50] [--episodes 10] [--commit NAME] [--skip-episodes]

(a) mpcrl_cdpg_terms against mpcrl_qlearning_td_gn on synthetic tables of the same shapes, one launch between two HIP events, the two
    kernels alternating repeat by repeat, after warm-up; median (min) in microseconds.  Tables: T 102, E 4096 (4096 x 100 terms), K 12,
    one control (the linear system's shape at a large batch), and T 6, E 256 (1024 terms), K 40, three controls (the chain's, n_mass 5;
    the Q-learning table has n_p 499 there).  One in ten solves has failed.  The launch overhead of an eager call is inside both figures.
(b) mpcrl_cdpg_apply (plain and natural) against mpcrl_qlearning_gn_apply at K 12 and K 40, the same way.
(c) an eager episode of each plant, policy gradient against Q-learning (method="gradient") at the same E, T and horizon, lr 0 on both
    sides (theta stays put: every episode is the same work): wall time around a call that ends in a synchronise, median of --repeats / 10
    episodes after one warm-up episode.
(d) --episodes episodes on the linear system (E 256, T 50) and on the chain at n_mass 5, N 40 (E 128, T 20; plant m x 1.1, D x 0.9,
    theta_bounds = chain_theta_bounds(ocp)), natural on and off at two lr, with a small trust_radius, and lr 0 as the control (the same
    seeds: what the cost does with theta fixed): the mean closed-loop cost per environment and episode, the clipped entries, the code."""
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


def episode_ms(learner, n):
    learner.run_episode()                   # warm-up: lazy initialisation, the solves' launch shape
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        learner.run_episode()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--commit", default="the working tree", help="what the figures are labelled as measured on")
    ap.add_argument("--skip-episodes", action="store_true", help="(a) and (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cdpg.py measures on the GPU; none found")
    import mpc4rl_amd as m
    from mpc4rl_amd import _lib
    from mpc4rl_amd.problems import chain_param_layout
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                        # kept as it grows: a run that is cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(f"# measured on {args.commit}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"# (a), (b): HIP events around one eager call, {args.repeats} interleaved repeats after warm-up, microseconds: median (min)")
    for T, E, n_p, K, nu in ((102, 4096, 12, 12, 1), (6, 256, 499, 40, 3)):
        g = torch.Generator(device=dev).manual_seed(T)
        M = (T - 2) * E
        rn = lambda *s: torch.randn(*s, generator=g, **f64)
        st = (torch.rand(T, E, generator=g, device=dev) < 0.1).to(torch.int32) * 2
        cost, live = torch.rand(T, E, generator=g, **f64), torch.ones(T, E, dtype=torch.uint8, device=dev)
        Vt, U0, Jt, act = rn(T, E), rn(T, E, nu), rn(T, E, nu, K), rn(T, E, nu)
        q, dq = rn(T - 1, E), rn(T - 1, E, n_p)
        sv = torch.zeros(T - 1, E, dtype=torch.int32, device=dev)
        idx = torch.arange(K, dtype=torch.int32, device=dev)
        td, valid = torch.zeros(T - 2, E, **f64), torch.zeros(T - 2, E, dtype=torch.uint8, device=dev)
        ws1 = torch.zeros(lib.mpcrl_qlearning_gn_workspace_bytes(T, E, K), dtype=torch.uint8, device=dev)
        ws2 = torch.zeros(lib.mpcrl_cdpg_workspace_bytes(T, E, K), dtype=torch.uint8, device=dev)
        m1, m2 = torch.zeros(K * (K + 1) // 2 + K + 2, **f64), torch.zeros(K * (K + 1) + K + 2, **f64)

        def gn():
            assert lib.mpcrl_qlearning_td_gn(_p(q), _p(Vt[: T - 1]), _p(dq), _p(st[: T - 1]), _p(sv), _p(cost), _p(live), T, E, n_p, 0.99, _p(idx), K,
                                             _p(ws1), _p(td), _p(valid), _p(m1), stream()) == 0

        def terms():
            assert lib.mpcrl_cdpg_terms(_p(Vt), _p(U0), _p(Jt), _p(st), _p(act), _p(cost), _p(live), T, E, nu, K, 0.99, _p(ws2), _p(td), _p(valid),
                                        _p(m2), stream()) == 0

        r = ab({"qlearning_td_gn": gn, "cdpg_terms": terms}, args.repeats)
        mb = T * E * nu * K * 8 / 2**20
        say(f"(a) {M} terms, K {K}, nu {nu} (J table {mb:.1f} MiB, dQ/dp table {(T - 1) * E * n_p * 8 / 2**20:.1f} MiB, valid {int(m2[-1])}): "
            + ", ".join(f"mpcrl_{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()))
        theta, step, w = torch.zeros(n_p, **f64), torch.zeros(n_p, **f64), torch.zeros(K, **f64)
        active, info = torch.zeros(K, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)

        def gn_apply():
            assert lib.mpcrl_qlearning_gn_apply(_p(m1), K, _p(idx), n_p, 0.0, 1e-3, _p(theta), _p(step), _p(info), stream()) == 0

        def apply(natural):
            return lambda: lib.mpcrl_cdpg_apply(_p(m2), K, _p(idx), n_p, 0.0, 1e-3, natural, None, None, None, float("inf"), _p(theta), _p(step), _p(w),
                                                _p(active), _p(info), stream())

        r = ab({"qlearning_gn_apply": gn_apply, "cdpg_apply": apply(0), "cdpg_apply (natural)": apply(1)}, args.repeats)
        say(f"(b) K {K}: " + ", ".join(f"mpcrl_{k} {med:8.1f} ({mn:8.1f}) us" for k, (med, mn) in r.items()) + f"; info {int(info[0])}")
    if args.skip_episodes:
        return

    def chain(n_mass, N, E, seed=1):
        ocp = m.chain_mass_ocp(n_mass, N=N)
        off = chain_param_layout(n_mass)[4]
        p = torch.tensor(ocp.p0)
        p[off["m"][0]: off["m"][1]] *= 1.1
        p[off["D"][0]: off["D"][1]] *= 0.9
        return ocp, (lambda: m.BatchedChainMassEnv(E, ocp, device=dev, p=p, w_std=0.01, seed=seed))

    n_ep = max(3, args.repeats // 10)
    say(f"# (c) one eager episode, lr 0, wall ms: median (min) of {n_ep} after a warm-up episode; Q-learning is method='gradient'")
    lin, cp = m.linear_system_ocp(), m.cartpole_ocp()
    ch, ch_env = chain(5, 40, 256)
    plants = [("linear   E 4096 T 100", lambda: m.LinearQLearning(lin, m.BatchedLinearSystemEnv(4096, device=dev, seed=5), 100, lr=0.0, noise_scale=0.1, seed=6),
               lambda: m.LinearPolicyGradient(lin, m.BatchedLinearSystemEnv(4096, device=dev, seed=5), 100, lr=0.0, noise_scale=0.1, seed=6)),
              ("cartpole E 1024 T 50 ", lambda: m.CartpoleQLearning(cp, m.BatchedCartPoleSwingUpEnv(1024, device=dev, seed=5), 50, lr=0.0, seed=6),
               lambda: m.CartpolePolicyGradient(cp, m.BatchedCartPoleSwingUpEnv(1024, device=dev, seed=5), 50, lr=0.0, seed=6)),
              ("chain n_mass 5 N 40 E 256 T 5", lambda: m.ChainQLearning(ch, ch_env(), 5, lr=0.0, noise_scale=0.05, seed=2),
               lambda: m.ChainPolicyGradient(ch, ch_env(), 5, lr=0.0, noise_scale=0.05, seed=2))]
    for name, make_q, make_pg in plants:
        res = []
        for make in (make_q, make_pg):
            learner = make()
            res.append(episode_ms(learner, n_ep))
            del learner
            torch.cuda.empty_cache()
        say(f"(c) {name}: Q-learning {res[0][0]:8.1f} ({res[0][1]:8.1f}) ms, policy gradient {res[1][0]:8.1f} ({res[1][1]:8.1f}) ms")
    say(f"# (d) {args.episodes} episodes each, eager: mean closed-loop cost per environment and episode (EpisodeStats.total_cost), mean delta, "
        "clipped entries, code; lr 0 is the control on the same seeds")
    ch, ch_env = chain(5, 40, 128)
    runs = [("linear E 256 T 50, trust_radius 0.05", (1e-2, 1e-1),
             lambda **kw: m.LinearPolicyGradient(lin, m.BatchedLinearSystemEnv(256, device=dev, seed=5), 50, noise_scale=0.1, seed=6, trust_radius=0.05, **kw)),
            ("chain n_mass 5 N 40 E 128 T 20, m x 1.1, D x 0.9, chain_theta_bounds, trust_radius 0.02", (1e-2, 1e-1),
             lambda **kw: m.ChainPolicyGradient(ch, ch_env(), 20, noise_scale=0.05, seed=2, theta_bounds=m.chain_theta_bounds(ch), trust_radius=0.02, **kw))]
    for name, lrs, make in runs:
        for natural, lr in [(False, 0.0)] + [(nat, lr) for nat in (False, True) for lr in lrs]:
            pg = make(lr=lr, natural=natural)
            costs = []
            for ep in range(args.episodes):
                st = pg.run_episode()
                costs.append(st.total_cost)
                say(f"(d) {name}: natural {natural!s:5s} lr {lr:g} episode {ep}: cost {st.total_cost:.6e}, mean delta {st.td_error_mean: .3e}, "
                    f"valid {st.converged_fraction:.4f}, |step| {float(st.step.norm()):.3e}, clipped {st.gn_active} of {pg.K}, info {st.gn_info}")
            h = len(costs) // 2
            say(f"(d) {name}: natural {natural!s:5s} lr {lr:g}: mean cost of the first {h} episodes {statistics.mean(costs[:h]):.6e}, "
                f"of the last {len(costs) - h} {statistics.mean(costs[h:]):.6e}")
            del pg
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
