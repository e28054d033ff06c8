"""What a roll-out step and a learning sweep of Q-learning on the chain of masses cost (ChainQLearning, eager and as HIP graphs), in one
process.

    python profiles/microbench/chain_qlearning.py [--out FILE] [--repeats 20] [--n-mass 5] [--horizon 40] [--envs 256] [--steps 5]
    python profiles/microbench/chain_qlearning.py --trace-steps 4        # a few eager roll-out steps and nothing else (for a kernel trace)

The default configuration is n_mass 5, N 40, E 256, T 5: the sweep is then 1024 instances, the benchmark's chain5 batch.
(a) one roll-out step (the policy's solve over E chains + the collect launch): the eager call, and one replay of its captured graph;
(b) one learning sweep (the Q solve and the V solve over E (T - 1) samples + the TD launch): the eager call, and one replay.
lr = 0, and before every timed roll-out step the environments, the observation, the table row and the cold mask are put back to the
start of the same episode (outside the timed region), so every repeat runs the same cold first step; the sweep runs on the tables of one
whole episode.  Every figure is HIP-event time after warm-up, one call between two events, the variants alternating repeat by repeat; the
median and the minimum over the repeats are reported in ms.  Host launch overhead is inside the eager figures on purpose: the loop pays it.

For the kernels' own times, trace `--trace-steps` with the profiler's kernel trace and statistics in a run of its own, and read the
collect kernel's row next to chain_sqp_kernel's."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)          # ms


def ab(fns, repeats, before, warmup=2):
    """fns: {label: callable}.  Interleaved rounds, before(label) run untimed ahead of every call; {label: (median, min) in ms}."""
    t = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, f in fns.items():
            before(k)
            torch.cuda.synchronize()
            ms = timed(f)
            if i >= warmup:
                t[k].append(ms)
    return {k: (statistics.median(v), min(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n-mass", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--trace-steps", type=int, default=0)
    args = ap.parse_args()
    if args.repeats < 20:
        sys.exit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("chain_qlearning.py measures on the GPU; none found")
    from mpc4rl_amd import BatchedChainMassEnv, ChainQLearning, chain_mass_ocp
    from mpc4rl_amd.problems import chain_param_layout
    dev = torch.device("cuda", 0)
    E, T = args.envs, args.steps
    ocp = chain_mass_ocp(args.n_mass, N=args.horizon)
    off = chain_param_layout(args.n_mass)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1                        # a plant that is not the model
    p[off["D"][0]: off["D"][1]] *= 0.9

    def learner(graphs):
        ql = ChainQLearning(ocp, BatchedChainMassEnv(E, ocp, device=dev, p=p, w_std=0.01, seed=1), T, lr=0.0, noise_scale=0.05, seed=2)
        if graphs:
            ql.enable_graphs()
        return ql

    if args.trace_steps:
        ql = learner(False)
        ql._start_episode()
        for _ in range(min(args.trace_steps, T)):
            ql._rollout_step()
        torch.cuda.synchronize()
        print(f"{min(args.trace_steps, T)} eager roll-out steps, n_mass {args.n_mass}, N {args.horizon}, E {E}")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; HIP events, {args.repeats} interleaved repeats of one call, "
        "ms per call: median (min)")
    say(f"# n_mass {args.n_mass}, N {args.horizon}, E {E}, T {T}: the sweep solves {E * (T - 1)} instances")
    ql = {"eager": learner(False), "graphs": learner(True)}
    ws = ql["eager"].workspace_bytes()
    say(f"# workspace: roll-out handle {ws[0] / 2**20:.1f} MiB, sweep handle {ws[1] / 2**20:.1f} MiB ({ws[1] / (E * (T - 1)) / 2**20:.2f} MiB per instance)")
    start = {}
    for k, q in ql.items():
        st = q.run_episode()                                   # fills the tables the sweep is timed on
        say(f"# {k}: one episode, converged_fraction {st.converged_fraction:.4f}, total_cost {st.total_cost:.4f}")
        q._start_episode()
        start[k] = q.env.state.clone()

    def rewind(k):                                             # the same cold first step every time
        q = ql[k]
        q.env.state.copy_(start[k]), q.obs.copy_(start[k]), q.row.zero_(), q.cold.fill_(1)

    step = {"eager": ql["eager"]._rollout_step, "graphs": ql["graphs"]._graphs["rollout"].replay}
    sweep = {"eager": ql["eager"]._sweep, "graphs": ql["graphs"]._graphs["sweep"].replay}
    r = ab(step, args.repeats, rewind)
    for k, (med, mn) in r.items():
        say(f"(a) roll-out step (cold solve of {E} + collect), {k:<7s} {med:9.3f} ({mn:9.3f}) ms")

    def warm_before(k):                                        # one untimed cold step, so that the timed one is the warm second step
        rewind(k)
        step[k]()

    r = ab(step, args.repeats, warm_before)
    for k, (med, mn) in r.items():
        say(f"(a) roll-out step (warm solve of {E} + collect), {k:<7s} {med:9.3f} ({mn:9.3f}) ms")
    r = ab(sweep, args.repeats, lambda k: None)
    for k, (med, mn) in r.items():
        say(f"(b) learning sweep (Q + V solve of {E * (T - 1)} + TD), {k:<7s} {med:9.3f} ({mn:9.3f}) ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
