"""What an episode of Q-learning on the linear system costs on library kernels (LinearQLearning, eager and as HIP graphs) and as framework
glue (BatchedQLearning), and what a PPO iteration on the same plant costs, in one process.

    python profiles/microbench/linear_learners.py [--out FILE] [--repeats 20] [--envs 4096] [--steps 100]

(a) one run_episode() of E environments x T steps: LinearQLearning eager, LinearQLearning after enable_graphs(), BatchedQLearning (T
    roll-out solves, the learning sweep's two solves over E (T - 1) samples, the TD step, the parameter step);
(b) one BatchedPPO.learn(1) on the linear system at E environments, n_steps = 8, batch_size = E, n_epochs = 1, episode_length = 100, with
    the value function as framework launches and as library kernels.
Every figure is HIP-event time after warm-up, one call between two events, the variants alternating repeat by repeat; the median and
the minimum over the repeats are reported in ms.  Host launch overhead and the host reads of run_episode()'s statistics are inside these
figures on purpose: the loops pay them."""
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


def ab(fns, repeats, warmup=2):
    """fns: {label: callable}.  Interleaved rounds; {label: (median, min) in ms}."""
    for _ in range(warmup):
        for f in fns.values():
            timed(f)
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t[k].append(timed(f))
    return {k: (statistics.median(v), min(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    if args.repeats < 20:
        sys.exit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("linear_learners.py measures on the GPU; none found")
    from mpc4rl_amd import BatchedLinearSystemEnv, BatchedPPO, BatchedQLearning, LinearQLearning, linear_system_ocp
    dev = torch.device("cuda", 0)
    E, T = args.envs, args.steps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; HIP events, {args.repeats} interleaved repeats of one call, "
        "ms per call: median (min)")
    # (a) lr = 0: every repeat runs the same episode at the same parameters
    ocp = linear_system_ocp()
    eager = LinearQLearning(ocp, BatchedLinearSystemEnv(E, device=dev, seed=1), T, lr=0.0)
    graphs = LinearQLearning(ocp, BatchedLinearSystemEnv(E, device=dev, seed=1), T, lr=0.0)
    graphs.enable_graphs()
    torch_form = BatchedQLearning(ocp, BatchedLinearSystemEnv(E, device=dev, seed=1), T, lr=0.0, device=dev)
    r = ab({"LinearQLearning, eager": eager.run_episode, "LinearQLearning, graphs": graphs.run_episode, "BatchedQLearning": torch_form.run_episode},
           args.repeats)
    base = r["BatchedQLearning"][0]
    for k, (med, mn) in r.items():
        say(f"(a) run_episode, E {E} x T {T}: {k:<26s} {med:9.2f} ({mn:9.2f}) ms   {base / med:5.2f}x")
    del eager, graphs, torch_form
    # (b)
    def learner(flag):
        return BatchedPPO(ocp, BatchedLinearSystemEnv(E, device=dev, seed=3), n_steps=8, batch_size=E, n_epochs=1, lr=1e-4, log_std_init=-1.0, seed=11,
                          value_kernels=flag, episode_length=100)
    ppo = {flag: learner(flag) for flag in (False, True)}
    r = ab({k: (lambda p=p: p.learn(1)) for k, p in ppo.items()}, args.repeats)
    for flag, (med, mn) in r.items():
        st = ppo[flag].last_stats()
        say(f"(b) BatchedPPO.learn(1), E {E}, T 8, B {E}, 1 epoch, value_kernels={flag!s:<5s} {med:9.2f} ({mn:9.2f}) ms   "
            f"valid_fraction {st['valid_fraction']:.4f}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
