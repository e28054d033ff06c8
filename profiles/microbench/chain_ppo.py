"""What a roll-out step and a minibatch of PPO on the chain of masses cost (BatchedPPO with chain_mass_ocp, eager), in one process.

    python profiles/microbench/chain_ppo.py [--out FILE] [--repeats 20] [--n-mass 5] [--horizon 40] [--envs 256] [--steps 4] [--batch 256]

The default configuration is n_mass 5, N 40, E 256, T 4, minibatch 256.
(a) one roll-out step: the policy's solve over E chains, the value network's forward, the eps draw, the collect launch
    (mpcrl_ppo_chain_collect) and the copy of the E iterates into the tables — the cold first step, and the warm second step;
(b) one minibatch: the iterate rows into the minibatch handle, ONE solve with du0*/dp ([3][n_p] per row), mpcrl_ppo_surrogate_grad_nu, the
    two apply launches, set_theta on both handles and the value network's step.
lr = 0, so theta and log_std stay where they are, and before every timed roll-out step the environments, the observation, the step
counts and the cold mask are put back to the start of the same roll-out (outside the timed region), so every repeat runs the same step;
the minibatch runs on the tables of one whole roll-out, the same rows every time.  Every figure is HIP-event time after warm-up, one call
between two events; the median and the minimum over the repeats are reported in ms.  Host launch overhead is inside the figures on
purpose: the loop pays it."""
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


def repeat(fn, repeats, before, warmup=2):
    """before() runs untimed ahead of every call; (median, min) in ms."""
    t = []
    for i in range(warmup + repeats):
        before()
        torch.cuda.synchronize()
        ms = timed(fn)
        if i >= warmup:
            t.append(ms)
    return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n-mass", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    if args.repeats < 20:
        sys.exit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("chain_ppo.py measures on the GPU; none found")
    from mpc4rl_amd import BatchedChainMassEnv, BatchedPPO, chain_mass_ocp
    from mpc4rl_amd.problems import chain_param_layout
    dev = torch.device("cuda", 0)
    E, T, B = args.envs, args.steps, args.batch
    ocp = chain_mass_ocp(args.n_mass, N=args.horizon)
    off = chain_param_layout(args.n_mass)[4]
    p = torch.tensor(ocp.p0)
    p[off["m"][0]: off["m"][1]] *= 1.1                        # a plant that is not the model
    p[off["D"][0]: off["D"][1]] *= 0.9
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; HIP events, {args.repeats} repeats of one call, ms per call: median (min)")
    say(f"# n_mass {args.n_mass}, N {args.horizon}, n_p {ocp.n_p}, E {E}, T {T}, minibatch {B}, episode_length {T}")
    ppo = BatchedPPO(ocp, BatchedChainMassEnv(E, ocp, device=dev, p=p, w_std=0.01, seed=1), n_steps=T, batch_size=B, n_epochs=1, episode_length=T,
                     lr=0.0, log_std_init=-1.0, seed=2)
    ws = ppo.workspace_bytes()
    tables = sum(t.numel() * t.element_size() for t in ppo.iters)
    say(f"# workspace: roll-out handle {ws[0] / 2**20:.1f} MiB, minibatch handle {ws[1] / 2**20:.1f} MiB ({ws[1] / B / 2**20:.2f} MiB per instance), "
        f"stored-iterate tables {tables / 2**20:.1f} MiB ({tables / (T * E) / 1024:.1f} KiB per row)")
    start = ppo.env.state.clone()
    ppo.collect()                                              # fills the tables the minibatch is timed on
    torch.cuda.synchronize()
    say(f"# one roll-out: accepted solves {float(ppo.OK.double().mean()):.4f}, mean cost {float(ppo.REW.mean()) / ppo.reward_scale:.4f}")

    def rewind():                                              # the same cold first step every time
        ppo.env.state.copy_(start), ppo.obs.copy_(start), ppo.steps.zero_(), ppo.ended.fill_(1)

    def warm_before():                                         # one untimed cold step, so that the timed one is the warm second step
        rewind()
        ppo._collect_step(0)

    med, mn = repeat(lambda: ppo._collect_step(0), args.repeats, rewind)
    say(f"(a) roll-out step (cold solve of {E} + value + collect + iterate rows)  {med:9.3f} ({mn:9.3f}) ms")
    med, mn = repeat(lambda: ppo._collect_step(1), args.repeats, warm_before)
    say(f"(a) roll-out step (warm solve of {E} + value + collect + iterate rows)  {med:9.3f} ({mn:9.3f}) ms")
    rewind()
    ppo.collect()
    idx = torch.randperm(T * E, generator=torch.Generator().manual_seed(3))[:B].to(dev).contiguous()
    med, mn = repeat(lambda: ppo._minibatch(idx), args.repeats, lambda: None)
    say(f"(b) minibatch (solve of {B} with du0/dp + surrogate + apply + value step) {med:9.3f} ({mn:9.3f}) ms")
    st = ppo.last_stats()
    say(f"# the last minibatches: valid_fraction {st['valid_fraction']:.4f}, mean_ratio {st['mean_ratio']:.6f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
