"""What PPO's value function costs as framework launches and as library kernels (BatchedPPO(value_kernels=False / True)), in one process.

    python profiles/microbench/ppo_value_step.py [--out FILE] [--repeats 25] [--inner 20]

(a) policy.predict_values on E = 4096 observations (float64 in, [E, 1] float64 out);
(b) the value step of one minibatch, gradient -> Adam (BatchedPPO._value_step: what _minibatch runs after the policy step), at
    B = 256 and B = 4096 over a roll-out of T E = 8 x 4096 rows;
(c) one learn(1) at E = 4096, n_steps = 8, batch_size = 4096, n_epochs = 1 (8 roll-out solves, 8 minibatch re-solves): reported, the
    value function is a small part of it.
Every figure is HIP-event time after warm-up: a repeat is `inner` back-to-back calls between two events (learn(1): one call), the two
variants alternate repeat by repeat, and the median and the minimum over the repeats are reported per call.  Host launch overhead is
inside these figures on purpose: the framework path is made of launches, and the loop pays them."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # us per call


def ab(fns, repeats, inner, warmup=3):
    """fns: {label: callable}.  Interleaved rounds; {label: (median, min) in us}."""
    for _ in range(warmup):
        for f in fns.values():
            timed(f, inner)
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t[k].append(timed(f, inner))
    return {k: (statistics.median(v), min(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if args.repeats < 20:
        sys.exit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("ppo_value_step.py measures on the GPU; none found")
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedPPO, cartpole_ocp
    dev = torch.device("cuda", 0)
    E, T = 4096, 8
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def learner(B, flag):
        env = BatchedCartPoleSwingUpEnv(E, device=dev, seed=3)
        return BatchedPPO(cartpole_ocp(), env, n_steps=T, batch_size=B, n_epochs=1, lr=1e-4, log_std_init=-1.0, seed=11, value_kernels=flag)

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; HIP events, {args.repeats} interleaved repeats of {args.inner} calls "
        "(learn: 1 call), us per call: median (min)")
    big = {flag: learner(4096, flag) for flag in (False, True)}
    for p in big.values():
        p.collect()                                   # tables and returns of a real roll-out
    torch.cuda.synchronize()

    def row(name, r):
        off, on = r[False], r[True]
        say(f"{name:<46s} framework {off[0]:9.1f} ({off[1]:9.1f})   kernels {on[0]:9.1f} ({on[1]:9.1f})   ratio {off[0] / on[0]:5.2f}x")

    # (a)
    def pv(p):
        def f():
            with torch.no_grad():
                p.policy.predict_values(p.obs)
        return f
    row("(a) predict_values, E = 4096", ab({k: pv(p) for k, p in big.items()}, args.repeats, args.inner))

    def pv_all(p):
        def f():
            with torch.no_grad():
                p.policy.predict_values(p.NEXT.reshape(-1, 4))
        return f
    row("    predict_values, T E = 32768 next states", ab({k: pv_all(p) for k, p in big.items()}, args.repeats, args.inner))

    # (b)
    def vstep(p):
        idx = torch.randperm(T * E, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[: p.B].contiguous()
        obs = p.OBS.reshape(-1, 4).index_select(0, idx)          # the minibatch's observations: _minibatch has them for its re-solve

        def f():
            p._value_step(idx, obs, 1)
        return f
    small = {flag: learner(256, flag) for flag in (False, True)}
    for flag, p in small.items():                     # the same roll-out: copy the tables the value step reads
        p.OBS.copy_(big[flag].OBS), p.RET.copy_(big[flag].RET)
    torch.cuda.synchronize()
    row("(b) value step (gradient -> Adam), B = 256", ab({k: vstep(p) for k, p in small.items()}, args.repeats, args.inner))
    row("(b) value step (gradient -> Adam), B = 4096", ab({k: vstep(p) for k, p in big.items()}, args.repeats, args.inner))
    del small

    # (c)
    r = ab({k: (lambda p=p: p.learn(1)) for k, p in big.items()}, args.repeats, 1, warmup=2)
    row("(c) learn(1), E 4096, T 8, B 4096, 1 epoch", r)
    for flag, p in big.items():
        st = p.last_stats()
        say(f"#   value_kernels={flag}: after {p.iterations} iterations value_loss {st['value_loss']:.4g}, valid_fraction {st['valid_fraction']:.4f}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
