"""Batched cartpole Q-learning (mpc4rl_amd.CartpoleQLearning): ms per roll-out step, ms per learning sweep and episodes/s, eager launches
against replayed HIP graphs.
    python profiles/microbench/qlearning_cartpole.py [--envs 4096] [--T 100] [--episodes 3]
An episode = the start (environment reset, noise draw), T roll-out steps (solve + collect), the learning sweep (Q solve, V solve over the
E (T - 1) samples, TD kernel), the apply; the phases are timed with events on the stream, the episode by the wall clock (statistics read
back included).  One untimed episode first (launch-shape probes of the solver handles)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mpc4rl_amd import BatchedCartPoleSwingUpEnv, CartpoleQLearning, cartpole_ocp  # noqa: E402


def timed_episode(ql):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ql._start_episode()
    ev[0].record()
    if ql._graphs is not None:
        for _ in range(ql.T):
            ql._graphs["rollout"].replay()
        ev[1].record()
        ql._graphs["sweep"].replay()
        ql.last_sweep = ql._graphs["sweep_out"]
    else:
        for _ in range(ql.T):
            ql._rollout_step()
        ev[1].record()
        ql.last_sweep = ql._sweep()
    ev[2].record()
    ql._allreduce()
    ql._apply()
    ev[3].record()
    st = ql._stats()
    wall = time.perf_counter() - t0
    return st, wall, ev[0].elapsed_time(ev[1]) / ql.T, ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--episodes", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"CartpoleQLearning E = {args.envs}, T = {args.T}: sweep batch {args.envs * (args.T - 1)} samples; {args.episodes} timed episodes "
          f"after one untimed", flush=True)
    for graphs in (False, True):
        env = BatchedCartPoleSwingUpEnv(args.envs, device=dev, seed=0)
        ql = CartpoleQLearning(cartpole_ocp(), env, args.T, seed=0)
        if graphs:
            ql.enable_graphs()
        timed_episode(ql)
        rows = [timed_episode(ql) for _ in range(args.episodes)]
        mode = "graphs" if graphs else "eager "
        for k, (st, wall, ms_step, ms_sweep, ms_apply) in enumerate(rows):
            L = st.episode_lengths.double()
            print(f"{mode} episode {k}: roll-out {ms_step:.3f} ms/step, sweep {ms_sweep:.2f} ms, apply {ms_apply:.3f} ms, episode {wall * 1e3:.1f} ms "
                  f"({1.0 / wall:.2f} episodes/s); mean length {float(L.mean()):.1f}, valid terms {st.converged_fraction:.4f}", flush=True)
        wall = sum(r[1] for r in rows) / len(rows)
        print(f"{mode} mean: roll-out {sum(r[2] for r in rows) / len(rows):.3f} ms/step, sweep {sum(r[3] for r in rows) / len(rows):.2f} ms, "
              f"{1.0 / wall:.2f} episodes/s", flush=True)


if __name__ == "__main__":
    main()
