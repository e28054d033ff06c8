"""CPU tests of the TD3 replay buffer's warm starts (DeviceReplayBuffer.iterates_of_last_sample, mpc4rl_amd/td3.py — the expressions
mpcrl_replay_sample repeats on the device) against a scripted episode log (tests/replay_cases.py): the iterate for next_obs is the
NEXT step's only where that step's obs is this row's next_obs — not after an episode that terminated, not after one cut off at the time
limit (whose done flag is 0), not across the write position, not into a slot never written.  First the generator itself."""
import numpy as np
import pytest
import torch

import replay_cases as R


def _all_cases():
    for (E, cap, S), seeds in R.CPU_CASES.items():
        yield (R.NX_CPU, R.NU_CPU, E, cap, S, seeds, False)
    for nx, nu, E, cap, S, _, seeds, excl in R.GPU_CASES:
        yield (nx, nu, E, cap, S, seeds, excl)


@pytest.mark.parametrize("nx,nu,E,cap,S,seeds,excl", list(_all_cases()))
def test_log_generator(nx, nu, E, cap, S, seeds, excl):
    """The scripted log keeps what it promises, for every case of the CPU and the GPU tests: exact small integers, every observation
    distinct, next_obs == the next step's obs exactly inside an episode and different in every entry after its end, the done column =
    terminated, the ring layout — and the table of every case holds every class of row the case can produce, so that a sample can."""
    total, total_x = {}, {}
    for seed in seeds:
        log = R.make_log(E, S, nx, nu, cap, seed)
        L = 2 * nx + nu + 2
        assert log.table.shape == (cap, E, L) and log.table.dtype == np.float32
        assert log.steps == min(S, cap) and log.pos == S % cap and log.iter_ok.shape == (cap, E) and log.iter_ok.dtype == np.uint8
        again = R.make_log(E, S, nx, nu, cap, seed)
        assert np.array_equal(again.table, log.table) and np.array_equal(again.iter_ok, log.iter_ok)
        t64 = log.table.astype(np.float64)
        written = log.t >= 0
        assert np.array_equal(t64[..., : 2 * nx], np.round(t64[..., : 2 * nx])) and float(np.abs(t64).max()) < 2 ** 24
        for slot in range(cap):      # the ring: slot t % cap holds the last step written there
            newest = [t for t in range(S) if t % cap == slot][-1:] or [-1]
            assert (log.t[slot] == newest[0]).all()
        assert int(written.sum()) == log.steps * E
        assert not (log.terminated & log.truncated).any() and not (~written & (log.terminated | log.truncated)).any()
        assert np.array_equal(log.table[..., -1] != 0, log.terminated)          # terminated ONLY
        assert not np.any(log.table[~written])
        obs, nxt = log.table[..., :nx][written], log.table[..., nx: 2 * nx][written]
        for j in range(nx):      # every stored observation differs from every other one in every entry
            assert len(np.unique(obs[:, j])) == len(obs)
        for slot in range(log.steps):
            for e in range(E):
                t = log.t[slot, e]
                if t + 1 > S - 1:
                    continue
                o_next = log.table[(t + 1) % cap, e, :nx]
                assert log.t[(t + 1) % cap, e] == t + 1
                if log.terminated[slot, e] or log.truncated[slot, e]:
                    assert (o_next != log.table[slot, e, nx: 2 * nx]).all()
                else:
                    assert o_next.tobytes() == log.table[slot, e, nx: 2 * nx].tobytes()
        R.add_counts(total, R.class_counts(log, R.expected_starts(log, R.whole_table(log))))
        if excl:
            for x in range(cap):
                ref = R.expected_starts(log, R.whole_table(log, x), x)
                assert not (ref["row_s"] // E == x).any() and not (ref["row_n"] // E == x).any()
                R.add_counts(total_x.setdefault(x, {}), R.class_counts(log, ref, x))
    R.assert_every_class(total, f"table {(nx, nu, E, cap, S)}")
    for x, tot in total_x.items():
        R.assert_every_class(tot, f"table {(nx, nu, E, cap, S)} without slot {x}")
    if cap == 1:
        assert total["continued"] is None and total["next_barred"] > 0


@pytest.mark.parametrize("E,cap,S", list(R.CPU_CASES))
def test_iterates_of_last_sample_against_the_log(E, cap, S):
    """DeviceReplayBuffer on the CPU, its table, flags and write position set from a log: sample() + iterates_of_last_sample() equal
    the log's answer exactly on the rows that were drawn, and the draw holds every class of row the case can produce."""
    from mpc4rl_amd.td3 import DeviceReplayBuffer
    nx, nu, n = R.NX_CPU, R.NU_CPU, R.N_CPU
    total = {}
    for seed in R.CPU_CASES[(E, cap, S)]:
        log = R.make_log(E, S, nx, nu, cap, seed)
        buf = DeviceReplayBuffer(cap, E, nx, nu, "cpu", iterate_dims=(3, 2, 2, 4))
        buf.data.copy_(torch.from_numpy(log.table))
        buf.iter_ok.copy_(torch.from_numpy(log.iter_ok).bool())
        buf.pos, buf.full = log.pos, S >= cap
        buf.pos_t.fill_(log.pos)
        gen = torch.Generator().manual_seed(100 + seed)
        obs, nxt, act, rew, done = buf.sample(n, gen)
        row_s, ok_s, row_n, ok_n = buf.iterates_of_last_sample()
        idx = buf.last_idx.numpy()
        ref = R.expected_starts(log, idx)
        counts = R.class_counts(log, ref)
        print(f"(E, cap, S) = {(E, cap, S)}, seed {seed}: {counts}")
        assert np.array_equal(buf.last_rows.numpy(), ref["rows"]) and np.array_equal(obs.numpy(), ref["rows"][:, :nx])
        assert np.array_equal(nxt.numpy(), ref["rows"][:, nx: 2 * nx]) and np.array_equal(done.numpy() != 0, ref["terminated"])
        assert np.array_equal(row_s.numpy(), ref["row_s"])
        wrong = row_n.numpy() != ref["row_n"]
        assert not wrong.any(), (f"{int(wrong.sum())} of {n} rows start the solve at next_obs from another row than the log's: "
                                 f"{int((wrong & ref['truncated']).sum())} truncated, {int((wrong & ref['terminated']).sum())} terminated, "
                                 f"{int((wrong & ref['cont']).sum())} continued, {int((wrong & ref['next_barred']).sum())} with the next slot barred")
        assert np.array_equal(~ok_s.numpy(), ref["cold_s"] != 0) and np.array_equal(~ok_n.numpy(), ref["cold_n"] != 0)
        R.add_counts(total, counts)
    R.assert_every_class(total, f"sample of {(E, cap, S)}")
