"""What tests/test_td3_replay_cpu.py, tests/test_gpu_td3_replay_edges.py and tests/test_gpu_next_rows.py share (no test of its own): a
scripted episode log as the reference for the warm starts of the TD3 replay solves (mpcrl_replay_sample, csrc/replay_kernel.hpp, and
DeviceReplayBuffer.iterates_of_last_sample, mpc4rl_amd/td3.py).  Numpy only.

The property under test: the target actor's solve at a sampled transition's next_obs starts from the roll-out solution stored with the
NEXT step of the same environment (row_n) only where that row's obs IS this row's next_obs — the episode did not end at this step, for
either reason, and the next step is in the table and may be read; everywhere else from the solution at obs (row_n = row_s).  The table's
done column holds `terminated` alone (what the TD target needs), so an episode cut off at the time limit cannot be told from the column:
the log keeps `terminated` and `truncated` of every row on its own, and the reference below never looks at the column.

The log takes no physics from anywhere.  The observation of step k of episode ep of environment e is the vector
    obs[j] = (-1)^j (id (nx + 1) + j + 1),   id = (e (S + 1) + ep) (S + 2) + k
small integers, exact in float32, distinct over all (e, ep, k) in every entry: inside an episode next_obs of step t is bit-equal to obs
of step t + 1; after an episode's end obs of step t + 1 is step 0 of a fresh episode and differs from next_obs of step t in EVERY entry."""
import dataclasses

import numpy as np


@dataclasses.dataclass
class Log:
    E: int
    S: int
    nx: int
    nu: int
    cap: int
    table: np.ndarray          # [cap, E, 2 nx + nu + 2] float32 after S writes (slot = t % cap): obs | next obs | action | reward | terminated
    steps: int                 # slots written: min(S, cap)
    pos: int                   # the slot written next: S % cap
    iter_ok: np.ndarray        # [cap, E] uint8, seeded
    t: np.ndarray              # [cap, E] the global step a table row holds (-1: never written)
    terminated: np.ndarray     # [cap, E] bool
    truncated: np.ndarray      # [cap, E] bool (never together with terminated)


def _obs(e, ep, k, S, nx):
    ident = (e * (S + 1) + ep) * (S + 2) + k
    j = np.arange(nx)
    return np.where(j % 2 == 0, 1.0, -1.0) * (ident * (nx + 1) + j + 1)


def make_log(E, S, nx, nu, cap, seed, p_term=0.15, p_trunc=0.15, p_cold=0.25):
    """S global steps of E environments from a script: every environment draws per step whether the episode terminates (p_term), is
    truncated (p_trunc) or goes on."""
    assert E >= 1 and S >= 1 and cap >= 1
    assert (E * (S + 1) * (S + 2) + 1) * (nx + 1) < 2 ** 24, "the observations would not be exact in float32"
    rng = np.random.default_rng(seed)
    L = 2 * nx + nu + 2
    table = np.zeros((cap, E, L), dtype=np.float32)
    t_of = np.full((cap, E), -1, dtype=np.int64)
    term, trunc = np.zeros((cap, E), dtype=bool), np.zeros((cap, E), dtype=bool)
    ep, k = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    for t in range(S):
        slot = t % cap
        u = rng.random(E)
        te, tr = u < p_term, (u >= p_term) & (u < p_term + p_trunc)
        for e in range(E):
            table[slot, e, :nx] = _obs(e, ep[e], k[e], S, nx)
            table[slot, e, nx: 2 * nx] = _obs(e, ep[e], k[e] + 1, S, nx)
        table[slot, :, 2 * nx: 2 * nx + nu] = rng.integers(-8, 9, (E, nu)) / 8.0
        table[slot, :, -2] = rng.integers(-100, 101, E) / 4.0
        table[slot, :, -1] = te                      # the done column: terminated ONLY
        t_of[slot], term[slot], trunc[slot] = t, te, tr
        ended = te | tr
        ep, k = ep + ended, np.where(ended, 0, k + 1)
    iter_ok = (rng.random((cap, E)) >= p_cold).astype(np.uint8)
    return Log(E, S, nx, nu, cap, table, min(S, cap), S % cap, iter_ok, t_of, term, trunc)


def sampled_slots(log, idx, exclude_pos=None):
    """(slot, env) of the sampled rows.  Without exclude_pos idx = slot * E + env.  With it, idx counts the rows of the other cap - 1
    slots in the order after that slot (include/mpcrl.h): slot = (exclude_pos + 1 + idx / E) % cap."""
    idx = np.asarray(idx, dtype=np.int64)
    if exclude_pos is None:
        assert idx.min() >= 0 and idx.max() < log.steps * log.E
        return idx // log.E, idx % log.E
    assert log.steps == log.cap and log.cap >= 2 and idx.min() >= 0 and idx.max() < (log.cap - 1) * log.E
    slot = (exclude_pos + 1 + idx // log.E) % log.cap
    assert not (slot == exclude_pos).any()
    return slot, idx % log.E


def expected_starts(log, idx, exclude_pos=None):
    """The reference for mpcrl_replay_sample's outputs on the rows ``idx``, from the log (never from the done column, never from the
    excluded slot): rows, obs64, nxt64, row_s, row_n, cold_s, cold_n, and the masks the class counts are made of."""
    slot, env = sampled_slots(log, idx, exclude_pos)
    E, cap, nx = log.E, log.cap, log.nx
    t = log.t[slot, env]
    assert (t >= 0).all()
    rows = log.table[slot, env]
    ended = log.terminated[slot, env] | log.truncated[slot, env]
    nslot = (t + 1) % cap
    written = t + 1 <= log.S - 1                       # step t + 1 has been played (and, t being in the table, is still in it)
    allowed = np.ones_like(written) if exclude_pos is None else nslot != exclude_pos
    cont = ~ended & written & allowed
    row_s = slot * E + env
    row_n = np.where(cont, nslot * E + env, row_s)
    ok = log.iter_ok.reshape(-1)
    return {
        "rows": rows, "obs64": rows[:, :nx].astype(np.float64), "nxt64": rows[:, nx: 2 * nx].astype(np.float64),
        "row_s": row_s, "row_n": row_n, "cold_s": (1 - ok[row_s]).astype(np.int32), "cold_n": (1 - ok[row_n]).astype(np.int32),
        "cont": cont, "terminated": log.terminated[slot, env], "truncated": log.truncated[slot, env],
        "next_barred": ~ended & (~written | ~allowed), "next_unwritten": ~written & (log.steps < cap),
    }


CLASSES = ("continued", "terminated", "truncated", "next_barred", "next_unwritten", "cold_s", "cold_n")


def class_counts(log, ref, exclude_pos=None):
    """How many rows of a sample fall into each class a case has to contain (CLASSES); None for a class the case cannot produce: a
    table of one slot (or of two with one excluded) has no next row, a full table no unwritten slot.  cold_n counts the rows whose
    NEXT row's flag decides (row_n != row_s) wherever there can be such rows."""
    can_continue = log.cap - (exclude_pos is not None) >= 2 and log.S >= 2
    return {
        "continued": int(ref["cont"].sum()) if can_continue else None,
        "terminated": int(ref["terminated"].sum()),
        "truncated": int(ref["truncated"].sum()),
        "next_barred": int(ref["next_barred"].sum()),      # the episode went on, but the next slot is the write position / the excluded slot
        "next_unwritten": int(ref["next_unwritten"].sum()) if log.steps < log.cap else None,
        "cold_s": int(ref["cold_s"].sum()),
        "cold_n": int((ref["cold_n"] * (ref["cont"] if can_continue else 1)).sum()),
    }


def add_counts(total, counts):
    for name, c in counts.items():
        total[name] = c if total.get(name) is None else total[name] + (c or 0)
    return total


def assert_every_class(total, what):
    empty = [name for name in CLASSES if total[name] is not None and total[name] == 0]
    assert not empty, f"{what}: no row of class {empty} in the sample ({total})"


# (E, cap, S) -> the seeds of the logs a case is run on.  A table of a handful of rows cannot hold every class at once (one environment
# and two slots: two rows), so such a case runs on several logs and the classes are counted over all of them.
NX_CPU, NU_CPU, N_CPU = 4, 1, 200        # the CPU cases' row shape and sample size
CPU_CASES = {
    (5, 4, 3): (0, 1),          # partially filled table
    (5, 4, 4): (0,),           # exactly full, pos = 0
    (7, 4, 11): (0,),          # wrapped table
    (3, 1, 5): (0, 5, 6),         # one slot, never a next row
    (1, 2, 9): (0, 1, 3),         # one environment, two slots
}

# mpcrl_replay_sample on the device: (nx, nu, E, cap, S, batch sizes, seeds, every slot as the excluded one too)
GPU_CASES = [
    (4, 1, 37, 5, 12, (1, 255, 256, 257, 1000), (0,), True),      # one lane, ragged and full workgroups, a second workgroup of one lane
    (2, 1, 1, 2, 9, (300,), (32, 33, 35, 36), True),             # one environment (with exclusion: one slot left)
    (9, 3, 3, 3, 7, (300,), (1,), False),                          # row_len 7 and 23: the linear system's and the chain's shapes
    (4, 1, 256, 4, 3, (500,), (0,), False),                        # steps < cap: nstep < steps decides
    (4, 1, 256, 4, 4, (500,), (0,), True),                         # exactly full, pos = 0
    (4, 1, 5, 1, 3, (64,), (3,), False),                           # cap = 1: no next row ever
]


def whole_table(log, exclude_pos=None):
    """idx of every row a sample can draw"""
    return np.arange((log.steps - (exclude_pos is not None)) * log.E, dtype=np.int64)
