"""GPU tests of the replay side of the TD3 loop at the shapes and edges its loop tests do not reach.

mpcrl_replay_sample (csrc/replay_kernel.hpp) against a scripted episode log (tests/replay_cases.py), through the C ABI: the rows from
which the two replay solves of an update start.  The log knows which episodes terminated and which were cut off at the time limit; the
table's done column holds `terminated` alone, so the reference never reads it.  The property: wherever row_n != row_s, the transition
stored at row_n was observed at this row's next_obs.  Every output is a copy, a widening or an integer: compared with torch.equal, over
sentinel-filled buffers with sentinel tails.  Then the same property in the closed loop (BatchedTD3 on the cartpole, episodes of four
steps), on both sampling and both collect paths, and mpcrl_policy_action beyond one control, bit for bit against the torch expressions
it replaces."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_cases as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)
E_ARG = -1          # MPCRL_E_ARG, include/mpcrl.h
TAIL = 5
S_F, S_I = -7777.0, -77      # sentinels: floating-point outputs, integer outputs


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


@pytest.fixture(scope="module")
def lib():
    from mpc4rl_amd import _lib
    return _lib.load()


# -------------------------------------------------------------------------------------------------------------------- mpcrl_replay_sample

class _Out:
    """every output of one call: sentinel-filled, with a sentinel tail"""

    def __init__(self, B, L, nx):
        self.B, self.L, self.nx = B, L, nx
        self.rows = torch.full((B * L + TAIL,), S_F, dtype=torch.float32, device=DEV)
        self.obs64, self.nxt64 = torch.full((B * nx + TAIL,), S_F, **F64), torch.full((B * nx + TAIL,), S_F, **F64)
        self.row_s, self.row_n = (torch.full((B + TAIL,), S_I, dtype=torch.int64, device=DEV) for _ in range(2))
        self.cold_s, self.cold_n = (torch.full((B + TAIL,), S_I, dtype=torch.int32, device=DEV) for _ in range(2))

    def all(self):
        return (self.rows, self.obs64, self.nxt64, self.row_s, self.row_n, self.cold_s, self.cold_n)

    def starts(self):
        return (self.row_s, self.row_n, self.cold_s, self.cold_n)

    def untouched(self, tensors):
        return all(bool((t == (S_F if t.is_floating_point() else S_I)).all()) for t in tensors)

    def tails_untouched(self):
        B, L, nx = self.B, self.L, self.nx
        return self.untouched([self.rows[B * L:], self.obs64[B * nx:], self.nxt64[B * nx:]] + [t[B:] for t in self.starts()])


def _call(lib, out, table, L, nx, E, cap, steps, idx, B, pos_t, exclude, iter_ok, starts=True):
    s = [_p(t) for t in (out.row_s, out.cold_s, out.row_n, out.cold_n)] if starts else [None] * 4
    rc = lib.mpcrl_replay_sample(_p(table), L, nx, E, cap, steps, _p(idx), B, _p(pos_t), int(exclude), _p(iter_ok), _p(out.rows), _p(out.obs64),
                                 _p(out.nxt64), *s, _stream())
    torch.cuda.synchronize()
    return rc


def _padded(rows, nx, nu, pad):
    """obs | next obs | action | pad entries | reward | done: the reward and done columns stay the last two (include/mpcrl.h)"""
    if not pad:
        return rows
    filler = np.full(rows.shape[:-1] + (pad,), 555.0, dtype=np.float32)
    return np.concatenate([rows[..., : 2 * nx + nu], filler, rows[..., 2 * nx + nu:]], axis=-1)


def _device_tables(log, exclude_pos, pad):
    """The table and flags on the device.  With an excluded slot: that slot of the table is NaN and its flags are the opposite of the
    log's — the reference reads neither, so any use of them shows."""
    table, ok = _padded(log.table, log.nx, log.nu, pad).copy(), log.iter_ok.copy()
    if exclude_pos is not None:
        table[exclude_pos], ok[exclude_pos] = np.nan, 1 - ok[exclude_pos]
    return torch.from_numpy(table).to(DEV), torch.from_numpy(ok).to(DEV)


def _check(lib, log, idx, exclude_pos=None, pad=0):
    """one launch on the rows idx (a device tensor) against the log; returns the class counts of the sample"""
    nx, E, cap = log.nx, log.E, log.cap
    L, B = 2 * nx + log.nu + 2 + pad, idx.numel()
    table, ok = _device_tables(log, exclude_pos, pad)
    pos_t = torch.tensor([log.pos if exclude_pos is None else exclude_pos], dtype=torch.int64, device=DEV)
    out = _Out(B, L, nx)
    assert _call(lib, out, table, L, nx, E, cap, log.steps, idx, B, pos_t, exclude_pos is not None, ok) == 0
    ref = R.expected_starts(log, idx.cpu().numpy(), exclude_pos)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert not any(bool(torch.isnan(t).any()) for t in (out.rows, out.obs64, out.nxt64))
    assert torch.equal(out.rows[: B * L].view(B, L), dev(_padded(ref["rows"], nx, log.nu, pad)))
    assert torch.equal(out.obs64[: B * nx].view(B, nx), dev(ref["obs64"])) and torch.equal(out.nxt64[: B * nx].view(B, nx), dev(ref["nxt64"]))
    assert torch.equal(out.row_s[:B], dev(ref["row_s"]))
    wrong = (out.row_n[:B] != dev(ref["row_n"])).cpu().numpy()
    assert not wrong.any(), (f"{int(wrong.sum())} of {B} rows start the solve at next_obs from another row than the log's: "
                             f"{int((wrong & ref['truncated']).sum())} truncated, {int((wrong & ref['terminated']).sum())} terminated, "
                             f"{int((wrong & ref['cont']).sum())} continued, {int((wrong & ref['next_barred']).sum())} with the next slot barred")
    assert torch.equal(out.cold_s[:B], dev(ref["cold_s"])) and torch.equal(out.cold_n[:B], dev(ref["cold_n"]))
    assert out.tails_untouched()
    # the property itself, on what the kernel wrote: the row it moved to holds this row's next obs as its obs
    moved = out.row_n[:B] != out.row_s[:B]
    flat = torch.from_numpy(log.table).to(DEV).reshape(cap * E, -1)
    assert torch.equal(flat[out.row_n[:B][moved], :nx], out.rows[: B * L].view(B, L)[moved, nx: 2 * nx])
    return R.class_counts(log, ref, exclude_pos)


def _draw(log, B, gen, exclude_pos=None):
    """B > 1: torch.randint over the rows the sample may draw.  B = 1 (one lane): one launch per class of row the table holds, the row
    drawn with torch.randint among that class's rows."""
    n_rows = (log.steps - (exclude_pos is not None)) * log.E
    if B > 1:
        return [torch.randint(0, n_rows, (B,), device=DEV, generator=gen)]
    ref = R.expected_starts(log, R.whole_table(log, exclude_pos), exclude_pos)
    masks = [ref["cont"], ref["terminated"], ref["truncated"], ref["next_barred"], ref["next_unwritten"], ref["cold_s"] != 0,
             (ref["cold_n"] != 0) & ref["cont"]]
    draws = []
    for m in masks:
        cand = torch.from_numpy(np.nonzero(m)[0]).to(DEV)
        if cand.numel():
            draws.append(cand[torch.randint(0, cand.numel(), (1,), device=DEV, generator=gen)])
    return draws


def _case_id(c):
    return "nx%d-nu%d-E%d-cap%d-S%d" % c[:5]


@pytest.mark.parametrize("case", R.GPU_CASES, ids=_case_id)
def test_replay_sample_against_the_log(lib, case):
    """Every listed table at every listed batch size — one lane, ragged and full workgroups, a second workgroup of one lane; one
    environment; rows of 7 and 23 floats; a partially filled and an exactly full table; one slot — with every class of row (continued,
    terminated, truncated, next slot barred or unwritten, cold flags at either row) in every sample."""
    nx, nu, E, cap, S, Bs, seeds, _ = case
    gen = torch.Generator(device=DEV).manual_seed(1000 * E + 10 * cap + S)
    for B in Bs:
        total = {}
        for seed in seeds:
            log = R.make_log(E, S, nx, nu, cap, seed)
            for idx in _draw(log, B, gen):
                R.add_counts(total, _check(lib, log, idx))
        print(f"{_case_id(case)} B {B}: {total}")
        R.assert_every_class(total, f"{_case_id(case)}, B = {B}")


@pytest.mark.parametrize("case", [c for c in R.GPU_CASES if c[7]], ids=_case_id)
def test_replay_sample_with_every_slot_excluded(lib, case):
    """exclude_pos on the wrapped and the exactly full tables, every slot of the table as the excluded one (the pipelined loop only ever
    excludes the write position; the kernel is told a slot).  The excluded slot is NaN on the device and its iter_ok flags are inverted:
    no output holds a NaN and no cold flag follows the inverted ones, so the slot is never read — not by the gather, not by the
    comparison of the next row's obs.  Two slots with one excluded leave one: no next row."""
    nx, nu, E, cap, S, Bs, seeds, _ = case
    assert S >= cap >= 2
    gen = torch.Generator(device=DEV).manual_seed(2000 * E + 10 * cap + S)
    for x in range(cap):
        for B in Bs:
            total = {}
            for seed in seeds:
                log = R.make_log(E, S, nx, nu, cap, seed)
                for idx in _draw(log, B, gen, x):
                    R.add_counts(total, _check(lib, log, idx, exclude_pos=x))
            R.assert_every_class(total, f"{_case_id(case)} without slot {x}, B = {B}")
            assert (total["continued"] is None) == (cap == 2)


def test_replay_sample_padded_row(lib):
    """row_len = 2 nx + nu + 2 + 3: three entries between the action and the reward; done is the LAST entry of the row, whatever its
    length (include/mpcrl.h) — with and without an excluded slot."""
    nx, nu, E, cap, S, _, seeds, _ = R.GPU_CASES[0]
    log = R.make_log(E, S, nx, nu, cap, seeds[0])
    gen = torch.Generator(device=DEV).manual_seed(5)
    for x in (None, log.pos, (log.pos + 2) % cap):
        idx = torch.randint(0, (cap - (x is not None)) * E, (257,), device=DEV, generator=gen)
        R.assert_every_class(_check(lib, log, idx, exclude_pos=x, pad=3), "padded row")


def test_replay_sample_without_iterate_tables(lib):
    """iter_ok = NULL: rows, obs64 and nxt64 are written, the four start arrays keep their sentinels — and may be NULL, with pos_t."""
    nx, nu, E, cap, S, _, seeds, _ = R.GPU_CASES[0]
    log = R.make_log(E, S, nx, nu, cap, seeds[0])
    table, L, B = torch.from_numpy(log.table).to(DEV), 2 * nx + nu + 2, 300
    idx = torch.randint(0, cap * E, (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    pos_t = torch.tensor([log.pos], dtype=torch.int64, device=DEV)
    rows = table.reshape(cap * E, L)[idx]
    for starts in (True, False):
        out = _Out(B, L, nx)
        assert _call(lib, out, table, L, nx, E, cap, log.steps, idx, B, pos_t if starts else None, 0, None, starts=starts) == 0
        assert torch.equal(out.rows[: B * L].view(B, L), rows) and torch.equal(out.obs64[: B * nx].view(B, nx), rows[:, :nx].double())
        assert torch.equal(out.nxt64[: B * nx].view(B, nx), rows[:, nx: 2 * nx].double())
        assert out.untouched(out.starts()) and out.tails_untouched()


def test_replay_sample_refusals(lib):
    """The argument check of mpcrl_replay_sample: MPCRL_E_ARG and nothing written."""
    nx, nu, E, cap, S, _, seeds, _ = R.GPU_CASES[0]
    log = R.make_log(E, S, nx, nu, cap, seeds[0])
    table, ok = _device_tables(log, None, 0)
    L, B = 2 * nx + nu + 2, 64
    idx = torch.randint(0, E, (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))      # rows of slot 0: valid for every call below
    pos_t = torch.tensor([log.pos], dtype=torch.int64, device=DEV)
    out = _Out(B, L, nx)
    good = dict(table=table, L=L, nx=nx, E=E, cap=cap, steps=cap, idx=idx, B=B, pos_t=pos_t, exclude=0, iter_ok=ok)
    refused = [dict(steps=cap + 1), dict(steps=0), dict(B=0), dict(L=2 * nx + 1),
               dict(exclude=1, steps=cap - 1), dict(exclude=1, cap=1, steps=1)]
    for change in refused:
        assert _call(lib, out, **{**good, **change}) == E_ARG, change
        assert out.untouched(out.all()), change
    for missing in range(4):      # iter_ok given, one of the start arrays NULL
        s = [_p(t) for t in (out.row_s, out.cold_s, out.row_n, out.cold_n)]
        s[missing] = None
        rc = lib.mpcrl_replay_sample(_p(table), L, nx, E, cap, cap, _p(idx), B, _p(pos_t), 0, _p(ok), _p(out.rows), _p(out.obs64), _p(out.nxt64), *s, _stream())
        torch.cuda.synchronize()
        assert rc == E_ARG and out.untouched(out.all()), missing
    assert _call(lib, out, **good) == 0 and not out.untouched([out.rows[: B * L]])      # (the unchanged call is accepted)


# ------------------------------------------------------------------------------------------------------------- the property in the loop

NEAR_ORIGIN = 0.01      # the factor on the state of the environments that are to terminate (test_td3_cartpole_collect_wrap_and_stats)


def _loop_run(fused_collect):
    """BatchedTD3 on 64 cartpoles with episodes of four steps, eleven steps into a table of eight slots; the truncations are spread
    over the slots, and every fifth environment is put next to the upright origin before the first of the eight steps the table keeps,
    so that episodes terminate there.  Returns what the assertions need."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedTD3, cartpole_ocp
    E, cap, T, n = 64, 8, 11, 1024
    env = BatchedCartPoleSwingUpEnv(E, device="cuda", seed=0, max_episode_steps=4)
    ag = BatchedTD3(cartpole_ocp(), env, batch_size=64, buffer_steps=cap, seed=0, replay_iterates=True, action_noise=0.0)
    assert ag._fused_collect and ag._fused_sample
    ag._fused_collect = fused_collect
    env.steps.copy_(torch.arange(E, device=DEV) % 4)
    buf = ag.buffer
    trunc, term = (torch.zeros(cap, E, dtype=torch.bool, device=DEV) for _ in range(2))
    for t in range(T):
        if t == T - cap:      # (set from outside before the oldest step the table will keep: the rows that do not lead here are overwritten)
            env.state[::5] *= NEAR_ORIGIN
            ag.obs.copy_(env.state)
        before = env.steps.clone()
        ag.collect(1)
        slot = t % cap
        term[slot] = buf.done[slot] != 0
        trunc[slot] = (before + 1 >= 4) & ~term[slot]           # cut off at the time limit: the environment is reset, the flag stays 0
        assert torch.equal(env.steps == 0, term[slot] | (before + 1 >= 4))      # (the bookkeeping agrees with the resets that happened)
    assert buf.full and buf.pos == T % cap and int(buf.pos_t) == buf.pos
    gen = torch.Generator(device=DEV).manual_seed(7)
    state = gen.get_state()
    buf.sample_fused(n, gen)
    fused = (buf.last_idx.clone(), buf.last_rows.clone()) + tuple(t.clone() for t in buf.last_starts)
    gen.set_state(state)
    buf.sample(n, gen)
    i_s, ok_s, i_n, ok_n = buf.iterates_of_last_sample()
    unfused = (buf.last_idx.clone(), buf.last_rows.clone(), i_s, (~ok_s).to(torch.int32), i_n, (~ok_n).to(torch.int32))
    return dict(buf=buf, E=E, cap=cap, T=T, trunc=trunc, term=term, fused=fused, unfused=unfused,
                tables=[buf.data.clone(), buf.iter_ok.clone()] + [t.clone() for t in buf.iters])


def test_td3_loop_next_state_starts_across_episode_ends():
    """The property in the closed loop.  Wherever a sampled row's row_n != row_s, the obs stored at row_n is bit-equal to the row's
    next_obs; an episode cut off at the time limit (done flag 0, environment reset) never moves to the next row although that row is
    written; every row whose episode went on and whose next step is in the table does move.  The stored iterate's stage-0 state IS the
    state it was solved for: small_kernel.hpp pins stage 0 (the QP step of stage 0 is x0 - x, full steps: x + (x0 - x), one rounding
    of a double away from x0 at the most, and x0 itself from a cold start), so after the cast to float32 it equals next_obs at row_n
    wherever that solve converged (and obs at row_s).  Both sampling paths (sample_fused; sample + iterates_of_last_sample) and both
    collect paths (mpcrl_td3_cartpole_collect; the framework's launches) give identical tables, starts and masks."""
    runs = {fc: _loop_run(fc) for fc in (True, False)}
    a, b = runs[True], runs[False]
    assert all(torch.equal(x, y) for x, y in zip(a["tables"], b["tables"]))
    assert all(torch.equal(x, y) for x, y in zip(a["fused"], b["fused"])) and torch.equal(a["trunc"], b["trunc"])
    for run in (a, b):
        buf, E, cap, nx = run["buf"], run["E"], run["cap"], 4
        idx, rows, row_s, cold_s, row_n, cold_n = run["fused"]
        assert torch.equal(row_s, idx)
        obs_flat = buf.data.reshape(cap * E, -1)[:, :nx]
        nxt = rows[:, nx: 2 * nx]
        bits = lambda t: t.contiguous().view(torch.int32)
        moved = row_n != row_s
        slot, e = idx // E, idx % E
        next_written = (slot + 1) % cap != buf.pos                     # a full table: step t + 1 is there unless t is the newest step
        trunc, term = run["trunc"][slot, e], run["term"][slot, e]
        cut = trunc & next_written
        astray = moved & ~(bits(obs_flat[row_n]) == bits(nxt)).all(dim=1)      # moved to a row that was NOT observed at next_obs
        n_cut, n_wrong = int(cut.sum()), int((cut & moved).sum())
        print(f"fused collect {run is a}: of {idx.numel()} sampled rows {int(moved.sum())} moved to the next step's row, {int(astray.sum())} of them to a row "
              f"whose obs is not their next_obs ({int((astray & trunc).sum())} cut off at the time limit); {n_cut} cut off with the next slot written, "
              f"{n_wrong} of them moved; {int(term.sum())} terminated ({int(run['term'].sum())} terminated rows in the table)")
        assert not bool(astray.any())
        x_n, x_s = buf.iters[0][row_n, :nx].to(torch.float32), buf.iters[0][row_s, :nx].to(torch.float32)
        warm_n, warm_s = moved & (cold_n == 0), cold_s == 0
        assert int(warm_n.sum()) > 0 and torch.equal(x_n[warm_n], nxt[warm_n]) and torch.equal(x_s[warm_s], rows[:, :nx][warm_s])
        assert n_cut > 0 and n_wrong == 0
        assert int(term.sum()) > 0 and not bool((term & moved).any())
        assert torch.equal(moved, ~trunc & ~term & next_written)
        assert int(moved.sum()) > 0 and int((~moved).sum()) > 0
        assert all(torch.equal(x, y) for x, y in zip(run["fused"], run["unfused"]))


# ------------------------------------------------------------------------------------------------------------------- mpcrl_policy_action

def _policy_reference(u0, status, eps, lo, hi, scale, sigma, clip, acc2):
    """the torch expressions of test_policy_action_kernel_and_fused_td3_glue (a), per control with vector lo and hi"""
    ok = torch.isfinite(u0).all(dim=1) & ((status == 0) | (status == 2) if acc2 else (status == 0))
    u = torch.nan_to_num(u0)
    a = torch.where(ok[:, None], 2.0 * ((u - lo) / (hi - lo)) - 1.0 if scale else u, torch.zeros_like(u)).to(torch.float32)
    if eps is not None:
        n = sigma * eps
        if clip > 0:
            n = n.clamp(-clip, clip)
        a = (a + n).clamp(-1.0, 1.0)
    return a, ok


@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("nu", [1, 3, 8])
def test_policy_action_beyond_one_control(lib, nu, B):
    """mpcrl_policy_action with 1, 3 and 8 controls and bounds of their own per control, scaled and unscaled, one lane / ragged / full
    workgroups / a second workgroup of one lane, accept_status2 off and on over statuses 0, 1, 2, 4, without noise (unclipped) and with
    noise at noise_clip 0 and 0.5; a NaN, +inf or -inf in ONE control of a row whose status is accepted zeroes the whole row's action
    (0 + noise) and its ok; ok = NULL; sentinel tails.  Bit for bit the torch expressions."""
    gen = torch.Generator(device=DEV).manual_seed(100 * nu + B)
    lo = -1.5 * torch.arange(1, nu + 1, **F64)
    hi = 2.0 * torch.arange(2, nu + 2, **F64)
    sigma = 0.3
    for bad_kind in range(4 if B == 1 else 1):      # (one lane: one launch per non-finite value, and one with none)
        u0 = torch.randn(B, nu, generator=gen, **F64) * 4.0
        status = torch.tensor([0, 1, 2, 4], dtype=torch.int32, device=DEV)[torch.randint(0, 4, (B,), device=DEV, generator=gen)]
        eps = torch.randn(B, nu, device=DEV, generator=gen)
        bad_vals = [float("nan"), float("inf"), float("-inf")]
        bad_rows = [1, B // 2, B - 2]
        if B == 1:
            bad_vals = bad_vals[bad_kind: bad_kind + 1]
            bad_rows = [0] * len(bad_vals)
        if B > 1:
            status[:4] = torch.tensor([0, 1, 2, 4], dtype=torch.int32, device=DEV)      # every status is there
            status[4:8] = torch.tensor([0, 1, 2, 4], dtype=torch.int32, device=DEV)
        for k, (r, v) in enumerate(zip(bad_rows, bad_vals)):
            u0[r, (k + r) % nu] = v
            status[r] = 0 if k != 1 else 2          # accepted statuses: it is the one control that rejects the row
        for scale in (1, 0):
            for acc2 in (0, 1):
                for noise, clip in ((None, 0.0), (eps, 0.0), (eps, 0.5)):
                    a_ref, ok_ref = _policy_reference(u0, status, noise, lo, hi, scale, sigma, clip, acc2)
                    for r, k in zip(bad_rows, range(len(bad_rows))):
                        if k != 1 or acc2:
                            n_r = 0.0 if noise is None else (sigma * eps[r]).clamp(-clip, clip) if clip > 0 else sigma * eps[r]
                            assert not bool(ok_ref[r]) and torch.equal(a_ref[r], (torch.zeros(nu, device=DEV) + n_r).clamp(-1.0, 1.0))
                    for with_ok in (True, False):
                        act = torch.full((B * nu + TAIL,), S_F, dtype=torch.float32, device=DEV)
                        ok = torch.full((B + TAIL,), 77, dtype=torch.uint8, device=DEV)
                        rc = lib.mpcrl_policy_action(_p(u0), _p(status), _p(noise), _p(lo), _p(hi), B, nu, scale, sigma, clip, acc2, _p(act),
                                                     _p(ok) if with_ok else None, _stream())
                        torch.cuda.synchronize()
                        assert rc == 0
                        assert torch.equal(act[: B * nu].view(B, nu), a_ref) and bool((act[B * nu:] == S_F).all())
                        assert torch.equal(ok[:B].bool(), ok_ref) if with_ok else bool((ok[:B] == 77).all())
                        assert bool((ok[B:] == 77).all()) and bool((ok[:B] <= 1).all()) == with_ok
        if B > 1:
            assert all(int((status == s).sum()) > 0 for s in (0, 1, 2, 4))
            assert bool((a_ref.abs() == 1.0).any()) and bool((a_ref.abs() < 1.0).any())      # the final clip binds on some entries only


def test_policy_action_refusals(lib):
    """nu = 0 and a NULL u0, status, lo, hi or action: MPCRL_E_ARG, nothing written.  B = 0: accepted, nothing written."""
    B, nu = 40, 3
    u0, status = torch.randn(B, nu, **F64), torch.zeros(B, dtype=torch.int32, device=DEV)
    lo, hi = -torch.ones(nu, **F64), torch.ones(nu, **F64)
    act, ok = torch.full((B * nu,), S_F, dtype=torch.float32, device=DEV), torch.full((B,), 77, dtype=torch.uint8, device=DEV)
    args = [u0, status, None, lo, hi]
    call = lambda a, B_, nu_, action: lib.mpcrl_policy_action(*[_p(t) for t in a], B_, nu_, 1, 0.1, 0.0, 1, _p(action), _p(ok), _stream())
    assert call(args, B, 0, act) == E_ARG
    for missing in (0, 1, 3, 4):
        a = list(args)
        a[missing] = None
        assert call(a, B, nu, act) == E_ARG, missing
    assert call(args, B, nu, None) == E_ARG
    assert call(args, 0, nu, act) == 0
    torch.cuda.synchronize()
    assert bool((act == S_F).all()) and bool((ok == 77).all())
    assert call(args, B, nu, act) == 0
    torch.cuda.synchronize()
    assert not bool((act == S_F).any()) and bool((ok == 1).all())
