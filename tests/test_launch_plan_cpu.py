"""The launch plan of the small-model solves (csrc/launch_plan.hpp) on the CPU: no device, no handle.

mpcrl_debug_launch_plan runs plan_small — the function mpcrl_solve and mpcrl_query_time_sliced decide with — on plain numbers; here it
is swept against the independent restatement of tests/launch_plan_cases.py over every horizon, the batch sizes either side of a round
of wavefronts, every flag subset, the three launch modes, both bound patterns, both linear-system settings and both tuner shapes, every
field compared; the cases that matter are pinned by literal.  The tuner's arithmetic (tuned_shape, tuned_best) has no export: a probe
program is compiled from the header with the host compiler alone, which also shows that the header needs nothing from HIP."""
import ctypes
import itertools
import os
import subprocess

import pytest

import launch_plan_cases as P
from launch_plan_cases import COLD, EXACT, EXACT_QP, LQ, PLAIN, RTI, SENS_PI, SLICED, TUNE_PLAIN, TUNE_SLICED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc4rl_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from mpc4rl_amd import _lib
    return _lib.load()


def plan(lib, model, N, B=4096, n_simd=1024, flags=COLD | SENS_PI, slice_mode=0, box_rows=1, linear_spl=3, shape=TUNE_SLICED):
    out = (ctypes.c_int32 * 12)()
    assert lib.mpcrl_debug_launch_plan(P.MODELS[model]["id"], N, B, n_simd, flags, slice_mode, box_rows, linear_spl, shape, out) == 0
    return dict(zip(P.FIELDS, out))


@pytest.mark.parametrize("model", sorted(P.MODELS))
def test_sweep_against_the_restatement(lib, model):
    out = (ctypes.c_int32 * 12)()
    mid, n, families = P.MODELS[model]["id"], 0, set()
    for args in itertools.product(P.SWEEP_N, P.SWEEP_B, P.SWEEP_SIMD, P.SWEEP_FLAGS, P.SWEEP_MODE, (0, 1), (1, 3), (TUNE_SLICED, TUNE_PLAIN)):
        assert lib.mpcrl_debug_launch_plan(mid, *args, out) == 0, args
        got, want = list(out), P.expected(model, *args)
        assert got == want, (model, args, dict(zip(P.FIELDS, got)), dict(zip(P.FIELDS, want)))
        families.add(got[0])
        n += 1
    assert n == 62 * 7 * 2 * 16 * 3 * 2 * 2 * 2
    assert families == ({PLAIN, SLICED, EXACT} if model == "cartpole" else {PLAIN, LQ})


def test_arguments(lib):
    out = (ctypes.c_int32 * 12)()
    ok = dict(model=0, N=20, B=8, n_simd=1024, flags=0, slice_mode=0, box_rows=0, linear_spl=3, shape=0)
    assert lib.mpcrl_debug_launch_plan(*ok.values(), out) == 0
    for bad in (dict(model=2), dict(model=-1), dict(N=1), dict(N=64), dict(B=0), dict(n_simd=0), dict(slice_mode=2), dict(shape=2)):
        assert lib.mpcrl_debug_launch_plan(*{**ok, **bad}.values(), out) == -1, bad
    assert lib.mpcrl_debug_launch_plan(*ok.values(), None) == -1


def test_cartpole_pins(lib):
    p = plan(lib, "cartpole", 20)      # the benchmark: 4096 instances are one round of 1024 four-instance wavefronts
    assert p == dict(family=SLICED, seg_short=1, box=1, lds_park=1, warm=0, lq_spl=0, lq_rl=0, grid=1024, sens_grid=1366, candidate=1, by_rule=1,
                     reserved=0)
    assert plan(lib, "cartpole", 20, shape=TUNE_PLAIN)["family"] == PLAIN and plan(lib, "cartpole", 20, shape=TUNE_PLAIN)["grid"] == 1366
    assert plan(lib, "cartpole", 20, box_rows=0)["box"] == 0 and plan(lib, "cartpole", 20, flags=SENS_PI)["warm"] == 1
    big = plan(lib, "cartpole", 20, B=32768)      # 8 rounds against 11: the rule keeps the plain launch
    assert (big["candidate"], big["by_rule"], big["family"], big["grid"]) == (1, 0, PLAIN, 10923)
    small = plan(lib, "cartpole", 20, B=96)
    assert (small["candidate"], small["by_rule"], small["family"]) == (1, 0, PLAIN)
    assert plan(lib, "cartpole", 20, B=96, slice_mode=1)["family"] == SLICED and plan(lib, "cartpole", 20, slice_mode=-1)["family"] == PLAIN
    for N in (31, 63):      # 2 x 32 and 1 x 64 lanes: no lane left for the parked instance
        assert plan(lib, "cartpole", N, slice_mode=1)["candidate"] == 0 and plan(lib, "cartpole", N, slice_mode=1)["family"] == PLAIN
    assert plan(lib, "cartpole", 62, slice_mode=1)["candidate"] == 1 and plan(lib, "cartpole", 62, slice_mode=1)["family"] == SLICED
    for N in range(2, 64):
        p = plan(lib, "cartpole", N, slice_mode=1)
        assert p["seg_short"] == (1 if N <= 31 else 0), N
        if N not in (31, 63):
            assert (p["family"], p["lds_park"]) == (SLICED, 1 if N <= 20 else 0), N
        for mode in (-1, 0, 1):      # an RTI call is never time-sliced
            assert plan(lib, "cartpole", N, flags=RTI | SENS_PI, slice_mode=mode)["family"] == PLAIN
    e = plan(lib, "cartpole", 20, flags=COLD | SENS_PI | EXACT_QP, slice_mode=1)
    assert (e["family"], e["grid"], e["sens_grid"], e["box"], e["candidate"]) == (EXACT, 1366, 1366, 0, 0)


def test_linear_pins(lib):
    for N in range(2, 64):
        p = plan(lib, "linear", N, slice_mode=1)
        want = (PLAIN, 0, 0) if N <= 7 else (LQ, 3, 8) if N <= 23 else (LQ, 3, 16) if N <= 47 else (LQ, 4, 16)
        assert (p["family"], p["lq_spl"], p["lq_rl"]) == want, N
        assert (p["candidate"], p["box"], p["seg_short"], p["lds_park"]) == (0, 0, 0, 0), N      # never sliced, never BOX, never SHORT
        assert p["sens_grid"] == (0 if p["family"] == LQ else -(-4096 // min(64 // (N + 1), 21))), N
        assert p["grid"] == -(-4096 // (64 // p["lq_rl"])) if p["family"] == LQ else p["grid"] == p["sens_grid"], N
        one = plan(lib, "linear", N, linear_spl=1)
        assert (one["family"], one["grid"], one["sens_grid"]) == (PLAIN,) + 2 * (-(-4096 // min(64 // (N + 1), 21)),), N


PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "launch_plan.hpp"
#ifdef __HIP__
#error "the probe is built by the host compiler alone"
#endif
int main(int argc, char **argv) {
    std::printf("%d %.9g\n", (int)mpcrl::TUNE_PERIOD, (double)mpcrl::TUNE_MARGIN);
    for (int i = 1; i + 2 < argc; i += 3) {
        mpcrl::TunerState t;
        t.calls = (unsigned)std::strtoul(argv[i], nullptr, 10), t.ms[0] = std::strtof(argv[i + 1], nullptr), t.ms[1] = std::strtof(argv[i + 2], nullptr);
        bool timed = false;
        const int shape = mpcrl::tuned_shape(t, &timed);
        std::printf("%d %d %d\n", shape, (int)timed, mpcrl::tuned_best(t));
    }
    mpcrl::TunerState fresh;
    std::printf("%u %g %g\n", fresh.calls, fresh.ms[0], fresh.ms[1]);
    return 0;
}
"""


def test_tuner_from_the_header_alone(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    prefers_plain, prefers_sliced = (100.0, 79.9), (100.0, 80.1)      # either side of the 0.80 margin
    cases = [(c, *ms) for ms in ((-1.0, -1.0), prefers_plain, prefers_sliced) for c in (0, 1, 2, 3, 64, 65, 66)]
    cases += [(7, -1.0, 50.0), (7, 100.0, -1.0), (7, 100.0, 80.0), (7, 100.0, 0.0)]      # one time unknown; on the margin; a zero time
    lines = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0].split() == ["64", "0.800000012"]
    for c, line in zip(cases, lines[1:]):
        assert tuple(int(v) for v in line.split()) == P.tuner(*c), (c, line)
    assert lines[1 + len(cases)].split() == ["0", "-1", "-1"]      # a fresh tuner: nothing timed
    # and by literal: probes at calls 1, 2 (65, 66) whatever the times say; otherwise plain only beyond the margin
    got = {c: tuple(int(v) for v in line.split()) for c, line in zip(cases, lines[1:])}
    for ms, best in (((-1.0, -1.0), TUNE_SLICED), (prefers_plain, TUNE_PLAIN), (prefers_sliced, TUNE_SLICED)):
        assert [got[(c, *ms)] for c in (0, 1, 2, 3, 64, 65, 66)] == [(best, 0, best), (TUNE_SLICED, 1, best), (TUNE_PLAIN, 1, best), (best, 0, best)] + \
            [(best, 0, best), (TUNE_SLICED, 1, best), (TUNE_PLAIN, 1, best)]
    assert [got[c][2] for c in cases[-4:]] == [TUNE_SLICED] * 4
