"""bench.py — headline benchmark: MPC + KKT-sensitivity solves per second, cartpole N=20, batch 4096 per GPU.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    (N > 1 without a launcher: bench.py re-executes itself under
     python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...; under a launcher
     (WORLD_SIZE set) it is one rank of that job)

One "step" = one pass of the hot path over one batch of synthetic inputs already resident in HBM: 4096
cartpole OCPs (BASELINE.json config 3: cold-start full SQP to tol 1e-6 + dV/dp + du0*/dp) per GPU, one
kernel launch through the C ABI.  With N > 1 the batch is sharded (weak scaling, 4096 per rank) and the
step ends with the single all-reduce of the accumulated theta-gradient that a data-parallel RL update
needs.  Rank 0 prints ONE JSON line.

Timing (timed_steps): W warm-ups, a barrier + device synchronisation, EXACTLY K timed steps, synchronisation + barrier, MAX over
ranks.  Protocol by round: rounds 1-4 and 6 — the headline's `value` / `ms_per_step` come from that window alone (`settle_steps` 0);
round 5 ran 40 untimed "settle" steps and the HBM-peak probe in front of the warm-ups (an idle GPU reaches its sustained clocks only
after ~20 of these 0.5 ms steps), which this round reports as the separate `steady_state` field, measured by a second window AFTER the
headline's.  The other configurations of BASELINE.json (chain n_mass 5 / 7, linear system, the TD3 closed loop) are measured after
both through the same timed_steps and attached as `secondary` (median of three windows; they keep their disclosed settle steps).

A plain run does only what its headline figure needs: set-up, W warm-ups, the K timed steps, the outputs (--dump-outputs) and the
line.  Everything else it measures — the `steady_state` window, the measured HBM peak (`roofline.peak_measured`), the `secondary`
configurations and the `cpu_baseline` — takes runs of its own and comes only with --full.

--dump-outputs DIR: after the timed steps, what the last timed step returned to its caller (the solver's u0*, V, status, iteration
counts, dV/dp, du0*/dp; for td3 the agent's theta, theta', observations and critic parameters) is written as DIR/<name>.npy in
float32 / float64 (integer outputs as exact float64), so that two builds can be compared output for output on the same seeded inputs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP64_MFMA_PEAK_TFLOPS = 78.6   # AMD spec; probe (profiles/microbench/mfma_f64_4x4x4_probe.hip): one v_mfma_f64_4x4x4 (512 flop) per 18 cycles and SIMD
B_PER_GPU = 4096
N_THETA = 3             # cartpole model parameters (M, m, l)


def algorithmic_bytes_per_solve(N, nx, nu, n_theta, sens):
    """8*[nx + 2*I + nu + 1 + s_V*n_theta + s_pi*nu*n_theta] + 4, I = (N+1)nx + N nu + N nx."""
    iterate = (N + 1) * nx + N * nu + N * nx
    return 8 * (nx + 2 * iterate + nu + 1 + (n_theta + nu * n_theta if sens else 0)) + 4


def make_inputs(B, rank):
    """rng = default_rng(0); theta ~ U(0.9 pi, 1.1 pi), other states 0 (reference reset distribution)."""
    rng = np.random.default_rng(rank)
    x0 = np.zeros((B, 4))
    x0[:, 2] = rng.uniform(0.9 * np.pi, 1.1 * np.pi, B)
    return x0


TRAFFIC_FILE = os.path.join("profiles", "r06_hbm_traffic.json")


def csrc_hash():
    """sha256 over the kernel sources (mpc4rl_amd/csrc/*, include/mpcrl.h), file names included, in sorted order: the counter
    passes store it next to their figures so that a traffic figure is never reported for kernels it was not measured on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "mpc4rl_amd", "csrc")
    srcs = [f for f in sorted(os.listdir(d)) if f.endswith((".hpp", ".hip")) or f == "Makefile"]      # (not the build directories)
    for f in srcs + [os.path.join("..", "..", "include", "mpcrl.h")]:
        h.update(os.path.basename(f).encode())
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def measured_traffic(workload, B, sens, rti):
    """(HBM bytes per step, source) from the committed PMC passes: FETCH_SIZE and WRITE_SIZE collected in separate rocprofv3
    --pmc runs of this very command (profiles/microbench/hbm_traffic.sh), summed over the kernels of one step and corrected as
    MI355X_MICROARCH.md prescribes.  A counter pass cannot run inside a timed bench run, so the figure is read from the file
    that pass wrote; it is only valid for the default batch of each workload AND for the kernel sources it was collected on
    (the file stores their hash: a mismatch returns None rather than a stale figure)."""
    try:
        doc = json.load(open(os.path.join(ROOT, TRAFFIC_FILE)))
        if doc.get("csrc_sha") != csrc_hash():
            return None, None
        d = doc[workload]
        if B != d["batch"] or not sens or rti:
            return None, None
        return float(d["traffic_bytes_per_step"]), TRAFFIC_FILE
    except Exception:
        return None, None


def measured_hbm_peak(dev, nbytes=1 << 30, reps=5):
    """the achievable HBM rate of THIS box from a device-to-device copy (read + write of 1 GiB, HIP events, best of
    `reps` after a warm-up), reported beside the 8 TB/s spec as roofline.peak_measured.  GB/s."""
    try:
        src = torch.empty(nbytes // 8, dtype=torch.float64, device=dev).normal_()
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize(dev)
        best = None
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src)
            b.record()
            torch.cuda.synchronize(dev)
            ms = a.elapsed_time(b)
            best = ms if best is None else min(best, ms)
        del src, dst
        return 2.0 * nbytes / (best * 1e-3) / 1e9
    except Exception:
        return None


def riccati_sweep_flops(N, nx, nu):
    """SURVEY.md §8d (Frison-Jorgensen count): flops of one Riccati sweep (factorisation + solve) of an N-stage problem."""
    return N * (7.0 / 3.0 * nx ** 3 + 4.0 * nx ** 2 * nu + 2.0 * nx * nu ** 2 + nu ** 3 / 3.0) + N * (8.0 * nx ** 2 + 8.0 * nx * nu + 2.0 * nu ** 2)


def usable_cores():
    """Host threads this process may actually use: the cgroup CPU quota if there is one (the GPU boxes expose 256 logical
    CPUs but grant a quota of 16), else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return n


def cpu_baseline(P, x0_np, sens, label="", budget_s=12.0):
    """The oracle's C++ port ("port"; acados cannot be built here: no sources, no network) on this box's host cores, on a bounded
    sample of the same workload: SURVEY.md §8d — same inputs, tolerances and iteration caps, median of up to 10 runs after 2
    warm-ups, all threads and one thread; the sample is sized from a probe so that the whole leg stays within ~budget_s seconds."""
    from oracle import cpu_port
    cores = usable_cores()
    flags = (cpu_port.SENS_V | cpu_port.SENS_PI) if sens else 0
    kw = dict(flags=flags, want_bnd=False)
    def run(n, threads):
        xs = np.tile(x0_np, (-(-n // len(x0_np)), 1))[:n]
        t0 = time.perf_counter()
        r = cpu_port.solve(P, xs, nthreads=threads, **kw)
        return time.perf_counter() - t0, r

    # sample size: doubled from 4 instances per core until one run takes budget / 12 seconds (these runs are the warm-ups)
    n, cap = 4 * cores, 4 * len(x0_np)
    t, _ = run(n, cores)
    t, _ = run(n, cores)
    while t < budget_s / 24.0 and n < cap:
        n = min(cap, 2 * n)
        t, _ = run(n, cores)
    tile = -(-n // len(x0_np))
    times, t_total, r = [], 0.0, None
    while len(times) < 10 and (t_total < 0.7 * budget_s or len(times) < 3):
        t, r = run(n, cores)
        times.append(t)
        t_total += t
    n1 = int(max(2, min(len(x0_np), 0.15 * budget_s * n / (float(np.median(times)) * cores))))
    t1, _ = run(n1, 1)
    one = n1 / t1
    return {"value": n / float(np.median(times)), "unit": "solves/s", "cores": cores, "kind": "port", "single_thread_value": one,
            "sample": f"median of {len(times)} runs x {n} instances after 2 warm-ups ({label}the workload's {len(x0_np)} instances"
                      f"{' tiled' if tile > 1 else ''}; oracle/cpu C++ port, one workspace per thread, OpenMP dynamic over instances; "
                      f"mean SQP iters {float(r.sqp_iter.mean()):.2f}, mean IPM iters {float(r.ipm_iter.mean()):.1f}); "
                      f"single thread: {n1} instances"}


def cpu_baseline_guarded(*a, **k):
    try:
        return cpu_baseline(*a, **k)
    except Exception as e:   # the bench line must still come out
        return {"value": None, "unit": "solves/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {e}"}


def spawn_command(args, argv, port):
    """The torchrun line `bench.py --gpus N` re-executes itself under when no launcher set WORLD_SIZE (one rank per GPU)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def maybe_spawn(args, argv):
    """--gpus N > 1 and not already a rank of a distributed job: become the launcher.  Returns the exit code, or None."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on these hosts (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(spawn_command(args, argv, free_port()), env=env)


def job_aggregate(elapsed_local, dist_mod, device):
    """Contract of the driver: the timed region is bracketed by barriers and its length is the MAX over ranks."""
    if dist_mod is None:
        return float(elapsed_local)
    tt = torch.tensor([elapsed_local], dtype=torch.float64, device=device)
    dist_mod.all_reduce(tt, op=dist_mod.ReduceOp.MAX)
    return float(tt.item())


DRY = bool(os.environ.get("MPCRL_BENCH_DRYRUN"))
STORE_BOUNDS = bool(os.environ.get("MPCRL_BENCH_STORE_BOUNDS"))      # linear workload: write the bound planes back as rounds 2-5 did (A/B of MPCRL_NO_BND_STORE)


def timed_steps(step, args, dist_mod, dev, rank=0):
    """The driver's contract for every workload: W untimed warm-up steps, then EXACTLY K steps bracketed by a barrier + device
    synchronisation on both sides; the job time is the MAX over ranks.  Returns (job seconds, mean HIP-event ms per step or None,
    result of the last step).  Under MPCRL_BENCH_DRYRUN (tests/test_bench_ranks.py: launcher and rank plumbing on CPU, gloo) the
    step is replaced by an uneven sleep, so that the line must carry the slowest rank's time."""
    cuda = dev.type == "cuda"
    sync = (lambda: torch.cuda.synchronize(dev)) if cuda else (lambda: None)
    if DRY:
        step = lambda: time.sleep(1e-3 * (rank + 1))
    r = None
    # settle: untimed steps of the same workload BEFORE the contract's W warm-ups, disclosed in the line as `settle_steps` (--settle 0
    # = none).  A GPU that was idle runs its first ~20 steps of 0.5 ms below its sustained clocks (per-step kernel time 0.555 -> 0.517
    # ms over steps 3..22); with the driver's W = 5, K = 20 the whole timed window sits on that ramp.
    for _ in range(getattr(args, "settle", 0) if not DRY else 0):
        r = step()
    for _ in range(args.warmup):
        r = step()
    sync()
    if dist_mod is not None:
        dist_mod.barrier()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)] if cuda else None
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if ev:
            ev[i][0].record()
        r = step()
        if ev:
            ev[i][1].record()
    sync()
    if dist_mod is not None:
        dist_mod.barrier()
    elapsed = job_aggregate(time.perf_counter() - t0, dist_mod, dev)
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev])) if ev else None
    return elapsed, kern_ms, r


def dry_line(args, world, rccl_ranks, elapsed, metric, secondary=None):
    """What a dry run prints instead of the bench line: the plumbing's figures, no throughput."""
    print(json.dumps({"metric": metric, "value": None, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": 1e3 * elapsed / args.steps, "dryrun": True, "workload": args.workload,
                      **({"rccl_ranks": rccl_ranks} if rccl_ranks is not None else {}),
                      **({"secondary": secondary} if secondary is not None else {})}), flush=True)


DUMP_MAX_BYTES = 64 << 20


def solve_outputs(r):
    """The arrays a caller of MPCBatch.solve receives (SolveResult), by name."""
    return {k: getattr(r, k) for k in ("u0", "V", "status", "iters", "dV_dp", "dpi_dp") if getattr(r, k) is not None}


def dump_outputs(out_dir, arrays, rank):
    """--dump-outputs: one DIR/<name>.npy per array (float32 / float64 as computed, integers as exact float64); the ranks > 0 of a
    multi-GPU job write <name>_rank<r>.npy beside rank 0's."""
    host = {}
    for k, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        host[k] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {DUMP_MAX_BYTES})")
    os.makedirs(out_dir, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ("" if rank == 0 else f"_rank{rank}") + ".npy"), a)


def chain_measure(n_mass, B, sens, steps, warmup, world, rank, dist, dev):
    """One chain_mass measurement through timed_steps: (job seconds, HIP-event ms per step, summary dict for the JSON line, ocp, x0,
    result of the last timed step).
    x0 = masses on the x axis (examples/chain_mass.py:17-25) + N(0, 1e-2) velocity perturbation, seed = rank."""
    from mpc4rl_amd import MPCBatch, chain_mass_ocp
    from mpc4rl_amd.distributed import allreduce_weighted_grad
    ocp = chain_mass_ocp(n_mass=n_mass)
    rng = np.random.default_rng(rank)
    x0 = np.tile(ocp.x0, (B, 1))
    M = n_mass - 2
    x0[:, 3 * (M + 1):] += rng.normal(0.0, 1e-2, (B, 3 * M))
    mpc = MPCBatch(ocp, B, device=dev)
    x0t = torch.as_tensor(x0, device=dev)

    def step():
        r = mpc.solve(x0t, sens_v=sens, sens_pi=sens, cold=True)
        if dist is not None and sens:
            allreduce_weighted_grad(r.dV_dp, r.V)     # local reduction kernel + one all_reduce of n_p + 2 doubles
        return r

    settle = SETTLE["chain"] if SETTLE_OVERRIDE is None else SETTLE_OVERRIDE
    elapsed, kern_ms, r = timed_steps(step, argparse.Namespace(steps=steps, warmup=warmup, settle=settle), dist, dev, rank)
    it = r.iters.cpu().numpy()
    conv = float((r.status == 0).float().mean().item())
    # iterate + outputs, plus the streamed stage factors of every Riccati sweep
    nx, nu, N, n_th = ocp.nx, ocp.nu, ocp.N, ocp.n_p
    b_alg = algorithmic_bytes_per_solve(N, nx, nu, n_th, sens)
    b_sweep = 2 * 8 * N * ((nx + nu) ** 2 + (nx + nu))
    sweeps = float(it[:, 1].mean()) + (1 + nu if sens else 0)
    achieved = (b_alg + sweeps * b_sweep) * B / (kern_ms * 1e-3) / 1e9
    fp64 = sweeps * riccati_sweep_flops(N, nx, nu) * B / (kern_ms * 1e-3) / 1e12
    traffic, traffic_src = measured_traffic(f"chain{n_mass}", B, sens, False)
    summ = {"value": world * B * steps / elapsed, "unit": "solves/s", "steps": steps, "warmup": warmup, "settle_steps": settle, "ms_per_step": 1e3 * elapsed / steps,
            "workload": f"chain_mass n_mass={n_mass} nx={nx} nu={nu} N={N}, {B} instances/GPU, cold-start GN-SQP tol 1e-5"
                        + (f" + dV/dp + du0*/dp ({n_th}-dim p)" if sens else ""),
            "converged_fraction": conv, "sqp_iters_mean": float(it[:, 0].mean()), "ipm_iters_mean": float(it[:, 1].mean()),
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src, "kernel_ms": kern_ms,
                         "algorithmic_bytes_per_solve": b_alg + sweeps * b_sweep, "sweeps_per_solve": sweeps,
                         "fp64": {"achieved": fp64, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": fp64 / FP64_MFMA_PEAK_TFLOPS,
                                  "note": "SURVEY.md 8d: sweeps/s x F_sweep, sweeps = interior-point iterations + 1 + nu"}}}
    del mpc
    return elapsed, kern_ms, summ, ocp, x0, r


def chain_bench(args):
    """BASELINE config 4: chain_mass n_mass = 5 (nx=21) / 7 (nx=33), N=40, batch 1024 PER GPU, GN-SQP tol 1e-5 + sensitivities, "1 -> 8
    GPU scaling".  The instances are independent per parameter point (examples/chain_mass.py:133-174): every rank solves its own
    1024, and a step ends with the ONE all-reduce of the 499- / 1173-dim theta-gradient sum a data-parallel update needs (§8e)."""
    world, rank, local, dist, dev = init_ranks(args)
    rccl_ranks = count_ranks(dist, dev)
    n_mass = 5 if args.workload == "chain5" else 7
    B = args.batch if args.batch != B_PER_GPU else 1024
    sens = not args.no_sens
    metric = f"MPC+KKT-sens solves/sec, chain_mass n_mass={n_mass} N=40 batch={B}"
    if DRY:
        elapsed, _, _ = timed_steps(None, args, dist, dev, rank)
        if rank == 0:
            dry_line(args, world, rccl_ranks, elapsed, metric)
        return finish_ranks(dist)
    elapsed, kern_ms, summ, ocp, x0, r = chain_measure(n_mass, B, sens, args.steps, args.warmup, world, rank, dist, dev)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, solve_outputs(r), rank)
    if rank == 0:
        nx, nu, N, n_th = ocp.nx, ocp.nu, ocp.N, ocp.n_p
        roof = dict(summ["roofline"])
        if args.full:
            peak_meas = measured_hbm_peak(dev)
            roof.update({"peak_measured": peak_meas, "frac_of_measured": (roof["achieved"] / peak_meas) if peak_meas else None})
        out = {"metric": metric, "value": summ["value"],
               "unit": "solves/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "settle_steps": summ["settle_steps"], "ms_per_step": summ["ms_per_step"],
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": summ["workload"],
                          "batch_per_gpu": B, "parallelism": f"instances sharded over {world} GPU(s)"
                          + (f"; one all-reduce of the {n_th}-dim theta-gradient per step" if world > 1 and sens else ""),
                          "converged_fraction": summ["converged_fraction"], "sqp_iters_mean": summ["sqp_iters_mean"],
                          "ipm_iters_mean": summ["ipm_iters_mean"]},
               "roofline": roof}
        if rccl_ranks is not None:
            out["rccl_ranks"] = rccl_ranks
        if world == 1 and args.full and not args.no_cpu:
            from oracle.problems import make_chain_mass
            out["cpu_baseline"] = cpu_baseline_guarded(make_chain_mass(n_mass=n_mass), x0, sens, label=f"chain_mass n_mass={n_mass}: ")
        print(json.dumps(out), flush=True)
    finish_ranks(dist)


def small_measure(linear, B, sens, rti, steps, warmup, world, rank, dist, dev, settle_kind="small"):
    """One cartpole / linear-system measurement through timed_steps: (job seconds, summary dict, ocp, x0, statuses, iteration counts,
    result of the last timed step)."""
    from mpc4rl_amd import MPCBatch, cartpole_ocp, linear_system_ocp
    from mpc4rl_amd.distributed import allreduce_weighted_grad
    n_theta = 12 if linear else N_THETA
    ocp = linear_system_ocp(discount_factor=0.99) if linear else cartpole_ocp()
    mpc = MPCBatch(ocp, B, device=dev)
    if linear:   # the state box of the linear-system environment (linear_system/environment.py: x in [0, 1] x [-1, 1]), interior part
        rng = np.random.default_rng(rank)
        x0_np = np.column_stack([rng.uniform(0.15, 0.85, B), rng.uniform(-0.5, 0.5, B)])
    else:
        x0_np = make_inputs(B, rank)
    x0 = torch.as_tensor(x0_np, device=dev)

    def step():
        # cold start every step (MPC.reset semantics) so that every step does the same, full work
        # (linear system: every step starts cold, so nobody will warm-start an interior point from this solve's bound multipliers
        # and slacks — MPCRL_NO_BND_STORE leaves those ten planes of the stored iterate alone; x, u, pi are still written back)
        r = mpc.solve(x0, sens_v=sens, sens_pi=sens, cold=not rti, rti=rti, store_bounds=not (linear and not rti and not STORE_BOUNDS))
        if dist is not None and sens:
            # data-parallel RL update: one all-reduce of [sum_i dV_i/dtheta, sum_i V_i, count]
            allreduce_weighted_grad(r.dV_dp[:, :n_theta], r.V)   # K5 reduction kernel + one all_reduce of 5 doubles
        return r

    if rti:
        mpc.solve(x0, cold=True)            # converge once; RTI steps then start from that iterate
    settle = settle_kind if isinstance(settle_kind, int) else (SETTLE[settle_kind] if SETTLE_OVERRIDE is None else SETTLE_OVERRIDE)
    elapsed, kern_ms, r = timed_steps(step, argparse.Namespace(steps=steps, warmup=warmup, settle=settle), dist, dev, rank)
    status = r.status.cpu().numpy()
    iters = r.iters.cpu().numpy()
    bytes_per = algorithmic_bytes_per_solve(ocp.N, ocp.nx, ocp.nu, n_theta, sens)
    achieved = bytes_per * B / (kern_ms * 1e-3) / 1e9
    # algorithmic flops = Riccati sweeps x F_sweep, sweeps per solve = interior-point iterations (+ 1 sensitivity
    # factorisation + nu adjoint solves)
    sweeps = float(iters[:, 1].mean()) + (1 + ocp.nu if sens else 0)
    fp64_tflops = sweeps * riccati_sweep_flops(ocp.N, ocp.nx, ocp.nu) * B / (kern_ms * 1e-3) / 1e12
    traffic, traffic_src = measured_traffic("linear" if linear else "cartpole", B, sens, rti)
    if linear and STORE_BOUNDS:
        traffic, traffic_src = None, None      # (the committed counter pass is the MPCRL_NO_BND_STORE form)
    name = "linear system N=40 nx=2 nu=1 (MPCRL_NO_BND_STORE)" if linear and not rti and not STORE_BOUNDS else ("linear system N=40 nx=2 nu=1" if linear else "cartpole N=20 nx=4 nu=1")
    summ = {"value": B * world * steps / elapsed, "unit": "solves/s", "steps": steps, "warmup": warmup, "settle_steps": settle, "ms_per_step": 1e3 * elapsed / steps,
            "workload": ("%s, %d instances/GPU, %s" % (name, B, "RTI (1 SQP iteration, warm)" if rti else "cold-start full-step SQP to tol 1e-6"))
                        + (" + dV/dp + du0*/dp" if sens else ""),
            "converged_fraction": float((status == 0).mean()), "sqp_iters_mean": float(iters[:, 0].mean()),
            "sqp_iters_max": int(iters[:, 0].max()), "ipm_iters_mean": float(iters[:, 1].mean()), "ipm_iters_max": int(iters[:, 1].max()),
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src, "kernel_ms": kern_ms,
                         "algorithmic_bytes_per_solve": bytes_per, "sweeps_per_solve": sweeps,
                         "fp64": {"achieved": fp64_tflops, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": fp64_tflops / FP64_MFMA_PEAK_TFLOPS,
                                  "note": "SURVEY.md 8d: sweeps/s x F_sweep, sweeps = interior-point iterations + 1 + nu; the path is a "
                                          "serial dependency chain, not flop-bound"}}}
    del mpc
    return elapsed, summ, ocp, x0_np, status, iters, r


SECONDARY = (("chain5", 10, 3), ("chain7", 5, 2), ("linear", 50, 5), ("td3", 20, 5))   # (workload, steps, warm-ups): BASELINE configs 4, 1, 5
SECONDARY_WINDOWS = 3
# Untimed "settle" steps in front of the W warm-ups (timed_steps), disclosed in every line as `settle_steps`; --settle N overrides.
# The HEADLINE line runs none (round 6: the driver's W and K are the whole protocol, as in rounds 1-4; round 5's headline ran 40 and
# its figure is the `steady_state` field of this round's line).  The non-headline workloads keep theirs: they are measured after the
# headline's region or by their own command lines, never by the driver's contract.
SETTLE = {"headline": 0, "small": 40, "chain": 3, "td3": 10}
STEADY_SETTLE = 40          # the headline's second, separately labelled window (`steady_state`)
SETTLE_OVERRIDE = None


def secondary_lines(world, rank, dist, dev):
    """The other single-GPU configurations of BASELINE.json, measured by the SAME timed_steps right after the headline's timed region,
    so that the driver's one bench run also times them: chain n_mass 5 / 7 at 1024 instances + sensitivities (config 4), the
    linear-system OCP at 4096 (config 1 batched), the TD3 closed loop at 4096 environments with HIP graphs (config 5: ms_per_step,
    env-steps/s, mpc_solves_per_s, the launch-shape probe times of its three solves).  Solver entries: ms_per_step, value (solves/s),
    iteration counts, roofline {frac, traffic}."""
    out = {}
    for wl, steps, warmup in SECONDARY:
        try:
            if DRY:
                elapsed, _, _ = timed_steps(None, argparse.Namespace(steps=steps, warmup=warmup), dist, dev, rank)
                out[wl] = {"ms_per_step": 1e3 * elapsed / steps, "steps": steps, "warmup": warmup, "dryrun": True}
            else:
                # MEDIAN of SECONDARY_WINDOWS windows of `steps` steps each (every window is a full timed_steps call: warm-up, barrier,
                # synchronise, exactly `steps` steps): these windows are 25-90 ms long, and on some boxes a ~31 ms stall BETWEEN launches
                # (kernels and per-wavefront lifetimes unchanged: profiles/r05_stall_probe.txt) tripled a figure now and then.  The
                # headline and the --workload lines keep the contract's single window.
                wins = []
                for _ in range(SECONDARY_WINDOWS):
                    if wl == "linear":
                        wins.append(small_measure(True, B_PER_GPU, True, False, steps, warmup, world, rank, dist, dev)[1])
                    elif wl == "td3":      # config 5 at its per-GPU size, HIP graphs on (the step a training loop runs)
                        wins.append(td3_measure(B_PER_GPU, steps, warmup, True, world, rank, dist, dev, SETTLE["td3"])[1])
                        if len(wins) == SECONDARY_WINDOWS:      # one window of the rounds 2-5 form (cold replay solves) beside it
                            cold_ms = td3_measure(B_PER_GPU, steps, warmup, True, world, rank, dist, dev, SETTLE["td3"], replay_iterates=False)[1]["ms_per_step"]
                            # and one of the opt-in pipelined loop (the update beside the roll-out step, one rank: BatchedTD3(pipeline=True))
                            pipe_ms = td3_measure(B_PER_GPU, steps, warmup, True, world, rank, dist, dev, SETTLE["td3"], pipeline=True)[1]["ms_per_step"] if world == 1 else None
                    else:
                        wins.append(chain_measure(int(wl[5:]), 1024, True, steps, warmup, world, rank, dist, dev)[2])
                wins.sort(key=lambda w: w["ms_per_step"])
                out[wl] = wins[len(wins) // 2]
                out[wl]["windows_ms_per_step"] = [w["ms_per_step"] for w in wins]
                out[wl]["statistic"] = "median of %d windows of %d steps" % (SECONDARY_WINDOWS, steps)
                if wl == "td3":
                    out[wl]["cold_replay_ms_per_step"] = cold_ms
                    out[wl]["pipelined_ms_per_step"] = pipe_ms
        except Exception as e:   # the headline line must still come out
            out[wl] = {"value": None, "error": repr(e)}
    return out


class _StdoutToStderr:
    """Sends everything written to file descriptor 1 (C libraries included) to stderr for the duration of the block: RCCL prints a
    banner when its first communicator is created, and stdout has to carry exactly ONE JSON line."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)


def init_ranks(args):
    """(world, rank, local, dist module or None, device): one process per GPU, RCCL ("nccl") when there is more than one rank.
    Dry run (no GPU): the same rendezvous over gloo, device = cpu."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(1, args.gpus) and not os.environ.get("MPCRL_BENCH_FORCE_DIST"):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)")
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if DRY:
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
            dist.barrier()
        return world, rank, local, dist, torch.device("cpu")
    if os.environ.get("MPCRL_BENCH_SHARE_GPU"):   # test-only: several ranks on one device (tests/test_gpu_fullsize.py, a 1-GPU box)
        local = local % max(1, torch.cuda.device_count())
    if world > 1 or os.environ.get("MPCRL_BENCH_FORCE_DIST"):   # the env switch lets a 1-GPU box exercise the RCCL path
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        with _StdoutToStderr():
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            probe = torch.zeros(1, device=torch.device("cuda", local))
            dist.all_reduce(probe)             # creates the communicator now (and has RCCL say what it has to say)
            torch.cuda.synchronize()
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback)"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    return world, rank, local, dist, dev


def finish_ranks(dist_mod):
    if dist_mod is not None:
        dist_mod.destroy_process_group()


def count_ranks(dist_mod, dev):
    """Number of ranks in the job's communicator as the collective itself reports it (all-reduce of ones), or None without one."""
    if dist_mod is None:
        return None
    one = torch.ones(1, dtype=torch.float64, device=dev)
    dist_mod.all_reduce(one)
    return int(round(float(one.item())))


def td3_measure(E, steps, warmup, graphs, world, rank, dist, dev, settle, replay_iterates=True, pipeline=False):
    """One TD3 closed-loop measurement through timed_steps: (job seconds, summary dict, the agent's state after the last timed step).
    A step = one environment step of all E environments + one TD3 update (batch E per rank); MPC solves per step and rank: E warm
    (roll-out actor) + E cold (target actor) + E / policy_delay cold with du0*/dtheta (policy gradient)."""
    from mpc4rl_amd import BatchedCartPoleSwingUpEnv, BatchedTD3, cartpole_ocp
    env = BatchedCartPoleSwingUpEnv(E, device=dev, seed=rank)
    agent = BatchedTD3(cartpole_ocp(), env, batch_size=E, buffer_steps=64, policy_delay=2, lr_actor=1e-6, seed=0, device=dev,
                       replay_iterates=replay_iterates, pipeline=pipeline and graphs and world == 1)
    agent.collect(4)                       # something to sample from
    if graphs:
        agent.enable_graphs()              # fills the replay buffer, then captures the roll-out step and the update into HIP graphs

    def step():                            # no host synchronisation inside the timed region: statistics are read after it
        agent.step()                       # = collect(1) + train(1); with graphs on one rank: one graph replay

    # the warm-up steps run here: the roll-out statistics are zeroed where the timed region starts
    for _ in range(settle + warmup):
        step()
    agent.collect(0)                       # zero the roll-out statistics
    elapsed, _, _ = timed_steps(step, argparse.Namespace(steps=steps, warmup=0), dist, dev, rank)
    state = {"theta": agent.theta.clone(), "theta_target": agent.theta_target.clone(), "obs": agent.obs.clone(),
             "critic_params": torch.cat([p.detach().reshape(-1) for p in agent.critic.parameters()])}
    st = agent.last_stats()
    tr = {"critic_loss": agent.last_critic_loss()} if agent._graphs else agent.train(1)
    solves = world * steps * (E + E + E / agent.policy_delay)
    summ = {"value": world * E * steps / elapsed, "unit": "env-steps/s", "steps": steps, "warmup": warmup, "settle_steps": settle,
            "ms_per_step": 1e3 * elapsed / steps,
            "workload": f"cartpole TD3 closed loop (BASELINE config 5): {E} environments/GPU, one environment step + one "
                        f"TD3 update (batch {E}, policy_delay 2) per step; MPC solves per step and GPU: {E} warm (actor) "
                        + (f"+ {E} (target actor) + {E // 2} with du0*/dtheta (policy gradient), both started from the roll-out "
                           f"policy's stored iterate of the sampled transition (replay_iterates); " if replay_iterates else
                           f"+ {E} cold (target actor) + {E // 2} cold with du0*/dtheta (policy gradient); ")
                        + ("roll-out step and update replayed as HIP graphs" if graphs else "eager launches")
                        + ("; PIPELINED (opt-in): the update runs beside the roll-out step of the same call and samples the replay table "
                           "without the slot being written" if agent.pipeline else ""),
            "mpc_solves_per_s": solves / elapsed, "converged_fraction": st["converged_fraction"], "critic_loss": tr["critic_loss"],
            "replay_iterates": bool(replay_iterates), "pipeline": bool(agent.pipeline),
            # launch shape of the solves (mpcrl_set_launch_mode 0): probe times in ms of the two shapes and the one in use
            "replay_launch_shape": {"target_actor": list(agent.target_mpc.mpc.launch_times()), "policy": list(agent.pi_mpc.mpc.launch_times()),
                                    "rollout_warm": list(agent.actor.mpc.launch_times(warm=True))}}
    del agent, env
    return elapsed, summ, state


def td3_bench(args):
    """BASELINE config 5: cartpole TD3 closed loop — 4096 batched environments per GPU, the MPC as the actor (one launch per
    environment step, warm-started, cold only where an episode ended), device replay, critic TD update with the target actor's
    batched solve, delayed deterministic policy gradient through du0*/dtheta, ONE all-reduce (critic gradients + theta-gradient)
    per update.  A step = one environment step of all environments + one TD3 update (batch 4096 per rank)."""
    world, rank, local, dist, dev = init_ranks(args)
    rccl_ranks = count_ranks(dist, dev)
    metric = "closed-loop environment steps/sec, cartpole TD3 with the MPC as actor"
    if DRY:
        elapsed, _, _ = timed_steps(None, args, dist, dev, rank)
        if rank == 0:
            dry_line(args, world, rccl_ranks, elapsed, metric)
        return finish_ranks(dist)
    settle = SETTLE["td3"] if SETTLE_OVERRIDE is None else SETTLE_OVERRIDE
    elapsed, summ, state = td3_measure(args.batch, args.steps, args.warmup, not args.no_graph, world, rank, dist, dev, settle,
                                       replay_iterates=not args.cold_replay, pipeline=args.td3_pipeline)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, state, rank)
    if rank == 0:
        print(json.dumps({
            "metric": metric, "value": summ["value"],
            "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "settle_steps": settle, "ms_per_step": summ["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": summ["workload"],
                       "parallelism": f"environments sharded over {world} GPU(s); one all-reduce of the critic + theta gradients per update",
                       "mpc_solves_per_s": summ["mpc_solves_per_s"], "converged_fraction": summ["converged_fraction"],
                       "critic_loss": summ["critic_loss"], "replay_launch_shape": summ["replay_launch_shape"]},
            **({"rccl_ranks": rccl_ranks} if rccl_ranks is not None else {})}), flush=True)
    finish_ranks(dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=B_PER_GPU)
    ap.add_argument("--no-sens", action="store_true", help="forward solve only (BASELINE config 2)")
    ap.add_argument("--rti", action="store_true", help="one SQP iteration from the stored iterate (build-side mode)")
    ap.add_argument("--full", action="store_true", help="also measure what the headline figure does not need: the steady_state window, "
                    "the measured HBM peak, the secondary configurations and the CPU baseline (a plain run does none of them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step returned "
                    "as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--settle", type=int, default=-1, help="untimed steps before the W warm-ups that bring an idle GPU to its sustained "
                    "clocks (reported as settle_steps); -1 = per workload (headline 0 + with --full a separate steady_state window, "
                    "linear 40, chain 3, TD3 10), 0 = none anywhere")
    ap.add_argument("--no-secondary", action="store_true", help="--full headline run: skip the chain5 / chain7 / linear / td3 figures "
                    "measured after the headline's timed region and attached to the line as `secondary`")
    ap.add_argument("--no-graph", action="store_true", help="td3 workload: eager launches instead of replayed HIP graphs")
    ap.add_argument("--td3-pipeline", action="store_true", help="td3 workload, one rank, graphs on: BatchedTD3(pipeline=True) — the update runs beside the "
                    "roll-out step of the same call (pipelined actor / learner: the sampler leaves out the slot being written; same work per step)")
    ap.add_argument("--cold-replay", action="store_true", help="td3 workload: the two replay solves of an update start cold (rounds 2-5) "
                    "instead of from the roll-out policy's stored iterates")
    ap.add_argument("--workload", default="cartpole", choices=["cartpole", "linear", "chain5", "chain7", "td3"],
                    help="cartpole = the headline metric (default); linear = the 2-state OCP of config 1 batched; chain5/chain7 = BASELINE "
                         "config 4; td3 = config 5 (none of these is the headline line)")
    args = ap.parse_args()
    global SETTLE_OVERRIDE
    SETTLE_OVERRIDE = None if args.settle < 0 else args.settle
    rc = maybe_spawn(args, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)
    if args.workload == "td3":
        return td3_bench(args)
    if args.workload in ("chain5", "chain7"):
        return chain_bench(args)
    linear = args.workload == "linear"

    world, rank, local, dist, dev = init_ranks(args)
    rccl_ranks = count_ranks(dist, dev)

    B = args.batch
    sens = not args.no_sens
    metric = ("MPC+KKT-sens solves/sec, %s batch=%d" if sens else "MPC solves/sec, %s batch=%d") % (
        "linear_system N=40" if linear else "cartpole N=20", B)
    want_secondary = args.full and not args.no_secondary and not linear and world == 1 and sens and not args.rti and B == B_PER_GPU
    if DRY:
        elapsed, _, _ = timed_steps(None, args, dist, dev, rank)
        sec = secondary_lines(world, rank, dist, dev) if want_secondary else None
        if rank == 0:
            dry_line(args, world, rccl_ranks, elapsed, metric, sec)
        return finish_ranks(dist)
    # The headline: the driver's contract and nothing else — W warm-ups, then EXACTLY K timed steps (no settle steps, the HBM probe
    # after the region).  With W = 5, K = 20 the 10 ms window sits on the clock ramp of a GPU that was idle; what the
    # same binary does once the clocks have settled is measured (--full) by a SECOND window after it and reported as `steady_state`, a
    # separately labelled field that never feeds `value` / `ms_per_step`.
    headline = not linear
    elapsed, summ, ocp, x0_np, status, iters, r = small_measure(linear, B, sens, args.rti, args.steps, args.warmup, world, rank, dist, dev,
                                                                settle_kind="headline" if headline else "small")
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, solve_outputs(r), rank)
    steady, peak_meas = None, None
    if args.full and headline and SETTLE_OVERRIDE is None:
        s_el, s_summ = small_measure(linear, B, sens, args.rti, args.steps, args.warmup, world, rank, dist, dev, settle_kind=STEADY_SETTLE)[:2]
        steady = {"ms_per_step": s_summ["ms_per_step"], "value": s_summ["value"], "unit": "solves/s", "settle_steps": STEADY_SETTLE,
                  "steps": args.steps, "warmup": args.warmup, "kernel_ms": s_summ["roofline"]["kernel_ms"],
                  "note": "the same workload and W / K measured again after the headline's region and %d more untimed steps (sustained "
                          "clocks): round 5's headline protocol; not part of value / ms_per_step" % STEADY_SETTLE}
    if args.full:
        peak_meas = measured_hbm_peak(dev)
    # the headline's timed region is over: the other configurations are measured after it, never inside it
    sec = secondary_lines(world, rank, dist, dev) if want_secondary else None

    if rank == 0:
        kern_ms = summ["roofline"]["kernel_ms"]
        # matrix-core work of the factor sweep: 6 v_mfma_f64_4x4x4 block-products (128 flop each) per stage step and instance
        mfma_tflops = 0.0 if linear else float(iters[:, 1].sum()) * ocp.N * 6 * 128 / (kern_ms * 1e-3) / 1e12
        roof = dict(summ["roofline"])
        if args.full:
            roof.update({"peak_measured": peak_meas, "frac_of_measured": (roof["achieved"] / peak_meas) if peak_meas else None})
        roof["mfma_f64_hw"] = {"achieved": mfma_tflops, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": mfma_tflops / FP64_MFMA_PEAK_TFLOPS,
                               "note": "hardware flops of the 6 v_mfma_f64_4x4x4 per factor-sweep stage step (padded 4x4x4 "
                                       "products; vector sweeps excluded): the MFMAs of the recursion wait on each other"}
        out = {
            "metric": metric,
            "value": summ["value"], "unit": "solves/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "settle_steps": summ["settle_steps"],
            "ms_per_step": summ["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": summ["workload"] + ("" if linear else (" (BASELINE config 3)" if sens else " (BASELINE config 2)")),
                       "batch_per_gpu": B, "parallelism": f"instances sharded over {world} GPU(s)" +
                       ("; one all-reduce of the theta-gradient per step" if world > 1 and sens else ""),
                       "converged_fraction": summ["converged_fraction"], "sqp_iters_mean": summ["sqp_iters_mean"],
                       "sqp_iters_max": summ["sqp_iters_max"], "ipm_iters_mean": summ["ipm_iters_mean"],
                       "ipm_iters_max": summ["ipm_iters_max"]},
            "roofline": roof,
        }
        if rccl_ranks is not None:
            out["rccl_ranks"] = rccl_ranks   # an all-reduce of ones over the job's communicator: how many ranks RCCL really joined
        if world == 1 and args.full and not args.no_cpu:
            from oracle.problems import make_cartpole, make_linear_system
            out["cpu_baseline"] = cpu_baseline_guarded(make_linear_system(gamma=0.99) if linear else make_cartpole(), x0_np, sens)
        if steady is not None:
            out["steady_state"] = steady
        if sec is not None:
            out["secondary"] = sec
        print(json.dumps(out), flush=True)
    finish_ranks(dist)


if __name__ == "__main__":
    main()
