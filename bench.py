#!/usr/bin/env python3
"""bench.py — control-ticks/sec of the batched operational-space controller on MI355X.

One "step" = one fused tick (Sai2Model::updateModel + RobotController::updateControllerTaskModels +
computeControlTorques, reference src/RobotController.cpp:53-74) over one batch of synthetic robots.
Workload at every N: BASELINE.json configs[2] — 65 536 batched 7-DOF Panda per GPU,
MotionForceTask + nullspace JointTask (SURVEY.md §8(d) "C3"); N > 1 shards the batch with no
collective on the data path (weak scaling, "C5" at N = 8).

Inputs are resident in HBM before the timed region; the timed region is K launches bracketed by a
barrier + device synchronize, MAX over ranks. Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

BYTES_PER_TICK = {2: 360, 3: 528, 4: 576, 5: 528}  # inputs + outputs per tick, doubles x 8
FLOP_PER_TICK = 11.4e3  # SURVEY.md §8(d), SVD iterations excluded
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_VECTOR_PEAK_TFLOPS = 78.6


PMC_KERNEL = {2: "tick_fast_kernel<1", 3: "tick_fast_kernel<2", 4: "tick_cert_kernel", 5: "tick_fast_kernel<2"}


def pmc_traffic_bytes(config):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary of this config's bench
    command (profiles/r<round>_c<config>_counters.json, the latest round; FETCH_SIZE and WRITE_SIZE are collected in
    separate passes and reported in KB; FETCH_SIZE under-reads coalesced streams by 2x on gfx950:
    MI355X_MICROARCH.md §HBM). None when no summary is committed."""
    import glob

    c = 3 if config == 5 else config
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_c{c}_counters.json")))
    if not files:
        return None
    data = json.load(open(files[-1]))
    for name, cnt in data.items():
        if PMC_KERNEL[config] in name and "FETCH_SIZE" in cnt and "WRITE_SIZE" in cnt:
            return (2 * cnt["FETCH_SIZE"]["avg_per_dispatch"] + cnt["WRITE_SIZE"]["avg_per_dispatch"]) * 1024
    return None


def cpu_baseline(inp, seconds=8.0):
    """the CPU oracle (our FP64 restatement of the reference, -O2) timed on this host's cores on a
    bounded sample of the same workload"""
    import oracle_lib as ol
    import sai2_primitives_perso_amd as pkg

    sample = min(8192, inp["B"])
    sub = {"B": sample, "tasks": inp["tasks"], "q": np.ascontiguousarray(inp["q"][:, :sample]),
           "dq": np.ascontiguousarray(inp["dq"][:, :sample])}
    for t, (kind, _) in enumerate(inp["tasks"]):
        key = f"{kind}{t}"
        sub[key] = {k: np.ascontiguousarray(v[:, :sample]) for k, v in inp[key].items()}
    # a 1-GPU box shares its host: use at most the 16-core share of one GPU
    cores = min(len(os.sched_getaffinity(0)), 16)
    res = {}
    for label, threads in (("single", 1), ("all", cores)):
        o = ol.Oracle(ol.panda_model(), ol.task_configs(sub["tasks"]), sample, threads=threads)
        pkg.workloads.load_inputs(o, sub)
        o.tick(want_output=False)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds / 2:
            o.tick(want_output=False)
            n += 1
        res[label] = n * sample / (time.perf_counter() - t0)
        o.close()
    return {
        "value": res["all"],
        "unit": "control-ticks/sec",
        "cores": cores,
        "kind": "port",
        "single_thread_value": res["single"],
        "sample": f"first {sample} robots of the same workload, repeated ticks for ~{seconds / 2:.0f} s per leg "
                  f"(1 thread, then OpenMP over {cores} threads); oracle/sai2_oracle.c, gcc -O2",
    }


PREROLL_S = 0.25  # untimed device work before the warm-up ticks (see main)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, ctrl, rank, world):
    """What the timed path hands its caller: the torques of the last tick, left in the ctx buffer SAI2B_BUF_TAU
    ([7][B] float64 on the device). Written as DIR/tau.npy (DIR/tau_rank<r>.npy per rank when N > 1). Over the
    64 MB budget (split between ranks) a fixed seeded sample of robots is written instead, in robot order."""
    import sai2_primitives_perso_amd as pkg

    ctrl.synchronize()
    ptr = ctrl.device_buffer(pkg._abi.BUF_TAU)

    class _Tau:  # zero-copy torch view of the library's torque buffer
        __cuda_array_interface__ = {"data": (int(ptr), False), "shape": (ctrl.dof, ctrl.B), "typestr": "<f8", "version": 2}

    tau = torch.as_tensor(_Tau(), device="cuda").cpu().numpy()
    max_robots = DUMP_LIMIT_BYTES // world // tau[:, :1].nbytes
    if ctrl.B > max_robots:
        tau = tau[:, np.sort(np.random.default_rng(0).choice(ctrl.B, max_robots, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "tau.npy" if world == 1 else f"tau_rank{rank}.npy"), np.ascontiguousarray(tau))


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N rank processes of this same script (rank r on
    GPU r, rendezvous on 127.0.0.1), relay their output (rank 0 prints the JSON line) and return the worst
    exit code. Runs before anything initialises the GPU in this process."""
    import socket
    import subprocess

    n = args.gpus
    if not args.single_device and torch.cuda.device_count() < n:
        print(f"bench.py: --gpus {n} but only {torch.cuda.device_count()} GPU(s) visible", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=None, help="robots per GPU (default: the config's size; 65536 for C3)")
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="gloo",
                    help="torch.distributed backend of the timing protocol for N > 1 (a barrier and a MAX of four scalars: "
                         "the path has no exchange step, so no RCCL communicator is set up by default; nccl = RCCL)")
    ap.add_argument("--single-device", action="store_true", help="rehearsal only: every rank uses cuda:0")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the torques of the last timed step to DIR/tau.npy (float64 [7][B], "
                         "at most 64 MB; one file per rank, DIR/tau_rank<r>.npy, when N > 1)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher. Nothing has touched the GPU yet
        # (device_count() does not initialise it), the ranks are fresh child processes, never an exec.
        raise SystemExit(spawn_ranks(args))

    import sai2_primitives_perso_amd as pkg

    rank, local_rank, world = pkg.sharding.env_rank()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    if args.single_device:
        local_rank = 0
    elif torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} GPU(s) visible "
                         "(--single-device rehearses every rank on cuda:0)")
    distributed = world > 1
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    torch.cuda.set_device(local_rank)
    pkg.sharding.init(args.backend, local_rank)  # no-op when WORLD_SIZE == 1
    red_device = "cuda" if args.backend == "nccl" else "cpu"

    B = args.batch or (65536 if args.config in (3, 5) else pkg.workloads.CONFIG_BATCH[args.config])
    inp = pkg.workloads.make_inputs(args.config if args.config != 5 else 3, B=B, rank=rank)
    ctrl = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=local_rank)

    pkg.workloads.load_inputs(ctrl, inp)  # H2D once: inputs are resident before the timed region
    ctrl.synchronize()
    stream = torch.cuda.ExternalStream(ctrl.stream(), device=torch.device("cuda", local_rank))

    def barrier():
        ctrl.synchronize()
        torch.cuda.synchronize()
        pkg.sharding.barrier()

    # Clock pre-roll: the device's clock governor settles only after tens of ms of sustained work, far more than W
    # warm-up ticks at the defaults (a few hundred us). A twin context (same kernels, same batch, a state of its own)
    # ticks back to back for PREROLL_S first, so the measured controller still runs exactly warmup + steps ticks.
    twin = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=local_rank)
    pkg.workloads.load_inputs(twin, inp)
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < PREROLL_S:
        for _ in range(32):
            twin.tick(want_output=False)
        twin.synchronize()
    twin.close()

    for _ in range(args.warmup):
        ctrl.tick(want_output=False)
    barrier()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window():
        """EXACTLY args.steps steps between two barriers (ctx stream drained + device synchronize + all ranks arrived)"""
        barrier()
        ev0.record(stream)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ctrl.tick(want_output=False)
        ev1.record(stream)
        ctrl.synchronize()  # the stream every launch of the window went to has drained: the K steps are done
        t1 = time.perf_counter()
        barrier()  # device synchronize + all ranks arrived (nothing left to wait for on this rank)
        return t1 - t0, ev0.elapsed_time(ev1) / args.steps  # wall; HIP events on the ctx stream

    # The timed region is exactly args.steps steps: one window, nothing repeated and no untimed ticks inside it. The
    # controller has then run exactly warmup + steps ticks, so --dump-outputs sees the same state from run to run.
    elapsed, step_ms_events = window()
    elapsed, step_ms_events = pkg.sharding.max_over_ranks([elapsed, step_ms_events], device=red_device)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, ctrl, rank, world)
    # per-kernel durations (outside the timed region): ONE event pair around back-to-back launches of the dominant
    # kernel alone, then around the tick's launch sequence (sai2b_profile_tick): the two parts add up to a step
    for attempt in range(3):
        kernel_ms, fallback_ms = ctrl.profile_tick(max(50, min(args.steps, 200)))
        kernel_ms, fallback_ms = pkg.sharding.max_over_ranks([kernel_ms, fallback_ms], device=red_device)
        consistent = kernel_ms + fallback_ms <= step_ms_events * 1.02 and kernel_ms <= step_ms_events
        if consistent:
            break
    pkg.sharding.barrier()

    if rank == 0:
        value = pkg.sharding.node_throughput(B, world, args.steps, elapsed)
        per_launch_bytes = BYTES_PER_TICK[args.config] * B
        achieved = per_launch_bytes / (kernel_ms * 1e-3) / 1e9
        out = {
            "metric": "control-ticks/sec (node), 65k batched 7-DOF Panda, 2-task hierarchy",
            "value": value,
            "unit": "control-ticks/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": {2: f"C2: {B} batched Panda, one 6-DOF MotionForceTask",
                             3: f"C3: {B} batched Panda per GPU, MotionForceTask(6) + nullspace JointTask",
                             4: f"C4: {B} batched Panda, partial MotionForceTask(3) + partial JointTask(2) + full JointTask, "
                                "singularity handling on (SVD-free kernel for general hierarchies + generic kernel over its work list)",
                             5: f"C5: {B} batched Panda per GPU (C3 workload sharded)"}[args.config]
                            + ", library defaults, OTG off (SURVEY.md §8(d))",
                "robots_per_gpu": B,
                "global_batch": B * world,
                "parallelism": f"batch-sharded x{world}, no collective",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": pmc_traffic_bytes(args.config) if B == (65536 if args.config in (3, 5) else pkg.workloads.CONFIG_BATCH[args.config]) else None,
                "kernel": {2: "sai2b::tick_fast_kernel<1>", 3: "sai2b::tick_fast_kernel<2>", 4: "sai2b::tick_cert_kernel<3>",
                           5: "sai2b::tick_fast_kernel<2>"}[args.config],
                "kernel_ms": kernel_ms,
                "fallback_kernel_ms": fallback_ms,
                "step_ms_hip_events": step_ms_events,
                "parts_sum_to_step": bool(consistent),
                "fp64_vector_frac": (FLOP_PER_TICK * B / (kernel_ms * 1e-3)) / (FP64_VECTOR_PEAK_TFLOPS * 1e12),
                "note": "achieved = algorithmic bytes/tick (SURVEY.md §8(d): 360/528/576 B for C2/C3/C4) x robots per launch / average launch duration of the "
                        "dominant kernel (one HIP event pair around back-to-back launches of it on the ctx stream); fallback_kernel_ms = what the "
                        "work-list pass behind it adds to a step; the path is FP64-VALU/latency bound, so the FP64 fraction (11.4 kflop/tick "
                        "formula-level figure) is reported beside the HBM fraction. traffic = 2*FETCH_SIZE + WRITE_SIZE "
                        "of the committed rocprofv3 --pmc passes of this command (profiles/), per launch. Measured FP64 FMA "
                        "issue ceilings (profiles/r01_fp64_fma_microbench.txt): 60 TF chip peak, 30 TF with one wavefront "
                        "per SIMD, which is what 65 536 robots at one lane per robot give",
            },
        }
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(inp)
        print(json.dumps(out), flush=True)
    pkg.sharding.finalize()


if __name__ == "__main__":
    main()
