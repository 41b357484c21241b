#!/usr/bin/env python3
"""sai2b_collision_query and sai2b_end_episodes on 65 536 Pandas, one process, one GPU, profiler off.
Configuration: 12 spheres (one per link and five more on alternate links), 1 plane, 2 obstacles, the default pairs.
collision_query with device tensors: distances only; distances + normals + gradients; every block. Windows of 50 back-to-back
calls, HIP events on the context's stream around each window, the variants alternating, the median of 40 windows of each.
end_episodes with device tensors at an empty, a 1 % and a full `extra`, measured the same way (an observation and a reward are
configured, so a closed episode writes its accumulators).
Beside each: the bytes the call moves and its floating-point operations, COUNTED FROM THE SHAPES by the code below, and the time
of a device-to-device copy that moves as many bytes (half read, half written; HIP events around 20 back-to-back copies, the median
of 11): the share of the HBM bound the kernel reaches is copy / kernel.
Usage: python scripts/bench_collision.py [--robots 65536] [--windows 40] [--calls 50]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402

N, SPHERES, PLANES, OBSTACLES = 7, 12, 1, 2
LINKS = list(range(7)) + [0, 2, 4, 6, 1]
VARIANTS = {"distances": ("distance",), "distances + normals + gradients": ("distance", "normal", "gradient"),
            "every block": ("distance", "index", "normal", "gradient", "centres")}
ROWS = dict(distance=3, index=3, normal=9, gradient=3 * N, centres=3 * SPHERES)


def make(B, blocks):
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    rng = np.random.default_rng(17)
    centres = rng.uniform(-0.05, 0.05, (SPHERES, 3))
    centres[7:, 2] += 0.1
    cfg = c.collision_config(LINKS, centres, rng.uniform(0.03, 0.07, SPHERES), n_planes=PLANES, n_obstacles=OBSTACLES, blocks=blocks,
                             margin_plane=0.05, margin_obstacle=0.05, margin_self=0.0)
    nrm = np.array([0.0, 0.0, 1.0])
    c.set_collision(cfg, c.collision_env_rows(cfg, planes=[((0, 0, 0), nrm)],
                                              obstacles=[(rng.uniform(-0.8, 0.8, (3, B)), rng.uniform(0.05, 0.15, B)) for _ in range(OBSTACLES)]))
    return c, cfg


def pairs_tested(cfg):
    return sum(bin(cfg.pair_mask[i]).count("1") for i in range(16))


def counted(cfg, blocks):
    """(bytes, flops) of one collision_query per robot, from the shapes. Bytes: q read, the environment rows read, the selected
    rows and the flags byte written. Flops (+, -, *, each 1; sqrt, divide, sin, cos each 1): the chain 7 x (R E: 45, p: 18, the turn:
    2 + 12), a centre 18 per sphere, a plane candidate 9, an obstacle candidate 11, a pair 11, a witness normal 9, a gradient 7 x 20
    per point (two points for self)."""
    env = bin(cfg.env_mask).count("1")
    out_rows = sum(ROWS[b] for b in blocks)
    nbytes = 8 * (N + 6 * PLANES + 4 * OBSTACLES + out_rows) + 1
    flops = N * (45 + 18 + 14) + 18 * SPHERES + 9 * PLANES * env + 11 * OBSTACLES * env + 11 * pairs_tested(cfg)
    if "normal" in blocks or "gradient" in blocks:
        flops += 2 * 9
    if "gradient" in blocks:
        flops += 4 * N * 20
    return nbytes, flops


def window(c, calls, fn):
    s = torch.cuda.ExternalStream(c.stream())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(s)
    for _ in range(calls):
        fn()
    t1.record(s)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def alternate(ctx, fns, windows, calls):
    for c, f in zip(ctx, fns):
        window(c, 3 * calls, f)
    t = [[] for _ in ctx]
    for _ in range(windows):
        for k, (c, f) in enumerate(zip(ctx, fns)):
            t[k].append(window(c, calls, f))
    return t


def copy_us(nbytes, device=0):
    """a device-to-device copy that reads nbytes / 2 and writes nbytes / 2, us per copy"""
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=f"cuda:{device}")
    dst = torch.empty_like(src)
    dst.copy_(src)
    t = []
    for _ in range(11):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            dst.copy_(src, non_blocking=True)
        t1.record()
        t1.synchronize()
        t.append(t0.elapsed_time(t1) * 1e3 / 20)
    return statistics.median(t)


def spread(v):
    v = sorted(v)
    return f"10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    B = a.robots
    ctx, cfgs, fns = [], [], []
    for name, blocks in VARIANTS.items():
        c, cfg = make(B, blocks)
        out = torch.zeros((c.collision_rows(), B), dtype=torch.float64, device="cuda")
        flags = torch.zeros(B, dtype=torch.uint8, device="cuda")
        ctx.append(c), cfgs.append(cfg), fns.append(lambda c=c, out=out, flags=flags: c.collision_query(out, flags))
    print(f"{B} Pandas, {SPHERES} spheres, {PLANES} plane, {OBSTACLES} obstacles, {pairs_tested(cfgs[0])} pairs tested (the default mask)")
    t = alternate(ctx, fns, a.windows, a.calls)
    for k, (name, blocks) in enumerate(VARIANTS.items()):
        med = statistics.median(t[k])
        per, flops = counted(cfgs[k], blocks)
        us = copy_us(per * B)
        print(f"collision_query, {name}: {med:.2f} us per call ({spread(t[k])}); counted {per} bytes and {flops} flops per robot = {per * B} bytes, "
              f"{flops * B / med * 1e-6:.3f} TFLOP/s FP64; a device-to-device copy of as many bytes takes {us:.2f} us ({per * B / us * 1e-6:.2f} TB/s): the "
              f"kernel reaches {100 * us / med:.1f} % of the HBM bound", flush=True)
    print("flag counts of the last query:", ctx[2].collision_counts())
    # ---- end_episodes: done byte and extra byte read per robot; a selected robot writes its byte, a closed one moves ret, disc,
    # last_return (3 doubles read or written, 1 more written), two ints written, the counter read and written
    c = ctx[0]
    c.set_observation(blocks=("episode_step",), max_episode_steps=1000000)
    c.set_reward(terms=dict(alive=1.0))
    c.observe_reward(out=False, done=False, reward=False, terms=False)
    extras = {"empty": torch.zeros(B, dtype=torch.uint8, device="cuda"), "1 %": (torch.rand(B, device="cuda") < 0.01).to(torch.uint8),
              "full": torch.ones(B, dtype=torch.uint8, device="cuda")}
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")

    def call(extra):
        done.zero_()  # (on torch's stream, ordered by the stream contract) every selected robot is closed in every call
        c.end_episodes(done, extra)

    names = list(extras)
    t = alternate([c] * 3, [lambda e=extras[k]: call(e) for k in names], a.windows, a.calls)
    for k, name in enumerate(names):
        sel = int(extras[name].sum().item())
        moved = B * 1 + (B if sel else 0) + sel * (1 + 8 * 5 + 4 * 4)
        med = statistics.median(t[k])
        us = copy_us(moved)
        print(f"end_episodes, {name} extra ({sel} robots closed): {med:.2f} us per call, the zeroing of the done bytes on the caller's stream and the "
              f"hand-over between the streams included ({spread(t[k])}); counted {moved} bytes; a device-to-device copy of as many takes {us:.2f} us",
              flush=True)
    print("closed by the last call:", c.end_episode_count())


if __name__ == "__main__":
    main()
