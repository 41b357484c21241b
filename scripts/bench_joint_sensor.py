#!/usr/bin/env python3
"""Period (tick + sim_step(None), torques never leaving the device) of the headline hierarchy C3 with and without the joint
sensors (sai2b_set_joint_sensor), one process, one GPU: 65 536 Pandas, contexts built alike alive side by side, windows of 50
back-to-back periods alternating between them, HIP events on the context's stream around each window, the median of 40 windows
of each (warm-up first; protocol of scripts/bench_hardware.py).
Contexts: no joint sensor (twice: the spread of a context measured against itself), the ideal rows (D = 0: the stage copies
the truth), and everything on (delay cycling 0..D, offset, position noise, quantum, finite-difference velocity with noise and a
filter) at D = 2 and D = 8.
The stage's own time: windows of 50 back-to-back sim_step(None) alone, alternating between the context without the feature and
each context with it; the difference of the medians is joint_sense_kernel (the simulation kernel is the same launch in both).
Beside it: the bytes the kernel moves per launch, from the row counts, and the time of a device-to-device hipMemcpyAsync that
moves as many (half read, half written; HIP events around 20 back-to-back copies, the median of 11).
Usage: python scripts/bench_joint_sensor.py [--robots 65536] [--windows 40] [--periods 50]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402


def make(B, depth, everything):
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    if depth is None:
        return c
    if not everything:
        c.set_joint_sensor(max_delay=depth)
        return c
    rng = np.random.default_rng(13)
    rows = c.joint_sensor_rows(np.arange(B) % (depth + 1), rng.uniform(-0.01, 0.01, (7, B)), rng.uniform(1e-5, 1e-4, (7, B)), rng.uniform(1e-5, 1e-4, (7, B)),
                               rng.uniform(1e-3, 1e-2, (7, B)), rng.uniform(0.2, 0.9, (7, B)))
    c.set_joint_sensor(rows, max_delay=depth, velocity_mode="finite_difference", seed=20261020)
    return c


def window(c, periods, tick=True):
    """device time of `periods` back-to-back periods (or sim steps alone), us per period"""
    s = torch.cuda.ExternalStream(c.stream())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(s)
    for _ in range(periods):
        if tick:
            c.tick(want_output=False)
        c.sim_step(None, 0.001, 1)
    t1.record(s)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / periods


def copy_us(nbytes, device=0):
    """a device-to-device copy that reads nbytes / 2 and writes nbytes / 2, us per copy"""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=f"cuda:{device}")
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


def alternate(ctx, windows, periods, tick):
    for c in ctx:
        window(c, 3 * periods, tick)
    t = [[] for _ in ctx]
    for _ in range(windows):
        for k, c in enumerate(ctx):
            t[k].append(window(c, periods, tick))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--periods", type=int, default=50)
    a = ap.parse_args()
    names = ["no joint sensor", "no joint sensor (again)", "ideal rows, D = 0", "everything, D = 2", "everything, D = 8"]
    ctx = [make(a.robots, d, e) for d, e in ((None, False), (None, False), (0, False), (2, True), (8, True))]
    t = alternate(ctx, a.windows, a.periods, True)
    med = [statistics.median(v) for v in t]
    for k, name in enumerate(names):
        v = sorted(t[k])
        print(f"{name}: {med[k]:.2f} us per period (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), x{med[k] / med[0]:.3f} of "
              f"'{names[0]}'", flush=True)
    ts = alternate(ctx, a.windows, a.periods, False)
    meds = [statistics.median(v) for v in ts]
    n, B = 7, a.robots
    # doubles read + written per robot and the clock ints (two read, one written): rows, q, dq, pprev and v read, pprev and v
    # written, a history slot of 2 n written and (a delay in force) one read, the measured pair written
    moved = {"ideal rows, D = 0": 8 * ((1 + 5 * n) + 2 * n + 2 * n + 2 * n + 2 * n) + 12,
             "everything, D = 2": 8 * ((1 + 5 * n) + 2 * n + 2 * n + 2 * n + 2 * n + 2 * n + 2 * n) + 12}
    moved["everything, D = 8"] = moved["everything, D = 2"]
    for k in (2, 3, 4):
        own, per = meds[k] - meds[0], moved[names[k]]
        us = copy_us(per * B)
        print(f"{names[k]}: sim_step alone {meds[k]:.2f} us against {meds[0]:.2f} us without: joint_sense_kernel {own:.2f} us per launch; it moves "
              f"{per * B} bytes ({per} per robot), a device-to-device copy of as many takes {us:.2f} us ({per * B / us * 1e-6:.2f} TB/s): "
              f"x{own / us:.2f} of the copy", flush=True)
    print(f"'{names[1]}' sim_step alone: {meds[1]:.2f} us (the spread of the difference)")
    st = ctx[4].joint_sensor_state()
    qm, _ = ctx[4].get_measured_state()
    q, _ = ctx[4].get_state()
    print(f"'{names[4]}': readings taken {int(st['clock'].min())}..{int(st['clock'].max())}, largest |q_measured - q| {np.abs(qm - q).max():.4f} rad")


if __name__ == "__main__":
    main()
