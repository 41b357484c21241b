#!/usr/bin/env python3
"""Period (tick + sim_step(None), torques never leaving the device) of the headline hierarchy C3 with and without the actuator
and force-sensor models (sai2b_set_hardware), one process, one GPU: 65 536 Pandas, the contexts alive side by side, windows of
50 back-to-back periods alternating between them, HIP events on the context's stream around each window, the median of 40
windows of each (warm-up first; protocol of scripts/bench_external_wrench.py).
Contexts: a wrench with its sensor on the MotionForceTask and no hardware (twice: the spread of a context measured against
itself), the same with a delay only (D = 2, d cycling 0..2), and with everything on (delay, lag, gain, torque noise, sensor
bias, noise and filter) at D = 2 and D = 8.
Also printed: the bytes each of the two kernels moves per launch, from the row counts, and the time of a device-to-device
hipMemcpyAsync that moves as many (half read, half written; HIP events around 20 back-to-back copies, the median of 11),
the yardstick for the kernels' own times from a `rocprofv3 --kernel-trace --stats` run of this script.
Usage: python scripts/bench_hardware.py [--robots 65536] [--windows 40] [--periods 50]"""
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
    rng = np.random.default_rng(11)
    c.set_external_wrench(pkg.workloads.EE_LINK, rng.uniform(-30, 30, (3, B)), rng.uniform(-5, 5, (3, B)), point=(0.02, -0.01, 0.07), sensor_task=0)
    if depth is None:
        return c
    rng = np.random.default_rng(13)
    delay = np.arange(B) % (depth + 1)
    if everything:
        act, sen = c.hardware_rows(delay, rng.uniform(0.2, 0.9, (7, B)), rng.uniform(0.9, 1.1, (7, B)), rng.uniform(0.05, 0.5, (7, B)),
                                   rng.uniform(-2, 2, (6, B)), rng.uniform(0.01, 0.5, (6, B)), rng.uniform(0.2, 1.0, B))
        c.set_hardware(act, sen, max_delay=depth, sensor_task=0, seed=20261020)
    else:
        act, _ = c.hardware_rows(delay)
        c.set_hardware(act, None, max_delay=depth)
    return c


def window(c, periods):
    """device time of `periods` back-to-back periods, us per period"""
    s = torch.cuda.ExternalStream(c.stream())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(s)
    for _ in range(periods):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--periods", type=int, default=50)
    a = ap.parse_args()
    names = ["no hardware", "no hardware (again)", "delay only, D = 2", "everything, D = 2", "everything, D = 8"]
    ctx = [make(a.robots, d, e) for d, e in ((None, False), (None, False), (2, False), (2, True), (8, True))]
    for c in ctx:
        window(c, 3 * a.periods)
    t = [[] for _ in ctx]
    for _ in range(a.windows):
        for k, c in enumerate(ctx):
            t[k].append(window(c, a.periods))
    med = [statistics.median(v) for v in t]
    for k, name in enumerate(names):
        v = sorted(t[k])
        print(f"{name}: {med[k]:.2f} us per period (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), x{med[k] / med[0]:.3f} of "
              f"'{names[0]}'", flush=True)
    n, B = 7, a.robots
    # doubles read + written per robot, and the two clock ints (read, one written): everything on, a delay in force
    act = 8 * ((1 + 3 * n) + n + n + n + n + n + n) + 12
    sen = 8 * (13 + 6 + 6 + 6 + 6) + 8
    print(f"bytes per launch at {B} robots, everything on: actuate_kernel {act * B} ({act} per robot), sense_kernel {sen * B} ({sen} per robot)")
    for name, nbytes in (("actuate_kernel", act * B), ("sense_kernel", sen * B)):
        us = copy_us(nbytes)
        print(f"a device-to-device copy moving the bytes of {name} ({nbytes}): {us:.2f} us, {nbytes / us * 1e-6:.2f} TB/s")
    st = ctx[4].get_hardware_state()
    print(f"'{names[4]}': periods served {int(st['period'].min())}..{int(st['period'].max())}, largest |applied torque| {np.abs(st['applied_torque']).max():.1f} N m")


if __name__ == "__main__":
    main()
