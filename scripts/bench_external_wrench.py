#!/usr/bin/env python3
"""Period (tick + sim_step(None), torques never leaving the device) of the headline hierarchy C3 with and without an external
wrench on every robot of the simulated plant, and the same with joint dynamics on, one process, one GPU: 65 536 Pandas, the
contexts alive side by side, windows of 50 back-to-back periods alternating between them, HIP events on the context's
stream around each window, the median of 40 windows of each (warm-up first; protocol of scripts/bench_joint_dynamics.py).
Contexts: no wrench (twice: the spread of a context measured against itself), a wrench on the end-effector link of every
robot (world frame, |F_i| <= 30 N, |M_i| <= 5 N m, pushed until changed, sensor on the MotionForceTask), joint dynamics as
scripts/bench_joint_dynamics.py sets them, and joint dynamics with the same wrench.
Usage: python scripts/bench_external_wrench.py [--robots 65536] [--windows 40] [--periods 50]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402


def make(B, wrench, joint_dynamics):
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    rng = np.random.default_rng(7)
    if joint_dynamics:
        c.set_joint_dynamics(armature=rng.uniform(0, 0.2, (7, B)), damping=rng.uniform(0, 5, (7, B)), friction=rng.uniform(0, 2, (7, B)),
                             torque_limit="model", limits="model", stop_stiffness=1e4, stop_damping=0.5, friction_velocity_eps=1e-3)
    if wrench:
        rng = np.random.default_rng(11)
        c.set_external_wrench(pkg.workloads.EE_LINK, rng.uniform(-30, 30, (3, B)), rng.uniform(-5, 5, (3, B)), point=(0.02, -0.01, 0.07),
                              sensor_task=0)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--periods", type=int, default=50)
    a = ap.parse_args()
    names = ["no wrench", "no wrench (again)", "wrench", "joint dynamics", "joint dynamics + wrench"]
    base = [0, 0, 0, 3, 3]  # the context each ratio is taken against
    ctx = [make(a.robots, w, j) for w, j in ((False, False), (False, False), (True, False), (False, True), (True, True))]
    for c in ctx:
        window(c, 3 * a.periods)
    t = [[] for _ in ctx]
    for _ in range(a.windows):
        for k, c in enumerate(ctx):
            t[k].append(window(c, a.periods))
    med = [statistics.median(v) for v in t]
    for k, name in enumerate(names):
        v = sorted(t[k])
        print(f"{name}: {med[k]:.2f} us per period (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), x{med[k] / med[base[k]]:.3f} of "
              f"'{names[base[k]]}'", flush=True)
    for k in (2, 4):
        print(f"{names[k]}: robots pushed in the last step: {ctx[k].robots_pushed()} of {a.robots}")


if __name__ == "__main__":
    main()
