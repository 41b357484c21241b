#!/usr/bin/env python3
"""Period (tick + sim_step(None) with three substeps, torques never leaving the device) of the headline hierarchy C3 with and
without whole-arm contact in the simulated plant, one process, one GPU: 65 536 Pandas, 12 spheres, 1 plane, 2 obstacles, the
default pairs; the contexts alive side by side, windows of back-to-back periods alternating between them, HIP events on the
context's stream around each window, the median of the windows of each (warm-up first; protocol of
scripts/bench_external_wrench.py). Contexts: no body contact (twice: the spread of a context measured against itself), body contact
with nobody touching (every plane and obstacle 2 m away; the spheres are laid out so that the closest default pair, on the
Panda's links 4 and 6, keeps 48 mm of clearance in every posture), body contact with a quarter of the robots touching (every
fourth robot's plane 5 mm into its lowest sphere at the start), and the same three with joint dynamics and an external wrench
on. How many robots touch at the end is printed with every context.
Two yardsticks beside them, references and not pass marks: the simulation kernel alone (windows of sim_step(None) without the
tick) of the context without body contact, which is the kernel a context without the feature always ran, and of the one with
it; and substeps x one collision_query that stores the distances alone.
Usage: python scripts/bench_body_contact.py [--robots 65536] [--windows 30] [--periods 40]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402

SUBSTEPS = 3
# 12 spheres of 20 mm: one at every link's origin and five more on alternate links (the one of link 4 mid-forearm, 0.15 m back
# from the wrist: 0.1 m forward it would sit on link 6's); the default pairs (links at least 2 apart). Over the workload's
# postures the closest pair is the origins of links 4 and 6, 88 mm apart whatever the posture
LINKS = [0, 1, 2, 3, 4, 5, 6, 0, 2, 4, 6, 1]
CENTRES = [[0, 0, 0]] * 7 + [[0, 0, -0.1], [0, 0, -0.1], [0, 0, -0.15], [0, 0, 0.1], [0, 0.1, 0]]
RADIUS = 0.02


def make(B, body, touching, hard):
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    rng = np.random.default_rng(7)
    if hard:
        c.set_joint_dynamics(armature=rng.uniform(0, 0.2, (7, B)), damping=rng.uniform(0, 5, (7, B)), friction=rng.uniform(0, 2, (7, B)),
                             torque_limit="model", limits="model", stop_stiffness=1e4, stop_damping=0.5, friction_velocity_eps=1e-3)
        c.set_external_wrench(pkg.workloads.EE_LINK, rng.uniform(-30, 30, (3, B)), rng.uniform(-5, 5, (3, B)), point=(0.02, -0.01, 0.07))
    cfg = c.collision_config(LINKS, CENTRES, RADIUS, n_planes=1, n_obstacles=2, blocks=("distance", "centres"))
    env = c.collision_env_rows(cfg, planes=[([0, 0, -2.0], [0, 0, 1.0])], obstacles=[([2.0, 0, 0], 0.05), ([0, 2.0, 0], 0.05)])
    c.set_collision(cfg, env)
    if touching:  # every fourth robot's floor comes up 5 mm into its lowest sphere
        out, _ = c.collision_query()
        z = out[3:].reshape(12, 3, B)[:, 2, :]
        env[2, ::4] = (z.min(axis=0) - RADIUS + 5e-3)[::4]
    c.set_collision(c.collision_config(LINKS, CENTRES, RADIUS, n_planes=1, n_obstacles=2), env)
    if body:
        c.set_body_contact(2e4, 0.2, 0.5)
    return c


def window(c, periods, tick=True):
    """device time of `periods` back-to-back periods, us per period"""
    s = torch.cuda.ExternalStream(c.stream())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(s)
    for _ in range(periods):
        if tick:
            c.tick(want_output=False)
        c.sim_step(None, 0.001, SUBSTEPS)
    t1.record(s)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / periods


def query_window(c, out, flags, periods):
    s = torch.cuda.ExternalStream(c.stream())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        t0.record(s)
        for _ in range(periods):
            c.collision_query(out, flags)
        t1.record(s)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / periods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--periods", type=int, default=40)
    a = ap.parse_args()
    B = a.robots
    names = ["no body contact", "no body contact (again)", "body contact, nobody touching", "body contact, a quarter touching",
             "joint dynamics + wrench", "joint dynamics + wrench + body contact, nobody touching",
             "joint dynamics + wrench + body contact, a quarter touching"]
    base = [0, 0, 0, 0, 4, 4, 4]
    spec = [(False, False, False), (False, False, False), (True, False, False), (True, True, False), (False, False, True), (True, False, True),
            (True, True, True)]
    ctx = [make(B, *s) for s in spec]
    for c in ctx:
        window(c, 2 * a.periods)
    t = [[] for _ in ctx]
    for _ in range(a.windows):
        for k, c in enumerate(ctx):
            t[k].append(window(c, a.periods))
    med = [statistics.median(v) for v in t]
    for k, name in enumerate(names):
        v = sorted(t[k])
        touch = f", {ctx[k].robots_touching()} of {B} touching at the end" if spec[k][0] else ""
        print(f"{name}: {med[k]:.2f} us per period (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), x{med[k] / med[base[k]]:.3f} of "
              f"'{names[base[k]]}', +{med[k] - med[base[k]]:.2f} us{touch}", flush=True)
    # the yardsticks: the simulation kernel alone, and substeps x one query storing the distances alone
    alone = {}
    for k in (0, 2, 3, 4, 5):
        v = []
        for _ in range(a.windows):
            v.append(window(ctx[k], a.periods, tick=False))
        alone[k] = statistics.median(v)
        print(f"simulation kernel alone, {names[k]}: {alone[k]:.2f} us per sim_step of {SUBSTEPS} substeps", flush=True)
    out = torch.zeros((ctx[0].collision_rows(), B), dtype=torch.float64, device="cuda")
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda")
    query_window(ctx[0], out, flags, a.periods)
    q = statistics.median(query_window(ctx[0], out, flags, a.periods) for _ in range(a.windows))
    print(f"one collision_query storing the distances alone: {q:.2f} us; {SUBSTEPS} of them: {SUBSTEPS * q:.2f} us")
    print(f"body contact costs {alone[2] - alone[0]:.2f} us per sim_step with nobody touching, {alone[3] - alone[0]:.2f} us with a quarter touching; "
          f"the step plus {SUBSTEPS} queries would be {alone[0] + SUBSTEPS * q:.2f} us, the kernel takes {alone[3]:.2f} us")


if __name__ == "__main__":
    main()
