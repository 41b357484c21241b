#!/usr/bin/env python3
"""Cost of mapping a policy's action to goals, one process, one GPU: 65 536 Pandas with the headline hierarchy (C3), the
action in a device tensor (nothing leaves the GPU).
  apply_action  one launch of action_kernel, for three configurations:
                A  DELTA_GOAL position + orientation of the MotionForceTask
                B  DELTA_CURRENT position + orientation + the joints of the JointTask (forward kinematics in the kernel)
                C  DELTA_GOAL, all four blocks, with a box and a lead (forward kinematics for the lead), and the joints
                and C without the lead (C'), which the torch form below can express
  torch form    what a user of the commit before the feature writes: the goal kept in torch tensors, the same mapping in
                torch ops (clamp, scale, add, Rodrigues' formula, a batched 3 x 3 product, box clamp), then sai2b_set_mft_goals /
                sai2b_set_mft_goal_wrench / sai2b_set_jt_goals with device pointers. Only possible where no current pose is
                needed: before this feature the pose of the robot as it is now exists on the device only through sai2b_observe,
                so B and C have no such form; A and C' do.
Time: HIP events on the context's stream around `calls` back-to-back calls, per call; the median of `windows` such windows
(10-90 % in brackets) after a warm-up, the cases in turn. The goal setters order the context's stream behind torch's, so the
interval covers the torch ops of the calls in between.
  headline      bench.py's step time (ms_per_step of `python bench.py --gpus 1 --no-cpu-baseline`), `--bench-runs` runs of this
                tree alternated with as many of the tree given with --parent-root (a checkout of the commit before the feature,
                built); without --parent-root that side is reported as not measured.
Usage: python scripts/bench_action.py [--robots 65536] [--windows 40] [--calls 50] [--bench-runs 3] [--parent-root DIR]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sai2_primitives_perso_amd as pkg  # noqa: E402
from bench_observe import headline  # noqa: E402
from bench_reset import Events  # noqa: E402

POS_SCALE, ORI_SCALE, FORCE_SCALE, MOMENT_SCALE, JT_SCALE = 0.02, 0.05, 10.0, 1.0, 0.05
BOX = dict(pos_lower=(-0.8, -0.8, 0.05), pos_upper=(0.8, 0.8, 1.2))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    B = a.robots
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    c.tick(want_output=False)
    mft = dict(pos_scale=POS_SCALE, ori_scale=ORI_SCALE, force_scale=FORCE_SCALE, moment_scale=MOMENT_SCALE)
    all_blocks = ("position", "orientation", "force", "moment")
    configs = {
        "A DELTA_GOAL position + orientation": dict(tasks={0: dict(mode="delta_goal", blocks=all_blocks[:2], **mft)}, clip_actions=True),
        "B DELTA_CURRENT position + orientation + joints": dict(tasks={0: dict(mode="delta_current", blocks=all_blocks[:2], **mft),
                                                                       1: dict(mode="delta_current", jt_scale=JT_SCALE, jt_limits="model")}, clip_actions=True),
        "C all blocks, box and lead, joints": dict(tasks={0: dict(mode="delta_goal", blocks=all_blocks, max_pos_lead=0.05, **BOX, **mft),
                                                          1: dict(mode="delta_goal", jt_scale=JT_SCALE, jt_limits="model")}, clip_actions=True),
        "C' all blocks, box, joints (no lead)": dict(tasks={0: dict(mode="delta_goal", blocks=all_blocks, **BOX, **mft),
                                                            1: dict(mode="delta_goal", jt_scale=JT_SCALE, jt_limits="model")}, clip_actions=True),
    }
    cfgs = {n: c.action_config(**kw) for n, kw in configs.items()}
    gen = torch.Generator(device="cuda").manual_seed(3)
    actions = {}
    for n in cfgs:
        c.set_action(cfgs[n])
        actions[n] = (torch.rand((c.action_rows(), B), dtype=torch.float64, device="cuda", generator=gen) * 2.4 - 1.2).contiguous()

    # the torch form: the goal lives in torch tensors
    pos_g = torch.from_numpy(inp["mft0"]["pos"]).cuda()
    rot_g = torch.from_numpy(inp["mft0"]["rot"]).cuda()
    q_g = torch.from_numpy(inp["jt1"]["q"]).cuda()
    lo = torch.tensor(BOX["pos_lower"], dtype=torch.float64, device="cuda")[:, None]
    hi = torch.tensor(BOX["pos_upper"], dtype=torch.float64, device="cuda")[:, None]
    q_lo = torch.tensor(list(c.model.q_lower)[:7], dtype=torch.float64, device="cuda")[:, None]
    q_hi = torch.tensor(list(c.model.q_upper)[:7], dtype=torch.float64, device="cuda")[:, None]

    def rotate(rot, w):
        """exp([w]x) rot for rot [9][B] row-major, w [3][B]: Rodrigues' formula with the series below th2 = 1e-8"""
        th2 = (w * w).sum(dim=0)
        th = torch.sqrt(th2)
        small = th2 < 1e-8
        safe = torch.where(small, torch.ones_like(th), th)
        ca = torch.where(small, 1.0 - th2 / 6.0, torch.sin(safe) / safe)
        cb = torch.where(small, 0.5 - th2 / 24.0, 2.0 * torch.sin(0.5 * safe) ** 2 / (safe * safe))
        W = torch.zeros((B, 3, 3), dtype=torch.float64, device="cuda")
        W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
        R = rot.t().reshape(B, 3, 3)
        D = ca[:, None, None] * W + cb[:, None, None] * (W @ W)
        return (R + D @ R).reshape(B, 9).t().contiguous()

    def torch_a():
        nonlocal pos_g, rot_g
        act = actions["A DELTA_GOAL position + orientation"].clamp(-1.0, 1.0)
        pos_g = pos_g + POS_SCALE * act[0:3]
        rot_g = rotate(rot_g, ORI_SCALE * act[3:6])
        c.set_mft_goals(0, pos_g, rot_g)

    def torch_c():
        nonlocal pos_g, rot_g, q_g
        act = actions["C' all blocks, box, joints (no lead)"].clamp(-1.0, 1.0)
        pos_g = torch.minimum(torch.maximum(pos_g + POS_SCALE * act[0:3], lo), hi)
        rot_g = rotate(rot_g, ORI_SCALE * act[3:6])
        f, m = (FORCE_SCALE * act[6:9]).contiguous(), (MOMENT_SCALE * act[9:12]).contiguous()
        q_g = torch.minimum(torch.maximum(q_g + JT_SCALE * act[12:19], q_lo), q_hi)
        c.set_mft_goals(0, pos_g, rot_g)
        c.set_mft_goal_wrench(0, f, m)
        c.set_jt_goals(1, q_g)

    def ours(n):
        return lambda: c.apply_action(actions[n])

    cases = {}
    for n in cfgs:
        cases[f"apply_action, {n} ({actions[n].shape[0]} rows)"] = (n, ours(n))
    cases["torch form of A (torch ops + sai2b_set_mft_goals, device pointers)"] = (None, torch_a)
    cases["torch form of C' (torch ops + three goal setters, device pointers)"] = (None, torch_c)
    ev = Events(c)
    t = {k: [] for k in cases}
    for k, (n, fn) in cases.items():  # warm-up of every shape
        if n:
            c.set_action(cfgs[n])
        ev.time(fn, a.calls)
    for _ in range(a.windows):  # the cases in turn, so that drift of the clocks falls on all alike
        for k, (n, fn) in cases.items():
            if n:
                c.set_action(cfgs[n])
            t[k].append(ev.time(fn, a.calls))
    med = {}
    for k in cases:
        v = sorted(t[k])
        med[k] = statistics.median(v)
        print(f"{k}: {med[k]:.2f} us per call (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f})", flush=True)
    keys = list(cases)
    print(f"apply_action A / torch form of A: {med[keys[0]] / med[keys[4]]:.4f}", flush=True)
    print(f"apply_action C' / torch form of C': {med[keys[3]] / med[keys[5]]:.4f}", flush=True)
    print("B and C have no torch form on the commit before the feature: the current pose is not available on the device there", flush=True)
    c.tick(want_output=False)  # the context still works
    c.synchronize()
    c.close()
    del c
    torch.cuda.synchronize()

    ours_ms, parent_ms = [], []
    for k in range(a.bench_runs):  # alternated: what else runs on the box falls on both alike
        ours_ms.append(headline(ROOT, a.bench_steps, 200))
        if a.parent_root:
            parent_ms.append(headline(a.parent_root, a.bench_steps, 200))
    if ours_ms:
        print(f"headline step (bench.py --gpus 1 --steps {a.bench_steps}), this tree: " + ", ".join(f"{x:.4f}" for x in ours_ms) + " ms", flush=True)
        print("headline step, parent commit: " + (", ".join(f"{x:.4f}" for x in parent_ms) + " ms" if parent_ms else "not measured"), flush=True)


if __name__ == "__main__":
    main()
