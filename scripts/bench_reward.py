#!/usr/bin/env python3
"""Cost of the reward, one process, one GPU: 65 536 Pandas with the headline hierarchy (C3) and a sensed wrench, device tensors.
  (a) observe          pose + twist + error + sensed of the MotionForceTask with all criteria: one launch of observe_kernel
  (b) observe_reward   the same rows and criteria and every reward term on: one launch of observe_reward_kernel
  (c) observe + torch  (a) followed by the same reward and return update written in torch ops on the observation rows, the only
                       form there is without the feature. Terms the rows cannot express are left out and named in the output.
Time: HIP events on the context's stream around `calls` back-to-back calls, per call; the median of `windows` such windows
(10-90 % in brackets) after a warm-up, the three cases in turn in every window. For (c) the events are recorded on torch's
current stream, which the context's calls are ordered with (sai2b.h "stream contract").
  headline   bench.py's step time (ms_per_step of `python bench.py --gpus 1 --no-cpu-baseline`), `--bench-runs` runs of this
             tree alternated with as many of the tree given with --parent-root (a checkout of the commit before the feature,
             built); without --parent-root that side is reported as not measured.
Usage: python scripts/bench_reward.py [--robots 65536] [--windows 40] [--calls 50] [--bench-runs 3] [--parent-root DIR]"""
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

WEIGHT = dict(alive=0.25, joint_speed=-0.01, torque=-1e-4, torque_rate=-1e-3, limit=-3.0, done=1.0)
TASK_WEIGHT = dict(pos=-1.0, pos_sq=-2.0, pos_tanh=0.7, ori=-0.3, ori_sq=-0.4, ori_tanh=0.5, lin_vel_sq=-0.05, ang_vel_sq=-0.02,
                   force_err_sq=-0.003, force_excess=-0.1)
DONE_VALUE = dict(success=10.0, joint_limit=-5.0, speed=-2.5, nonfinite=-20.0, force=-7.0, timeout=0.125)
POS_SCALE, ORI_SCALE, FORCE_SOFT_LIMIT, SOFT_MARGIN, GAMMA = 0.1, 0.3, 7.0, 0.3, 0.99
# what (c) cannot form from the rows of (a): FORCE_ERR_SQ needs sigma_force and the goal force, TORQUE and TORQUE_RATE the stored
# torques, LIMIT the margin (three more global blocks through HBM would give the last three)
LEFT_OUT = ("force_err_sq", "torque", "torque_rate", "limit")


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
    rng = np.random.default_rng(2)
    c.set_mft_sensed_wrench(0, rng.normal(0, 5, (3, B)), rng.normal(0, 1, (3, B)))
    c.set_mft_goal_wrench(0, rng.normal(0, 4, (3, B)), rng.normal(0, 1, (3, B)))
    c.tick(want_output=False)
    c.sim_step()
    c.set_observation(tasks=[0], task_blocks=["pose", "twist", "error", "sensed"], success_tasks=[0], pos_tolerance=0.02, ori_tolerance=0.05,
                      joint_limit_margin=0.1, max_joint_speed=1.0, nonfinite=True, force_tasks=[0], max_sensed_force=8.0, max_episode_steps=1000)
    c.set_reward(terms=WEIGHT, tasks={0: dict(terms=TASK_WEIGHT, pos_scale=POS_SCALE, ori_scale=ORI_SCALE, force_soft_limit=FORCE_SOFT_LIMIT)},
                 done_value=DONE_VALUE, limit_soft_margin=SOFT_MARGIN, gamma=GAMMA)
    lay = c.observation_layout()
    rows = c.observation_rows()
    out = torch.zeros((rows, B), dtype=torch.float64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    reward = torch.zeros(B, dtype=torch.float64, device="cuda")
    ret, disc = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.ones(B, dtype=torch.float64, device="cuda")
    last_return = torch.zeros(B, dtype=torch.float64, device="cuda")
    done_value = torch.tensor([DONE_VALUE[k] for k in pkg._abi.DONE_BITS], dtype=torch.float64, device="cuda")
    bits = torch.tensor([1 << k for k in range(6)], dtype=torch.uint8, device="cuda")
    twist, error, sensed = lay["twist0"], lay["error0"], lay["sensed0"]
    w, tw = WEIGHT, TASK_WEIGHT

    def observe():
        c.observe(out=out, done=done)

    def observe_reward():
        c.observe_reward(out=out, done=done, reward=reward, terms=False)

    def observe_torch():
        nonlocal ret, disc, last_return
        c.observe(out=out, done=done)
        dp, do = out[error.start + 6], out[error.start + 7]
        v = out[twist]
        fn = torch.linalg.vector_norm(out[sensed.start:sensed.start + 3], dim=0)
        dv = ((done[None, :] & bits[:, None]) != 0).to(torch.float64)
        r = w["alive"] + w["done"] * (done_value[:, None] * dv).sum(dim=0)
        r = r + tw["pos"] * dp + tw["pos_sq"] * dp * dp + tw["pos_tanh"] * (1 - torch.tanh(dp / POS_SCALE))
        r = r + tw["ori"] * do + tw["ori_sq"] * do * do + tw["ori_tanh"] * (1 - torch.tanh(do / ORI_SCALE))
        r = r + tw["lin_vel_sq"] * (v[:3] * v[:3]).sum(dim=0) + tw["ang_vel_sq"] * (v[3:] * v[3:]).sum(dim=0)
        r = r + tw["force_excess"] * torch.clamp(fn - FORCE_SOFT_LIMIT, min=0.0)
        r = torch.where(torch.isfinite(r), r, torch.zeros_like(r))
        ret = ret + disc * r
        disc = disc * GAMMA
        closed = done != 0
        last_return = torch.where(closed, ret, last_return)
        ret = torch.where(closed, torch.zeros_like(ret), ret)
        disc = torch.where(closed, torch.ones_like(disc), disc)

    def time(fn, calls):
        """us per call: events on torch's current stream, which every call of the context is ordered with"""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / calls

    cases = {"(a) observe": observe, "(b) observe_reward": observe_reward, "(c) observe + the reward in torch ops": observe_torch}
    for fn in cases.values():
        time(fn, 3 * a.calls)
    t = {n: [] for n in cases}
    for _ in range(a.windows):  # the cases in turn, so that drift of the clocks falls on all alike
        for n, fn in cases.items():
            t[n].append(time(fn, a.calls))
    print(f"{B} robots, {rows} observation rows, all criteria; reward: {c.reward_rows()} terms", flush=True)
    print("(c) leaves out: " + ", ".join(LEFT_OUT) + " (not in the observation rows of (a))", flush=True)
    base = statistics.median(t["(a) observe"])
    for n in cases:
        v = sorted(t[n])
        m = statistics.median(v)
        print(f"{n}: {m:.2f} us per call (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), {m / base:.4f} of (a)", flush=True)
    c.tick(want_output=False)  # the context still works
    c.synchronize()
    c.close()
    del c
    torch.cuda.synchronize()

    ours, parent = [], []
    for k in range(a.bench_runs):  # alternated: what else runs on the box falls on both alike
        ours.append(headline(ROOT, a.bench_steps, 200))
        if a.parent_root:
            parent.append(headline(a.parent_root, a.bench_steps, 200))
    if ours:
        print(f"headline step (bench.py --gpus 1 --steps {a.bench_steps}), this tree: " + ", ".join(f"{x:.4f}" for x in ours) + " ms", flush=True)
        print("headline step, parent commit: " + (", ".join(f"{x:.4f}" for x in parent) + " ms" if parent else "not measured"), flush=True)


if __name__ == "__main__":
    main()
