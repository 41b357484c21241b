#!/usr/bin/env python3
"""Cost of an episode reset with its start state and goals drawn on the device, one process, one GPU: 65 536 Pandas with the
headline hierarchy (C3), everything device-resident, masks selecting 0 %, 1 % (scattered) and 100 % of the robots.
  reset_robots          reset_robots(mask, q, dq): the state given (scripts/bench_reset.py's rows, measured again in this session)
  parent form           what the library offered before the sampler: q drawn with torch ops, no criterion, reset_robots, observe
                        for the new pose, goals built in torch, the whole-batch goal setters (which have no mask: the caller
                        keeps the other robots' goals and merges)
  sampled               reset_robots_sampled(mask) with goals for both tasks: no criterion; the ratio criterion at 0.06 with 8
                        tries; at 0.1 with 32 tries
Time: HIP events on the context's stream around `calls` back-to-back calls, per call; the median of `windows` such windows
(10-90 % in brackets) after a warm-up, the cases taken in turn within every window.
Usage: python scripts/bench_reset_sampler.py [--robots 65536] [--windows 30] [--calls 20]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sai2_primitives_perso_amd as pkg  # noqa: E402
from bench_reset import Events  # noqa: E402

GOALS = {0: dict(pos_lower=(-0.1, -0.1, -0.05), pos_upper=(0.1, 0.1, 0.15), theta_max=0.5), 1: dict(half_width=0.2)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    B = a.robots
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)

    def controller(**criterion):
        c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
        pkg.workloads.load_inputs(c, inp)
        c.tick(want_output=False)
        c.sim_step()
        cfg = c.reset_sampler_config(seed=7, goal_tasks=(0, 1), **criterion)
        c.set_reset_sampler(cfg, torch.from_numpy(c.reset_sampler_rows(cfg, dq_sigma=0.1, goals=GOALS)).cuda())
        return c

    c = controller()
    crit = {"ratio >= 0.06, 8 tries": controller(ratio_task=0, min_ratio=0.06, max_tries=8),
            "ratio >= 0.1, 32 tries": controller(ratio_task=0, min_ratio=0.1, max_tries=32)}
    q, dq = (torch.from_numpy(inp[k]).cuda() for k in ("q", "dq"))
    rng = np.random.default_rng(3)
    masks = {"0 %": np.zeros(B, dtype=bool), "1 % scattered": np.zeros(B, dtype=bool), "100 %": np.ones(B, dtype=bool)}
    masks["1 % scattered"][rng.choice(B, size=max(1, B // 100), replace=False)] = True
    dev = {k: torch.from_numpy(m).cuda() for k, m in masks.items()}

    # the parent form's own bookkeeping
    lo = torch.from_numpy(0.5 * (pkg.workloads.PANDA_LOWER + pkg.workloads.PANDA_UPPER) - 0.4 * (pkg.workloads.PANDA_UPPER - pkg.workloads.PANDA_LOWER)).cuda()[:, None]
    width = torch.from_numpy(0.8 * (pkg.workloads.PANDA_UPPER - pkg.workloads.PANDA_LOWER)).cuda()[:, None]
    c.set_observation(tasks=(0,), task_blocks=("pose",))
    pose = torch.zeros((c.observation_rows(), B), dtype=torch.float64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    g = c.get_mft_goals(0)
    goal_pos, goal_rot = torch.from_numpy(g[0]).cuda(), torch.from_numpy(g[1]).cuda()
    goal_q = torch.from_numpy(c.get_jt_goals(1)[0]).cuda()
    zero = torch.zeros((7, B), dtype=torch.float64, device="cuda")
    p_lo = torch.tensor(GOALS[0]["pos_lower"], dtype=torch.float64, device="cuda")[:, None]
    p_w = torch.tensor(GOALS[0]["pos_upper"], dtype=torch.float64, device="cuda")[:, None] - p_lo
    torch.cuda.synchronize()

    def parent(m):
        qn = lo + width * torch.rand((7, B), dtype=torch.float64, device="cuda")
        c.reset_robots(m, qn, zero)
        c.observe(pose, done)
        sel = m[None, :]
        goal_pos.copy_(torch.where(sel, pose[0:3] + p_lo + p_w * torch.rand((3, B), dtype=torch.float64, device="cuda"), goal_pos))
        goal_rot.copy_(torch.where(sel, pose[3:12], goal_rot))
        goal_q.copy_(torch.where(sel, qn + 0.2 * (2 * torch.rand((7, B), dtype=torch.float64, device="cuda") - 1), goal_q))
        c.set_mft_goals(0, goal_pos, goal_rot)
        c.set_jt_goals(1, goal_q)

    cases = []
    for k in masks:
        n = int(masks[k].sum())
        cases.append((f"reset_robots, {k} ({n} robots)", lambda m=dev[k]: c.reset_robots(m, q, dq), None))
        cases.append((f"parent form (torch draws, reset_robots, observe, goal setters), {k}", lambda m=dev[k]: parent(m), None))
        cases.append((f"reset_robots_sampled, no criterion, {k}", lambda m=dev[k]: c.reset_robots_sampled(m), c))
        if n:
            for name, cc in crit.items():
                cases.append((f"reset_robots_sampled, {name}, {k}", lambda m=dev[k], cc=cc: cc.reset_robots_sampled(m), cc))
    evs = {id(x): Events(x) for x in [c] + list(crit.values())}
    ev_of = lambda ctx: evs[id(ctx if ctx is not None else c)]
    for _, fn, ctx in cases:
        ev_of(ctx).time(fn, 2 * a.calls)
    t = {name: [] for name, _, _ in cases}
    for _ in range(a.windows):  # the cases in turn, so that drift of the clocks falls on all alike
        for name, fn, ctx in cases:
            t[name].append(ev_of(ctx).time(fn, a.calls))
    for name, _, ctx in cases:
        v = sorted(t[name])
        m = statistics.median(v)
        extra = ""
        if ctx is not None and not name.endswith(", 0 %"):
            k = ctx.reset_sampler_counts()
            extra = f"; last call: {k['reset']} reset, {k['rejected']} candidates rejected, {k['exhausted']} exhausted"
        print(f"{name}: {m:.2f} us per call (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}){extra}", flush=True)
    for x in [c] + list(crit.values()):
        x.tick(want_output=False)  # the contexts still work
        x.synchronize()
        x.close()


if __name__ == "__main__":
    main()
