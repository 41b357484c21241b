#!/usr/bin/env python3
"""Cost of an observation, one process, one GPU: 65 536 Pandas with the headline hierarchy (C3).
  observe    one launch of observe_kernel into device tensors (nothing leaves the GPU), for four selections:
             pose + twist + error of the MotionForceTask; every block of the feature; the done byte alone (all criteria on); both
  getters    what the first selection costs without the feature, same build, same box: get_mft_status + get_mft_velocity +
             get_state into host arrays (a kernel, a wait and device-to-host copies each)
Time: HIP events on the context's stream around `calls` back-to-back calls, per call; the median of `windows` such windows
(10-90 % in brackets) after a warm-up, the cases in turn. The interval covers whatever is slower, the host's enqueueing or
the device's work, which is what a loop that observes every control period pays.
  headline   bench.py's step time (ms_per_step of `python bench.py --gpus 1 --no-cpu-baseline`), `--bench-runs` runs of this
             tree alternated with as many of the tree given with --parent-root (a checkout of the commit before the feature,
             built); without --parent-root that side is reported as not measured.
Usage: python scripts/bench_observe.py [--robots 65536] [--windows 40] [--calls 50] [--bench-runs 3] [--parent-root DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sai2_primitives_perso_amd as pkg  # noqa: E402
from bench_reset import Events  # noqa: E402


def headline(root, steps, warmup):
    """ms per step of one run of root/bench.py, in a process of its own (which also keeps its library apart from ours)"""
    root = os.path.abspath(root)
    env = {k: v for k, v in os.environ.items() if k != "SAI2B_LIB"}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--no-cpu-baseline"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {root} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


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
    c.tick(want_output=False)
    c.sim_step()
    criteria = dict(success_tasks=[0], pos_tolerance=0.02, ori_tolerance=0.05, joint_limit_margin=0.1, max_joint_speed=1.0, nonfinite=True,
                    force_tasks=[0], max_sensed_force=8.0, max_episode_steps=1000)
    selections = {
        "pose + twist + error of one task": dict(tasks=[0], task_blocks=["pose", "twist", "error"]),
        "every block": dict(blocks=list(pkg._abi.OBS_BLOCKS), tasks=[0], task_blocks=list(pkg._abi.OBS_TASK_BLOCKS)),
        "done byte only, all criteria": dict(criteria),
        "every block + all criteria": dict(blocks=list(pkg._abi.OBS_BLOCKS), tasks=[0], task_blocks=list(pkg._abi.OBS_TASK_BLOCKS), **criteria),
    }
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    cfgs, outs = {}, {}
    for name, sel in selections.items():
        cfgs[name] = c.observation_config(**sel)
        c.set_observation(cfgs[name])
        outs[name] = torch.zeros((c.observation_rows(), B), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def getters():
        c.get_mft_status(0)
        c.get_mft_velocity(0)
        c.get_state()

    def observe(name):
        rows = outs[name]
        if rows.shape[0] == 0:
            return lambda: c.observe(out=False, done=done)
        return lambda: c.observe(out=rows, done=done if cfgs[name].criteria else False)

    ev = Events(c)
    results = {}
    names = ["getters"] + list(selections)
    t = {n: [] for n in names}
    for n in selections:  # warm-up of every shape
        c.set_observation(cfgs[n])
        ev.time(observe(n), 3 * a.calls)
    ev.time(getters, 10)
    for _ in range(a.windows):  # the cases in turn, so that drift of the clocks falls on all alike
        t["getters"].append(ev.time(getters, max(1, a.calls // 10)))
        for n in selections:
            c.set_observation(cfgs[n])
            t[n].append(ev.time(observe(n), a.calls))
    base = statistics.median(t["getters"])
    label = {"getters": "host getters (get_mft_status + get_mft_velocity + get_state to host arrays)"}
    for n in names:
        v = sorted(t[n])
        m = statistics.median(v)
        results[n] = m
        what = label[n] if n in label else f"observe, {n}, device output ({outs[n].shape[0]} rows)"
        print(f"{what}: {m:.2f} us per call (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), {m / base:.4f} of the host getters", flush=True)
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
