#!/usr/bin/env python3
"""Snapshot banks (sai2b_snapshot_save / _load) against a device-to-device copy of the same number of bytes, one process, one
GPU: 65 536 Pandas on the headline hierarchy C3 with the generators off, acceleration-limited and jerk-limited (the per-robot
size differs several-fold between the three). The yardstick is not the code under test: a hipMemcpyAsync (torch's
Tensor.copy_ between two device buffers) of words * 4 * robots bytes on the same stream. Windows of `calls` back-to-back
calls alternate between the cases, HIP events on the context's stream around each window, the median of `windows` windows of
each (warm-up first; protocol of scripts/bench_external_wrench.py). Slots and masks are device tensors, so nothing is staged.
Cases: identity save, identity load, a load with an empty mask, a load of 1 % of the robots (scattered), a clone of slot 0
into every robot, a load through a random permutation of the slots.
Usage: python scripts/bench_snapshot.py [--robots 65536] [--windows 20] [--calls 20] [--out profiles/snapshot_bench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402

MODES = {"generators off": (False, False), "acceleration-limited": (True, False), "jerk-limited": (True, True)}


def make(B, otg, jerk):
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    cfgs = [pkg.motion_force_task_config("m", internal_otg=otg), pkg.joint_task_config("j", internal_otg=otg)]
    for c in cfgs:
        c.internal_otg_jerk_limited = 1 if jerk else 0
    c = pkg.Controller(pkg.panda_model(), cfgs, B, device=0)
    c.set_state(inp["q"], inp["dq"])
    c.reinitialize()
    for _ in range(3):
        c.tick(want_output=False)
        c.sim_step(None, 0.001, 1)
    c.synchronize()
    return c


def window(stream, fn, calls):
    """device time of `calls` back-to-back calls, us per call"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(calls):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.robots
    lines = [f"snapshot banks, {B} Pandas, hierarchy C3 [MotionForceTask, JointTask]; median of {a.windows} windows of {a.calls} calls, us per call",
             "bytes: what the call moves on one side (robots moved x words x 4); rate: bytes / time; ratio: rate / rate of the copy"]
    rng = np.random.default_rng(3)
    for mode, (otg, jerk) in MODES.items():
        c = make(B, otg, jerk)
        stream = torch.cuda.ExternalStream(c.stream())
        words = c.snapshot_words(pkg.SNAP_EPISODE)
        total = words * 4 * B
        with torch.cuda.stream(stream):
            src, dst = torch.zeros(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
            ident = torch.arange(B, dtype=torch.int32, device="cuda")
            zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
            perm = torch.from_numpy(rng.permutation(B).astype(np.int32)).cuda()
            none = torch.zeros(B, dtype=torch.bool, device="cuda")
            few = torch.from_numpy(rng.uniform(size=B) < 0.01).cuda()
            bank = c.snapshot_bank(B)
            bank.save()
            cases = [
                ("copy of the same bytes", lambda: dst.copy_(src), B),
                ("copy (again)", lambda: dst.copy_(src), B),
                ("identity save", lambda: bank.save(ident), B),
                ("identity load", lambda: bank.load(ident), B),
                ("load, empty mask", lambda: bank.load(ident, none), 0),
                ("load, 1 % scattered", lambda: bank.load(ident, few), int(few.sum().item())),
                ("clone of slot 0", lambda: bank.load(zeros), B),
                ("load, random permutation", lambda: bank.load(perm), B),
            ]
            for _, fn, _ in cases:
                window(stream, fn, 3 * a.calls)
            t = [[] for _ in cases]
            for _ in range(a.windows):
                for k, (_, fn, _) in enumerate(cases):
                    t[k].append(window(stream, fn, a.calls))
        med = [statistics.median(v) for v in t]
        copy_rate = total / med[0]
        lines.append(f"-- {mode}: {words} words = {words * 4} bytes per robot, {total / 2**20:.1f} MiB per batch")
        for k, (name, _, moved) in enumerate(cases):
            v = sorted(t[k])
            nbytes = moved * words * 4
            rate = nbytes / med[k]  # bytes per us
            lines.append(f"{name:<26} {med[k]:9.2f} us (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f})  {nbytes / 2**20:8.1f} MiB  "
                         f"{rate * 1e-6:7.3f} TB/s  x{rate / copy_rate:.3f} of the copy")
        print("\n".join(lines[-len(cases) - 1:]), flush=True)
        bank.close()
        c.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
