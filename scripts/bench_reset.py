#!/usr/bin/env python3
"""Cost of an episode reset, one process, one GPU: 65 536 Pandas with the headline hierarchy (C3), everything device-resident.
  baseline   set_state(q, dq) + reinitialize(): the whole-batch pair (two device copies, reinit_kernel, otg_reinit_kernel)
  reset      reset_robots(mask, q, dq) with a device mask selecting 0 %, 1 % (scattered) and 100 % of the robots: one launch of
             reset_subset_kernel, whose wavefronts without a selected robot leave after their mask load
Time: HIP events on the context's stream around `calls` back-to-back calls, per call; the median of `windows` such windows
(10-90 % in brackets) after a warm-up. The interval covers whatever is slower, the host's enqueueing or the device's work,
which is what a loop that resets every control period pays.
Usage: python scripts/bench_reset.py [--robots 65536] [--windows 40] [--calls 50]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402


class Events:
    """two HIP events of the runtime the library runs on, recorded on the context's stream"""

    def __init__(self, ctrl):
        self.hip = C.CDLL(pkg._abi.LIB_PATH)
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.stream = C.c_void_p(ctrl.stream())
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, fn, calls):
        """-> microseconds per call"""
        assert self.hip.hipEventRecord(self.ev[0], self.stream) == 0
        for _ in range(calls):
            fn()
        assert self.hip.hipEventRecord(self.ev[1], self.stream) == 0
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value * 1e3 / calls


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    B = a.robots
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    c.tick(want_output=False)
    c.sim_step()
    q, dq = (torch.from_numpy(inp[k]).cuda() for k in ("q", "dq"))
    rng = np.random.default_rng(3)
    masks = {"0 %": np.zeros(B, dtype=bool), "1 % scattered": np.zeros(B, dtype=bool), "100 %": np.ones(B, dtype=bool)}
    masks["1 % scattered"][rng.choice(B, size=max(1, B // 100), replace=False)] = True
    wavefronts = {k: int(np.add.reduceat(m, np.arange(0, B, 64)).astype(bool).sum()) for k, m in masks.items()}
    dev = {k: torch.from_numpy(m).cuda() for k, m in masks.items()}
    torch.cuda.synchronize()

    def baseline():
        c.set_state(q, dq)
        c.reinitialize()

    cases = [("baseline: set_state + reinitialize", baseline)]
    for k in masks:
        cases.append((f"reset_robots, {k} ({int(masks[k].sum())} robots in {wavefronts[k]} of {(B + 63) // 64} wavefronts)",
                      lambda m=dev[k]: c.reset_robots(m, q, dq)))
    ev = Events(c)
    for _, fn in cases:
        ev.time(fn, 3 * a.calls)
    t = {name: [] for name, _ in cases}
    for _ in range(a.windows):  # the cases in turn, so that drift of the clocks falls on all alike
        for name, fn in cases:
            t[name].append(ev.time(fn, a.calls))
    base = statistics.median(t[cases[0][0]])
    for name, _ in cases:
        v = sorted(t[name])
        m = statistics.median(v)
        print(f"{name}: {m:.2f} us per call (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), {m / base:.3f} of the baseline", flush=True)
    c.tick(want_output=False)  # the context still works
    c.synchronize()
    c.close()


if __name__ == "__main__":
    main()
