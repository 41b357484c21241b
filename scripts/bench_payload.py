#!/usr/bin/env python3
"""Step time of a context with per-robot payloads against the same context without, one process, one GPU: 65 536 Pandas, the
two controllers alive side by side, short windows of back-to-back ticks alternating between them, the median window of each
(warm-up first; as bench.py, time is host wall clock around enqueue + synchronize of a window).
Cases: the headline hierarchy (C3), the three-level hierarchy (C4), C3 on the 16-lane generic tick alone, and the single-task
hierarchy C2 at its 4 096 robots (the FAST = 1 kernels).
Usage: python scripts/bench_payload.py [--robots 65536] [--windows 60] [--ticks 50]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402


def make(config, B, env, payload):
    inp = pkg.workloads.make_inputs(config, B=B, seed=1)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    pkg.workloads.load_inputs(c, inp)
    if payload:
        rng = np.random.default_rng(7)
        m = rng.uniform(0.1, 3.0, B)
        com = rng.uniform(-0.1, 0.1, (3, B))
        A = rng.normal(size=(B, 3, 3)) * 0.1
        S = A @ A.transpose(0, 2, 1)
        I = np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]])
        c.set_link_payload(6, m, com, np.ascontiguousarray(I))
    return c


def window(c, ticks):
    t0 = time.perf_counter()
    for _ in range(ticks):
        c.tick(want_output=False)
    c.synchronize()
    return (time.perf_counter() - t0) / ticks * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=60)
    ap.add_argument("--ticks", type=int, default=50)
    a = ap.parse_args()
    cases = [("C3 headline tick", 3, {}, a.robots), ("C4 three-level hierarchy", 4, {}, a.robots),
             ("C3, 16-lane generic tick", 3, {"SAI2B_NO_FAST_PATH": "1", "SAI2B_GENERIC_LANES": "16"}, a.robots),
             ("C2 single task, 4 096 robots", 2, {}, 4096)]
    for name, config, env, robots in cases:
        plain, loaded = make(config, robots, env, False), make(config, robots, env, True)
        for c in (plain, loaded):
            window(c, 3 * a.ticks)
        t = {0: [], 1: []}
        for _ in range(a.windows):
            t[0].append(window(plain, a.ticks))
            t[1].append(window(loaded, a.ticks))
        m0, m1 = statistics.median(t[0]), statistics.median(t[1])
        q = lambda v: (sorted(v)[len(v) // 10], sorted(v)[-1 - len(v) // 10])
        print(f"{name}: no payload {m0:.2f} us (10-90 %: {q(t[0])[0]:.2f}-{q(t[0])[1]:.2f}), payload {m1:.2f} us "
              f"({q(t[1])[0]:.2f}-{q(t[1])[1]:.2f}), ratio {m1 / m0:.3f}", flush=True)
        plain.close(), loaded.close()


if __name__ == "__main__":
    main()
