#!/usr/bin/env python3
"""Period (tick + sim_step(None), torques never leaving the device) of the headline hierarchy C3 with and without contact
in the simulated plant, one process, one GPU: 65 536 Pandas, the contexts alive side by side, short windows of
back-to-back periods alternating between them, the median window of each (warm-up first; as bench.py, time is host wall
clock around enqueue + synchronize of a window; protocol of scripts/bench_payload.py).
Contexts: no contact (twice: the spread of a context measured against itself), one contact point and four, each with the
force sensor attached to the MotionForceTask. Every robot has its own plane 4 mm under its control point.
--round-trip adds the loop a force-controlled batch had to run before: the sensor detached, the state fetched every period,
the reading computed on the host (tests/contact_reference.py on the CPU oracle) and uploaded with set_mft_sensed_wrench;
it is orders slower, so it gets a few short windows of its own.
This commit against the previous one cannot be measured in one process (one process loads one library): run the script
once per build with SAI2B_LIB=<that build's libsai2b.so> (only the "no contact" rows exist on a build without contact:
--no-contact-only) in alternation and compare the "no contact" medians with the spread of the two "no contact" rows.
Usage: python scripts/bench_contact.py [--robots 65536] [--windows 60] [--periods 50] [--round-trip] [--no-contact-only]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sai2_primitives_perso_amd as pkg  # noqa: E402


def make(B, n_points):
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    if n_points:
        rng = np.random.default_rng(7)
        R, p = pkg.workloads.fk(inp["q"].T)
        _, x, _ = pkg.workloads.frame_jacobian(R, p)
        point = np.ascontiguousarray(x.T) - np.array([[0.0], [0.0], [0.004]])
        normal = np.zeros((3, B))
        normal[2] = 1.0
        a = 0.04
        pts = [pkg.workloads.EE_FRAME_POS] if n_points == 1 else [(a, a, 0.1), (-a, a, 0.1), (-a, -a, 0.1), (a, -a, 0.1)]
        c.set_contact(pkg.workloads.EE_LINK, pts, point, normal, rng.uniform(1e3, 2e4, B), rng.uniform(0, 0.5, B), rng.uniform(0, 0.8, B),
                      sensor_task=0)
    return c


def window(c, periods):
    t0 = time.perf_counter()
    for _ in range(periods):
        c.tick(want_output=False)
        c.sim_step(None, 0.001, 1)
    c.synchronize()
    return (time.perf_counter() - t0) / periods * 1e6


def round_trip(B, windows, periods):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    from contact_reference import ContactReference

    c = make(B, 1)
    cfg, rows = c.get_contact()
    cfg.sensor_task = -1
    c.set_contact(cfg, None, rows[0:3], rows[3:6], rows[6], rows[7], rows[8])
    ref = ContactReference(ol.panda_model(), B, cfg.link, np.array([list(cfg.points[0])]), rows, threads=16)
    o = ol.Oracle(ol.panda_model(), ol.task_configs(pkg.workloads.make_inputs(3, B=B, seed=1)["tasks"]), B, threads=16)
    t = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(periods):
            c.tick(want_output=False)
            c.sim_step(None, 0.001, 1)
            ref.set_state(*c.get_state())
            rep = ref.report(sensor=(o, 0))
            c.set_mft_sensed_wrench(0, np.ascontiguousarray(rep["sensed"][:3]), np.ascontiguousarray(rep["sensed"][3:]))
        t.append((time.perf_counter() - t0) / periods * 1e6)
    print(f"round trip through the host, 1 point: {statistics.median(t):.0f} us per period ({min(t):.0f}-{max(t):.0f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=60)
    ap.add_argument("--periods", type=int, default=50)
    ap.add_argument("--round-trip", action="store_true")
    ap.add_argument("--no-contact-only", action="store_true")
    a = ap.parse_args()
    if a.no_contact_only:
        ctx = [make(a.robots, 0), make(a.robots, 0)]
        for c in ctx:
            window(c, 3 * a.periods)
        t = [[], []]
        for _ in range(a.windows):
            for k, c in enumerate(ctx):
                t[k].append(window(c, a.periods))
        print("no contact: " + " / ".join(f"{statistics.median(v):.2f}" for v in t) + " us per period", flush=True)
        return
    names = ["no contact", "no contact (again)", "1 point + sensor", "4 points + sensor"]
    ctx = [make(a.robots, n) for n in (0, 0, 1, 4)]
    for c in ctx:
        window(c, 3 * a.periods)
    t = [[] for _ in ctx]
    for _ in range(a.windows):
        for k, c in enumerate(ctx):
            t[k].append(window(c, a.periods))
    med = [statistics.median(v) for v in t]
    for k, name in enumerate(names):
        v = sorted(t[k])
        print(f"{name}: {med[k]:.2f} us per period (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f}), x{med[k] / med[0]:.3f}", flush=True)
    if a.round_trip:
        round_trip(a.robots, 3, 5)
    print(f"robots in contact at the end: {ctx[2].robots_in_contact()} / {ctx[3].robots_in_contact()} of {a.robots}")


if __name__ == "__main__":
    main()
