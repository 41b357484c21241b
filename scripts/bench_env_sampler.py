#!/usr/bin/env python3
"""Cost of redrawing the plant on the device, one process, one GPU: 65 536 Pandas with the headline hierarchy (C3), a payload on
both targets, a contact, joint dynamics, hardware and an external wrench in force, everything device-resident, masks selecting
0 %, 1 % (scattered) and 100 % of the robots.
  randomize_robots      each group alone and all groups together
  parent form           what the library offered before the sampler: the same number of draws in torch ops, merged with the
                        rows of the robots the mask leaves alone (the setters have no mask), then the five whole-batch setters
                        with device tensors
  copy                  one hipMemcpyAsync, device to device, of half the bytes the full-mask call of all groups reads and
                        writes (a copy of n bytes reads n and writes n): the nominal rows in, the feature and sample rows out
Time: HIP events on the context's stream around `calls` back-to-back calls, per call; the median of `windows` such windows
(10-90 % in brackets) after a warm-up, the cases taken in turn within every window.
Usage: python scripts/bench_env_sampler.py [--robots 65536] [--windows 30] [--calls 20]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sai2_primitives_perso_amd as pkg  # noqa: E402
from bench_reset import Events  # noqa: E402
from sai2_primitives_perso_amd import _abi  # noqa: E402

N, LINK, MAX_DELAY = 7, 6, 4
CFG = dict(seed=7, groups=tuple(_abi.ENV_GROUPS), payload_target="both", payload_mass_scale=(0.5, 1.5), payload_com_half=(0.01, 0.02, 0.0),
           contact_height=(-0.01, 0.03), contact_tilt_max=0.3, contact_stiffness_scale=(0.5, 2.0, 1), contact_damping_scale=(0.8, 1.2),
           contact_friction_scale=(0.5, 1.5), armature_scale=(0.5, 1.5), damping_scale=(0.0, 2.0), friction_scale=(0.9, 1.1),
           torque_limit_scale=(0.7, 1.0), delay_lower=1, delay_upper=3, lag_scale=(0.8, 1.2), gain_scale=(0.95, 1.05),
           torque_noise_scale=(0.5, 1.5), sensor_bias_half=(0.1, 0.1, 0.1, 0.01, 0.01, 0.0), sensor_noise_scale=(0.5, 2.0),
           push_force=(1.0, 10.0), push_moment=(0.0, 1.0), push_steps_lower=0, push_steps_upper=20)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    B = a.robots
    inp = pkg.workloads.make_inputs(3, B=B, seed=1)
    rng = np.random.default_rng(3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()

    c = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B, device=0)
    pkg.workloads.load_inputs(c, inp)
    # the nominal plant: non-uniform per-robot rows of the five features
    nrm = rng.normal(size=(3, B))
    nom = dict(payload=dev(np.concatenate([rng.uniform(0.2, 2.0, (1, B)), rng.uniform(-0.05, 0.05, (3, B)), rng.uniform(1e-3, 1e-2, (3, B)),
                                           rng.uniform(-1e-4, 1e-4, (3, B))])),
               contact=dev(np.concatenate([rng.uniform(-0.5, 0.5, (2, B)), rng.uniform(-0.2, 0.0, (1, B)), nrm / np.linalg.norm(nrm, axis=0),
                                           rng.uniform(1e3, 1e4, (1, B)), rng.uniform(0, 0.5, (1, B)), rng.uniform(0, 0.8, (1, B))])),
               joint=dev(np.concatenate([rng.uniform(0, 0.1, (N, B)), rng.uniform(0, 1, (N, B)), rng.uniform(0, 0.5, (N, B)), rng.uniform(20, 80, (N, B))])),
               actuator=dev(np.concatenate([rng.integers(0, MAX_DELAY + 1, (1, B)), rng.uniform(0.3, 0.8, (N, B)), rng.uniform(0.9, 1.1, (N, B)),
                                            rng.uniform(0, 0.2, (N, B))])),
               sensor=dev(np.concatenate([rng.uniform(-0.5, 0.5, (6, B)), rng.uniform(0, 0.1, (6, B)), rng.uniform(0.5, 1.0, (1, B))])),
               wrench=dev(np.zeros((7, B))))
    contact_cfg = c.contact_config(LINK, [[0.0, 0.0, 0.1]], 0, 1e-3)
    hw_cfg = c.hardware_config(MAX_DELAY, 0, 11, 0)

    def setters(r):
        """the five whole-batch setters with device tensors: what a caller without the sampler writes new rows with"""
        p = r["payload"]
        c.set_link_payload(LINK, p[0], p[1:4], p[4:10], target="both")
        k = r["contact"]
        c.set_contact(contact_cfg, None, k[0:3], k[3:6], k[6], k[7], k[8])
        j = r["joint"]
        c.set_joint_dynamics(armature=j[0:N], damping=j[N : 2 * N], friction=j[2 * N : 3 * N], torque_limit=j[3 * N : 4 * N])
        c.set_hardware(r["actuator"], r["sensor"], config=hw_cfg)
        w = r["wrench"]
        c.set_external_wrench(LINK, w[0:3], w[3:6], w[6])

    setters({k: v.clone() for k, v in nom.items()})
    c.tick(want_output=False)
    c.sim_step()
    c.set_env_sampler(**CFG)
    lay = c.env_sampler_layout(c.get_env_sampler())

    masks = {"0 %": np.zeros(B, dtype=bool), "1 % scattered": np.zeros(B, dtype=bool), "100 %": np.ones(B, dtype=bool)}
    masks["1 % scattered"][rng.choice(B, size=max(1, B // 100), replace=False)] = True
    dmask = {k: torch.from_numpy(m).cuda() for k, m in masks.items()}
    cur = {k: v.clone() for k, v in nom.items()}
    torch.cuda.synchronize()

    def lerp(r, u):
        if len(r) == 3 and r[2]:
            return torch.exp(math.log(r[0]) + (math.log(r[1]) - math.log(r[0])) * u)
        return r[0] + (r[1] - r[0]) * u

    def sphere(u0, u1):
        z, phi = 2 * u0 - 1, 2 * math.pi * u1
        r = torch.sqrt(1 - z * z)
        return torch.stack([r * torch.cos(phi), r * torch.sin(phi), z])

    def parent(m):
        u = torch.rand((32 + 7 * N, B), dtype=torch.float64, device="cuda")
        sel = m[None, :]
        p, k, j, h, s = nom["payload"], nom["contact"], nom["joint"], nom["actuator"], nom["sensor"]
        sc = lerp(CFG["payload_mass_scale"], u[0:1])
        half = torch.tensor(CFG["payload_com_half"], dtype=torch.float64, device="cuda")[:, None]
        cur["payload"] = torch.where(sel, torch.cat([p[0:1] * sc, p[1:4] + half * (2 * u[1:4] - 1), p[4:10] * sc]), cur["payload"])
        hgt, th, ax = lerp(CFG["contact_height"], u[4:5]), CFG["contact_tilt_max"] * u[5:6], sphere(u[6], u[7])
        n = k[3:6]
        turned = n * torch.cos(th) + torch.linalg.cross(ax, n, dim=0) * torch.sin(th) + ax * (ax * n).sum(0, keepdim=True) * (1 - torch.cos(th))
        mat = torch.cat([k[6:7] * lerp(CFG["contact_stiffness_scale"], u[8:9]), k[7:8] * lerp(CFG["contact_damping_scale"], u[9:10]),
                         k[8:9] * lerp(CFG["contact_friction_scale"], u[10:11])])
        cur["contact"] = torch.where(sel, torch.cat([k[0:3] + hgt * n, turned, mat]), cur["contact"])
        js = torch.cat([lerp(CFG[name], u[11 + i * N : 11 + (i + 1) * N]) for i, name in enumerate(("armature_scale", "damping_scale", "friction_scale", "torque_limit_scale"))])
        cur["joint"] = torch.where(sel, j * js, cur["joint"])
        o = 11 + 4 * N
        delay = CFG["delay_lower"] + torch.floor((CFG["delay_upper"] - CFG["delay_lower"] + 1) * u[o : o + 1])
        hs = torch.cat([lerp(CFG[name], u[o + 1 + i * N : o + 1 + (i + 1) * N]) for i, name in enumerate(("lag_scale", "gain_scale", "torque_noise_scale"))])
        act = torch.cat([delay, h[1:] * hs])
        act[1 : 1 + N].clamp_(max=1.0)
        cur["actuator"] = torch.where(sel, act, cur["actuator"])
        o += 1 + 3 * N
        bias = torch.tensor(CFG["sensor_bias_half"], dtype=torch.float64, device="cuda")[:, None]
        cur["sensor"] = torch.where(sel, torch.cat([s[0:6] + bias * (2 * u[o : o + 6] - 1), s[6:12] * lerp(CFG["sensor_noise_scale"], u[o + 6 : o + 7]), s[12:13]]),
                                    cur["sensor"])
        o += 7
        f, mo = lerp(CFG["push_force"], u[o : o + 1]) * sphere(u[o + 1], u[o + 2]), lerp(CFG["push_moment"], u[o + 3 : o + 4]) * sphere(u[o + 4], u[o + 5])
        steps = CFG["push_steps_lower"] + torch.floor((CFG["push_steps_upper"] - CFG["push_steps_lower"] + 1) * u[o + 6 : o + 7])
        cur["wrench"] = torch.where(sel, torch.cat([f, mo, steps]), cur["wrench"])
        setters(cur)

    # what the full-mask call of all groups reads and writes, in rows of B doubles
    rows_in = 10 + 10 + 9 + 4 * N + (1 + 3 * N) + 12
    rows_out = rows_in + 7 + lay["total"]
    moved = (rows_in + rows_out) * 8 * B + 9 * B  # (and the mask byte, the counter read and written)
    src, dst = (torch.zeros(moved // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
    ev = Events(c)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    torch.cuda.synchronize()

    def copy():
        assert ev.hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), moved // 2, 3, ev.stream) == 0  # hipMemcpyDeviceToDevice

    cases = []
    for k in masks:
        n = int(masks[k].sum())
        for g in list(_abi.ENV_GROUPS) + [0]:
            cases.append((f"randomize_robots, {g or 'all groups'}, {k} ({n} robots)", lambda m=dmask[k], g=g: c.randomize_robots(m, g)))
    # (the parent form's setters overwrite the feature rows, never the sampler's nominal: the draws of the other cases stay what they are)
    for k in masks:
        cases.append((f"parent form (torch draws, five whole-batch setters), {k}", lambda m=dmask[k]: parent(m)))
    cases.append((f"copy of {moved // 2} bytes (half of the {moved} the full call of all groups moves)", copy))
    for _, fn in cases:
        ev.time(fn, 2 * a.calls)
    t = {name: [] for name, _ in cases}
    for _ in range(a.windows):  # the cases in turn, so that drift of the clocks falls on all alike
        for name, fn in cases:
            t[name].append(ev.time(fn, a.calls))
    med = {}
    for name, _ in cases:
        v = sorted(t[name])
        med[name] = statistics.median(v)
        print(f"{name}: {med[name]:.2f} us per call (10-90 %: {v[len(v) // 10]:.2f}-{v[-1 - len(v) // 10]:.2f})", flush=True)
    full = next(v for k, v in med.items() if k.startswith("randomize_robots, all groups, 100 %"))
    for k in masks:
        own = next(v for n_, v in med.items() if n_.startswith(f"randomize_robots, all groups, {k}"))
        par = med[f"parent form (torch draws, five whole-batch setters), {k}"]
        print(f"all groups, {k}: parent form / randomize_robots = {par / own:.1f}")
    cp = next(v for k, v in med.items() if k.startswith("copy of"))
    print(f"all groups, 100 %: the copy takes {cp / full:.2f} of the call ({moved / full * 1e-3:.0f} GB/s moved by the call, {moved / cp * 1e-3:.0f} GB/s by the copy)")
    counts = c.env_sampler_counts()
    print(f"last call: {counts['drawn']} drawn, {counts['lag_clipped']} with a lag clipped")
    c.tick(want_output=False)  # the context still works
    c.sim_step()
    c.synchronize()
    c.close()


if __name__ == "__main__":
    main()
