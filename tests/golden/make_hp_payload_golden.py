#!/usr/bin/env python3
"""Generates tests/golden/hp_payload.npz: robots WITH A PAYLOAD in and around the singularity-blending region of a
MotionForceTask, with the exact answer of their control tick from the 40-digit tests/hp_reference.py on the robot's URDF text
plus the payload as a body on a fixed joint (tests/payload_cases.py). 32 poses of tests/singular_poses.py (the 6R arm's
3-row and 6-row tasks, the sliding-base Panda's 6-row task behind a JointTask), two payloads alternating over the robots. Arrays per cell as in
tests/golden/hp_singular.npz (make_hp_golden.py, whose candidates, threshold test and serialisation these are); the same
rejection of poses within 1e-6 of a decision threshold.

Run:  python tests/golden/make_hp_payload_golden.py [--check]   (deterministic)"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import hp_reference as hp  # noqa: E402
import make_hp_golden as mg  # noqa: E402
import payload_cases as pc  # noqa: E402

_MODELS = {}


def evaluate(args):
    """the exact tick of one robot with its payload: None when it sits on a threshold"""
    cell, text_k, tasks, q, dq, goals, b = args
    hp.mp.dps = 40
    if (cell, text_k) not in _MODELS:
        _MODELS[cell, text_k] = hp.Model(pc.hp_texts(cell)[text_k])
    model = _MODELS[cell, text_k]
    state = hp.new_state(model, tasks)
    before = hp.copy.deepcopy(state)
    tau, info, kin = hp.tick(model, tasks, state, q, dq, goals)
    if mg.near_threshold(tasks, info, q, model) or not np.isfinite(float(hp.norm_inf(tau))):
        return None
    kap = hp.kappa_emp(model, tasks, before, q, dq, goals, tau, info, kin, seed=[b, 0])
    inf = info[next(i for i, x in enumerate(tasks) if x["kind"] == "mft")]
    return dict(tau=np.array([float(x) for x in tau]), alpha=float(inf["alpha"]), nsing=inf["sc"], c1=inf["c1"], c2=inf["c2"], kappa=kap)


def build_cell(cell, B, pool):
    tasks = mg.truth_tasks(cell)
    qs, dq, goals = mg.candidates(cell, 3 * B)
    P = len(pc.HP_PAYLOADS)
    # robot b of the fixture carries payload b % P: candidates are taken in order, each tried with the payload of the slot it
    # would fill
    keep, rows = [], []
    res = {k: pool.map(evaluate, [(cell, k, tasks, qs[0, :, b], dq[:, b], mg.robot_goals(goals, b), b) for b in range(qs.shape[2])])
           for k in range(P)}
    for b in range(qs.shape[2]):
        r = res[len(keep) % P][b]
        if r is not None and len(keep) < B:
            keep.append(b), rows.append(r)
    assert len(keep) == B, (cell, len(keep))
    data = {f"{cell}.q": qs[:, :, keep], f"{cell}.dq": dq[:, keep]}
    for t, g in enumerate(goals):
        for k, v in g.items():
            data[f"{cell}.{tasks[t]['kind']}{t}_{k}"] = np.ascontiguousarray(v[:, keep])
    data[f"{cell}.tau"] = np.array([r["tau"] for r in rows]).T[None].copy()
    for key in ("alpha", "nsing", "c1", "c2", "kappa"):
        data[f"{cell}.{key}"] = np.array([[r[key] for r in rows]], dtype=float)
    data[f"{cell}.kappa"] = np.float64(np.float32(data[f"{cell}.kappa"]))
    assert (data[f"{cell}.nsing"] > 0).sum() >= B // 4 and (data[f"{cell}.nsing"] == 0).any(), data[f"{cell}.nsing"]
    return data


def build():
    data = {}
    with multiprocessing.get_context("fork").Pool(8) as pool:
        for cell, B in pc.HP_CELLS.items():
            data.update(build_cell(cell, B, pool))
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    blob = mg.serialise(build())
    if a.check:
        same = open(pc.HP_FIXTURE, "rb").read() == blob
        print("fixture reproduced bit for bit" if same else "fixture DIFFERS from the committed file")
        sys.exit(0 if same else 1)
    with open(pc.HP_FIXTURE, "wb") as f:
        f.write(blob)
    z = np.load(pc.HP_FIXTURE)
    print(len(blob), "bytes;", {c: int((z[f"{c}.nsing"] > 0).sum()) for c in pc.HP_CELLS}, "robots in the region")


if __name__ == "__main__":
    main()
