#!/usr/bin/env python3
"""Generates tests/golden/hp_plant.npz: the exact answers of the simulated plant (contact, joint dynamics, the external
wrench, the plant payload, the sensor rows) from the 40-digit model hp_reference.plant_step / plant_report, on the eight
cells of tests/hp_plant_fixture.CELLS, with the per-robot scales of its bound (hp_plant_fixture's docstring).

Cell <c>, [rows][B] with B = 67; inputs float32 (values a float32 holds exactly), answers float64, scales float32:
  <c>.q, <c>.dq, <c>.tau [n][B]; <c>.joint [6][n][B], <c>.stop_k [n]; <c>.contact [9][B]; <c>.wrench [7][B] (F and M of a
  link-frame wrench in the URDF frame of the link); <c>.base_pos [3], <c>.base_rot [9] (float64, batch-uniform)
  <c>.p1.dq, <c>.p1.s_dq: one period of one substep
  <c>.p2x3.q, .dq, .depth, .normal_force [K][B], .wrench_world [6][B], .stop_torque, .dissipative_torque [n][B], .ext_wrench
  [6][B], .ext_torque [n][B], .sensed<t> [6][B] after two periods of three substeps; .s_<check> [B] per check of
  hp_plant_fixture.checks; .flags [2][4][B] (uint8: touching, at_stop, saturated, pushed after each period), .steps [2][B]

Edge robots take the first slots of every cell that has the feature (EDGES), the others are drawn at random. A robot is
redrawn until the conditions of hp_plant_fixture's docstring hold in the 40-digit model after each period.

Run:  python tests/golden/make_hp_plant_golden.py [--check] [--jobs 8]   (deterministic; --check rebuilds in memory and
compares with the committed file bit for bit)"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import hp_plant_fixture as hf  # noqa: E402
import hp_reference as hp  # noqa: E402
from make_hp_golden import serialise  # noqa: E402

DIRS = 8  # seeded perturbed runs per robot
EDGES = {
    "joint": ("dq_zero", "dq_tiny", "tau_at_limit", "infinite", "on_lower", "lower_clipped", "upper_clipped", "armature_mixed", "damping_huge"),
    "contact": ("along_normal", "vt_tiny", "vt_large", "damping_clipped", "lift_off", "frictionless"),
    "wrench": ("for_ever", "one_period", "off", "nan", "zero_wrench"),
}
_SETUP = {}


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _f(v):
    return np.array([float(x) for x in np.ravel(v)]).reshape(np.shape(v))


def edges_of(cell):
    c = hf.CELLS[cell]
    return [(k, e) for k in ("joint", "contact", "wrench") if c[k] for e in EDGES[k]]


def setup(cell):
    """the 40-digit models of a cell (one per payload), its tasks and its batch-uniform inputs"""
    if cell in _SETUP:
        return _SETUP[cell]
    import payload_cases as pc

    c = hf.CELLS[cell]
    text = hf.urdf_text(c["robot"])
    base = None if c["base"] is None else c["base"]()
    model = hp.Model(text, base=base)
    carried = None
    if c["payload"] is not None:
        m, com, I = hf.payloads()
        carried = [hp.Model(pc.urdf_with_payload(text, c["payload"], m[k], com[:, k], I[:, k]), base=base) for k in range(hf.P)]
        assert pc.link_name(text, c["payload"]) == hf.link_name(c["robot"], c["payload"])
    tasks = [dict(link=hf.link_name(c["robot"], l), point=np.array(hf.FRAME_POINT), frot=np.eye(3), sensor_rot=hf.SENSOR_ROT,
                  sensor_pos=hf.SENSOR_POS) for l in c["tasks"]]
    for f in ("contact", "wrench"):
        if c[f]:
            assert model.moving[c[f]["link"]]["child"] == hf.link_name(c["robot"], c[f]["link"])
    rng = np.random.default_rng([31, sum(map(ord, cell))])
    stop_k = f32(np.exp(rng.uniform(np.log(2e3), np.log(1e5), model.dof)))
    _SETUP[cell] = dict(model=model, carried=carried, tasks=tasks, base=base, stop_k=stop_k, seed=sum(map(ord, cell)) * 1000 + len(cell))
    return _SETUP[cell]


def features(cell, inp, b):
    """the dicts hp_reference.plant_step takes, for robot b with the inputs inp"""
    c, s = hf.CELLS[cell], setup(cell)
    n = s["model"].dof
    joint = contact = wrench = None
    if c["joint"]:
        joint = dict(rows=inp["joint"], k=s["stop_k"], c=np.full(n, hf.STOP_DAMPING), e=np.full(n, hf.FRICTION_EPS))
    if c["contact"]:
        con = c["contact"]
        contact = dict(link=hf.link_name(c["robot"], con["link"]), points=hf.points(con["n_points"]), rows=inp["contact"], v_eps=hf.V_EPS,
                       sensor=s["tasks"][con["sensor"]] if con["sensor"] >= 0 else None)
    if c["wrench"]:
        w = c["wrench"]
        wrench = dict(link=hf.link_name(c["robot"], w["link"]), point=np.array(hf.WRENCH_POINT), frame=w["frame"], rows=np.array(inp["wrench"]),
                      sensor=s["tasks"][w["sensor"]] if w["sensor"] >= 0 else None)
    payload = s["carried"][b % hf.P] if s["carried"] is not None else None
    return joint, contact, wrench, payload


def run(cell, inp, b, noise=None, conv=None):
    """both variants of robot b -> dict of float arrays (p1.dq, p2x3.*), the flags and steps per period, and `ok`: the
    conditions on the inputs hold. conv: what turns the model's numbers into the arrays (default: floats)"""
    _f = conv or globals()["_f"]
    s = setup(cell)
    model, tasks = s["model"], s["tasks"]
    joint, contact, wrench, payload = features(cell, inp, b)
    info = None if noise is None else dict(noise=noise)
    kw = dict(joint=joint, contact=contact, payload=payload, info=info)
    out = {}
    _, dq1 = hp.plant_step(model, inp["q"], inp["dq"], inp["tau"], hf.DT, 1, True, wrench=wrench, **kw)
    out["p1.dq"] = _f(dq1)
    q, dq = inp["q"], inp["dq"]
    flags, steps, ok = [], [], True
    for _ in range(2):
        q, dq = hp.plant_step(model, q, dq, inp["tau"], hf.DT, 3, True, wrench=wrench, **kw)
        rep = hp.plant_report(model, q, dq, inp["tau"], joint=joint, contact=contact, wrench=wrench, info=info)
        flags.append([int(bool(rep.get(f, False))) for f in hf.FLAGS])
        if contact is not None:
            ok = ok and all(abs(x) >= 1e-9 for x in rep["depth"]) and not any(0 < x < 1e-6 for x in rep["normal_force"])
        if joint is not None:
            lo, hi = joint["rows"][4], joint["rows"][5]
            ok = ok and not any(abs(q[i] - hp.mpf(lo[i])) < 1e-9 or abs(q[i] - hp.mpf(hi[i])) < 1e-9 for i in range(model.dof))
        if wrench is not None:
            wrench = dict(wrench, rows=np.concatenate([wrench["rows"][:6], [rep["steps"]]]))
            steps.append(rep["steps"])
    out.update({"p2x3.q": _f(q), "p2x3.dq": _f(dq)})
    for key in ("depth", "normal_force", "wrench_world", "applied_torque", "stop_torque", "dissipative_torque", "ext_wrench", "ext_torque"):
        if key in rep:
            out[f"p2x3.{key}"] = _f(rep[key])
    for t, task in enumerate(tasks):
        if id(task) in rep["sensed"]:
            out[f"p2x3.sensed{t}"] = _f(rep["sensed"][id(task)])
    out["flags"], out["steps"], out["ok"] = np.array(flags, dtype=np.uint8), np.array(steps, dtype=float), ok
    return out


def scales(cell, inp, b, exact, dps_scale=1.0):
    """{<variant>.s_<check>: the scale of the bound} of robot b: the largest change over DIRS perturbed runs plus eps of
    the block's own size"""
    blocks = [("p1.s_dq", "p1.dq", slice(None)), ("p2x3.s_q", "p2x3.q", slice(None)), ("p2x3.s_dq", "p2x3.dq", slice(None))]
    blocks += [(f"p2x3.s_{check}", f"p2x3.{key}", rows) for check, key, rows in hf.checks(cell)]
    worst = {name: 0.0 for name, _, _ in blocks}
    for k in range(DIRS):
        got = run(cell, inp, b, noise=hp.Noise([setup(cell)["seed"], b, k], dps_scale))
        for name, key, rows in blocks:
            worst[name] = max(worst[name], float(np.abs(got[key][rows] - exact[key][rows]).max()))
    return {name: worst[name] + hf.EPS * float(np.abs(exact[key][rows]).max()) if worst[name] > 0 or np.any(exact[key][rows]) else 0.0
            for name, key, rows in blocks}


# ---- the inputs ----

def _kin(cell, q, dq, link, point):
    """world position and velocity of a point of a link, and the link's rotation (floats)"""
    model = setup(cell)["model"]
    pos, jinfo = model.poses(hp.M_(q))
    J, x, R = model.jacobian(pos, jinfo, link, hp.M_(point))
    return _f(x), _f(J[:3] @ hp.M_(dq)), _f(R)


def draw(cell, b, attempt):
    """the inputs of robot b (an edge robot in the first slots), attempt: which redraw"""
    c, s = hf.CELLS[cell], setup(cell)
    model = s["model"]
    n = model.dof
    rng = np.random.default_rng([77, s["seed"], b, attempt])
    edges = edges_of(cell)
    kind, edge = edges[b] if b < len(edges) else (None, None)
    lo, hi = model.lower.copy(), model.upper.copy()
    inp = {}
    if c["joint"]:
        rows = np.empty((6, n))
        rows[0], rows[1], rows[2], rows[3] = rng.uniform(0, 0.2, n), rng.uniform(0, 5, n), rng.uniform(0, 2, n), rng.uniform(5, 30, n)
        rows[4], rows[5] = lo + rng.uniform(0, 0.05, n), hi - rng.uniform(0, 0.05, n)
        rows = f32(rows)
        lo, hi = rows[4], rows[5]
        q = lo + (hi - lo) * rng.uniform(0.2, 0.8, n)
        tau = rng.normal(0, 20, n)
        inp["joint"] = rows
    else:
        q = (lo + hi) / 2 + 0.3 * (hi - lo) * rng.uniform(-1, 1, n)
        tau = rng.normal(0, 5, n)
    slow = cell == "joint_payload_contact" and kind is None and b % 2 == 0  # contact friction below v_eps on light outer links
    dq = rng.normal(0, 2e-4 if slow else 0.5, n)
    q, dq, tau = f32(q), f32(dq), f32(tau)
    if c["joint"]:
        i, up, by = int(rng.integers(0, n)), bool(rng.integers(0, 2)), rng.uniform(0.005, 0.03)
        if kind is None and rng.integers(0, 2):  # half of the random robots start beyond a stop
            q[i] = f32(hi[i] + by if up else lo[i] - by)
        if kind == "joint":
            j = 1 % n
            if edge == "dq_zero":
                dq[0] = 0.0
            elif edge == "dq_tiny":
                dq[:] = f32(1e-3 * hf.FRICTION_EPS * np.where(np.arange(n) % 2, -1.0, 1.0))
            elif edge == "tau_at_limit":
                tau[:] = np.where(np.arange(n) % 2, -rows[3], rows[3])
            elif edge == "infinite":
                rows[3], rows[4], rows[5] = np.inf, -np.inf, np.inf
            elif edge == "on_lower":
                q[j] = lo[j]
            elif edge == "lower_clipped":  # beyond the lower stop, 1 - c dq < 0
                q[j], dq[j] = f32(lo[j] - 0.02), 3.0
            elif edge == "upper_clipped":  # beyond the upper stop, 1 + c dq < 0
                q[j], dq[j] = f32(hi[j] + 0.02), -3.0
            elif edge == "armature_mixed":
                rows[0, 0], rows[0, 1] = 0.0, 10.0
            elif edge == "damping_huge":
                rows[1, n - 1] = 1e4
        near = (np.abs(np.abs(tau) - rows[3]) < 1e-6) & (np.abs(tau) != rows[3])
        tau[near] = f32(tau[near] * 0.5)
    if c["contact"]:
        con = c["contact"]
        name, pts = hf.link_name(c["robot"], con["link"]), hf.points(con["n_points"])
        k = float(f32(np.exp(rng.uniform(np.log(con["k"][0]), np.log(con["k"][1])))))
        d, mu = rng.uniform(0, 0.5), rng.uniform(0, 0.8)
        x0, v0, R = _kin(cell, q, dq, name, pts[0])
        if con["n_points"] > 1:  # a plane nearly parallel to the plate: the depths of the corners differ by a few N / k
            th, ph = rng.uniform(0, 1) * 10.0 / k / hf.PLATE, rng.uniform(0, 2 * np.pi)
            if edge == "lift_off":  # parallel: every corner leaves the surface
                th = 0.0
            nrm = R @ np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)])
        else:
            nrm = rng.normal(size=3)
        third, depth = int(rng.integers(0, 3)), rng.uniform(2, 30) / k
        only_lowest = False
        if kind == "contact":
            third = 2
            if con["n_points"] == 1 and edge != "along_normal":  # a normal the point's velocity has a good share along
                nrm = v0 / np.linalg.norm(v0) + 0.5 * rng.normal(size=3)
            if edge == "along_normal":  # the point that approaches along the normal is the one that touches
                nrm, only_lowest = -v0, con["n_points"] > 1
                for p in pts:
                    vj = _kin(cell, q, dq, name, p)[1]
                    hj = np.array([_kin(cell, q, dq, name, pp)[0] for pp in pts]) @ (-vj)
                    if np.argmin(hj) == int(np.flatnonzero((pts == p).all(axis=1))[0]):
                        nrm = -vj
                        break
            elif edge in ("vt_tiny", "vt_large"):
                nn = nrm / np.linalg.norm(nrm)
                vt = v0 - (nn @ v0) * nn
                dq = f32(dq * (1e-3 if edge == "vt_tiny" else 1e3) * hf.V_EPS / np.linalg.norm(vt))
            elif edge == "damping_clipped":
                nn = nrm / np.linalg.norm(nrm)
                dq, d = f32(dq * 3.0 / (nn @ v0)), 0.5
            elif edge == "lift_off":
                nn = nrm / np.linalg.norm(nrm)
                dq, depth = f32(dq * 0.5 / (nn @ v0)), 5e-5
            elif edge == "frictionless":
                mu = 0.0
        nrm = f32(nrm / np.linalg.norm(nrm))
        xs = np.array([_kin(cell, q, dq, name, p)[0] for p in pts])
        h = np.sort(xs @ nrm)
        if only_lowest:
            cc = h[0] + min(depth, 0.5 * (h[1] - h[0]))
        elif third == 0:
            cc = h[0] - rng.uniform(0.01, 0.05)
        elif third == 1 and len(h) > 1:
            jj = int(rng.integers(0, len(h) - 1))
            cc = h[jj] + rng.uniform(0.2, 0.8) * (h[jj + 1] - h[jj])
        else:
            cc = h[-1] + depth
        tang = rng.normal(size=3)
        tang -= (tang @ nrm) * nrm
        # the plane point: on the plane near the first contact point (its tangential offset costs no height)
        p0 = xs[0] + (cc - xs[0] @ nrm) * nrm / (nrm @ nrm) + 0.3 * tang
        inp["contact"] = f32(np.concatenate([p0, nrm, [k, d, mu]]))
    if c["wrench"]:
        rows = np.concatenate([rng.uniform(-30, 30, 3), rng.uniform(-5, 5, 3), [rng.choice([-1.0, -1.0, 1.0, 2.0, 4.0])]])
        if kind == "wrench":
            rows[6] = dict(for_ever=-1.0, one_period=1.0, off=0.0, nan=np.nan, zero_wrench=3.0)[edge]
            if edge == "zero_wrench":
                rows[:6] = 0.0
        inp["wrench"] = f32(rows)
    inp.update(q=q, dq=dq, tau=tau)
    return inp


def evaluate(args):
    """robot b of a cell: drawn (and redrawn until the conditions hold), its exact answers and its scales"""
    cell, b, dps = args
    hp.mp.dps = dps
    for attempt in range(12):
        inp = draw(cell, b, attempt)
        exact = run(cell, inp, b)
        if exact["ok"]:
            break
    else:
        raise AssertionError((cell, b, "no draw meets the conditions"))
    return inp, exact, scales(cell, inp, b, exact)


def row_of(cell, inp, b, dps=40):
    """the answers and scales of robot b from the fixture's own inputs (tests/test_hp_plant.py: regeneration)"""
    hp.mp.dps = dps
    exact = run(cell, inp, b)
    return exact, scales(cell, inp, b, exact)


def inputs_of(d, b):
    """robot b's inputs out of a loaded cell"""
    return {k: d[k][..., b] for k in ("q", "dq", "tau", "joint", "contact", "wrench") if k in d}


def build_cell(cell, pool):
    s = setup(cell)
    rows = pool.map(evaluate, [(cell, b, 40) for b in range(hf.B)], chunksize=1)
    data = {}
    for k in ("q", "dq", "tau", "joint", "contact", "wrench"):
        if k in rows[0][0]:
            data[f"{cell}.{k}"] = np.stack([r[0][k] for r in rows], axis=-1).astype(np.float32)
    if hf.CELLS[cell]["joint"]:
        data[f"{cell}.stop_k"] = s["stop_k"].astype(np.float32)
    if s["base"] is not None:
        data[f"{cell}.base_pos"], data[f"{cell}.base_rot"] = np.asarray(s["base"][0], dtype=float), np.asarray(s["base"][1], dtype=float).ravel()
    for k in rows[0][1]:
        if k.startswith("p") and k != "p2x3.applied_torque":
            data[f"{cell}.{k}"] = np.stack([r[1][k] for r in rows], axis=-1)
    data[f"{cell}.p2x3.flags"] = np.stack([r[1]["flags"] for r in rows], axis=-1)
    if hf.CELLS[cell]["wrench"]:
        data[f"{cell}.p2x3.steps"] = np.stack([r[1]["steps"] for r in rows], axis=-1)
    for k in rows[0][2]:
        data[f"{cell}.{k}"] = np.float32([r[2][k] for r in rows])
    return data


def build(jobs=8, cells=None):
    ctx = multiprocessing.get_context("fork")
    data = {}
    for cell in cells or list(hf.CELLS):
        setup(cell)
    with ctx.Pool(min(jobs, 16)) as pool:
        for cell in cells or list(hf.CELLS):
            data.update(build_cell(cell, pool))
            print(cell, "done", flush=True)
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--cells", nargs="*")
    ap.add_argument("--out", default=hf.FIXTURE)
    a = ap.parse_args()
    blob = serialise(build(a.jobs, a.cells))
    if a.check:
        with open(hf.FIXTURE, "rb") as f:
            same = f.read() == blob
        print("fixture reproduced bit for bit" if same else "fixture DIFFERS from the committed file")
        sys.exit(0 if same else 1)
    with open(a.out, "wb") as f:
        f.write(blob)
    print(f"{os.path.relpath(a.out, ROOT)}: {len(blob)} bytes")


if __name__ == "__main__":
    main()
