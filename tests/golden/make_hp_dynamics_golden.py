#!/usr/bin/env python3
"""Generates tests/golden/hp_dynamics.npz: the exact rigid-body dynamics of the simulation harness (csrc/sai2b_sim.hip)
and exact control ticks of robots with prismatic joints inside the chain, from the 40-digit restatement
tests/hp_reference.py (no Newton-Euler recursion: bias() differentiates the body poses).

Dynamics cell <c> (tests/hp_dynamics_fixture.DYN_CELLS), [n][B] unless said:
  <c>.q, <c>.dq, <c>.tau: the inputs, on binary grids (q 2^-30, dq 2^-14, tau 2^-10); <c>.base_pos [3], <c>.base_rot
  [3][3] when the robot stands on a base transform
  <c>.b0: the exact b = C(q, dq) dq without gravity, <c>.g: g(q), rounded to float64 (b with gravity is b0 + g, to
  an ulp: hp_dynamics_fixture.answer)
  <c>.beta0, <c>.betag [B]: the forward-error scale, max over the joints of the sum of the absolute values of the
  products b is summed from; <c>.cond [B]: cond_2(M) (float32)
  <c>.<s>.q, <c>.<s>.dq: the exact state after the variant s of hp_dynamics_fixture.SIMS (tau held, dt 1e-3; sim1.q
  is not stored: it is q + dt sim1.dq);
  <c>.<s>.steps [2]: substeps, periods; <c>.<s>.xscale, <c>.<s>.minv [B]: over its steps the max of
  cond_2(M) ||M^-1 (tau - b)||_inf + ||M^-1||_2 ||beta||_inf, and of ||M^-1||_2 (float32)
Tick cell <c> (TICK_CELLS): the hierarchy of hp_dynamics_fixture.hierarchy, gravity compensation on, regular robots
only (no singular direction, every decision threshold make_hp_golden.near_threshold checks 1e-6 away):
  <c>.q, <c>.dq, <c>.mft<t>_{pos,rot,v,w,a,alpha}, <c>.jt<t>_{q,dq,ddq}: the inputs
  <c>.tau: the exact torques; <c>.kappa [B]: hp_reference.kappa_emp (float32)
  <c>.x [3][B], <c>.R [9][B], <c>.v, <c>.w [3][B]: the MotionForceTask's frame pose and J dq
  <c>.sim1.*: the exact state after one period (substeps 1, gravity) under the exact torques, as above

Run:  python tests/golden/make_hp_dynamics_golden.py [--check] [--jobs 16]   (deterministic; --check rebuilds in
memory and compares with the committed file bit for bit)
"""
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

import hp_dynamics_fixture as hd  # noqa: E402
import hp_reference as hp  # noqa: E402
import make_hp_golden as mhg  # noqa: E402
from make_hp_golden import _grid, serialise  # noqa: E402

_MODELS = {}


def model_of(cell, base):
    """hp_reference's model of a cell (base: the fixture's float64 base pose, or None)"""
    key = (cell, None if base is None else (tuple(base[0]), tuple(np.ravel(base[1]))))
    if key not in _MODELS:
        robot = (hd.DYN_CELLS.get(cell) or hd.TICK_CELLS[cell])["robot"]
        _MODELS[key] = hp.Model(hd.urdf_text(robot), base=base)
    return _MODELS[key]


def _f(v):
    return np.array([float(x) for x in v])


def sim_row(model, q, dq, tau, sub, periods, gravity):
    """the exact state after `periods` periods of `sub` substeps, and the scales of its bound"""
    info = []
    for _ in range(periods):
        q, dq = hp.sim_step(model, q, dq, tau, hd.DT, sub, gravity, info=info)
    xs = max(i["cond"] * i["x"] + i["minv"] * i["beta"] for i in info)
    return dict(q=_f(q), dq=_f(dq), xscale=xs, minv=max(i["minv"] for i in info))


def evaluate_dyn(args):
    cell, base, q, dq, tau, dps = args
    hp.mp.dps = dps
    model = model_of(cell, base)
    b0, beta0 = hp.bias_terms(model, q, dq, False)
    bg, betag = hp.bias_terms(model, q, dq, None)
    M, g = model.dynamics(hp.M_(q))[2:]
    with hp.mp.workdps(20):
        ev = hp.mp.eigsy(hp.mp.matrix(M.tolist()), eigvals_only=True)
        cond = float(max(ev) / min(ev))
    row = dict(b0=_f(b0), bg=_f(bg), g=_f(g), beta0=float(max(beta0)), betag=float(max(betag)), cond=cond)
    for name, sub, grav, periods in hd.SIMS:
        row[name] = sim_row(model, q, dq, tau, sub, periods, grav)
    return row


def dyn_inputs(cell):
    c = hd.DYN_CELLS[cell]
    rng = np.random.default_rng([4321, len(cell), sum(map(ord, cell))])
    model = model_of(cell, None)
    n, B = model.dof, c["B"]
    mid, half = (model.lower + model.upper) / 2, (model.upper - model.lower) / 2
    q = _grid(mid[:, None] + 0.6 * half[:, None] * rng.uniform(-1, 1, (n, B)), 30)
    dq = _grid(rng.normal(0, 0.5, (n, B)), 14)
    tau = _grid(rng.normal(0, 2.0, (n, B)), 10)
    return q, dq, tau


def _pack_sims(data, cell, rows, names):
    for name in names:
        sub, periods = next((s, p) for nm, s, _, p in hd.SIMS if nm == name)
        data[f"{cell}.{name}.steps"] = np.array([sub, periods], dtype=float)
        for k in ("q", "dq") if name != "sim1" else ("dq",):
            data[f"{cell}.{name}.{k}"] = np.array([r[name][k] for r in rows]).T.copy()
        for k in ("xscale", "minv"):
            data[f"{cell}.{name}.{k}"] = np.float32([r[name][k] for r in rows])


def build_dyn_cell(cell, pool, dps=40):
    c = hd.DYN_CELLS[cell]
    base = None if c["base"] is None else c["base"]()
    q, dq, tau = dyn_inputs(cell)
    rows = pool.map(evaluate_dyn, [(cell, base, q[:, b], dq[:, b], tau[:, b], dps) for b in range(q.shape[1])], chunksize=2)
    data = {f"{cell}.q": q, f"{cell}.dq": dq, f"{cell}.tau": tau}
    if base is not None:
        data[f"{cell}.base_pos"], data[f"{cell}.base_rot"] = np.asarray(base[0], dtype=float), np.asarray(base[1], dtype=float)
    assert all(np.array_equal(r["bg"], r["b0"] + r["g"]) or np.abs(r["bg"] - r["b0"] - r["g"]).max() <= 2 * hd.EPS * r["betag"]
               for r in rows)
    for k in ("b0", "g"):
        data[f"{cell}.{k}"] = np.array([r[k] for r in rows]).T.copy()
    for k in ("beta0", "betag", "cond"):
        data[f"{cell}.{k}"] = np.float32([r[k] for r in rows])
    _pack_sims(data, cell, rows, [s[0] for s in hd.SIMS])
    return data


def tick_tasks(cell):
    import sai2_primitives_perso_amd as pkg

    robot = hd.TICK_CELLS[cell]["robot"]
    m, links = pkg.model_from_urdf(hd.urdf_text(robot), is_file=False)
    return mhg.config_tasks(hd.configs(robot, pkg.joint_task_config, pkg.motion_force_task_config, links, m.dof),
                            hd.hierarchy(robot, m.dof))


def tick_inputs(cell, count):
    """poses and goals of `count` candidate robots, in order (deterministic)"""
    import sai2_primitives_perso_amd as pkg
    import urdf_np

    robot = hd.TICK_CELLS[cell]["robot"]
    rng = np.random.default_rng([2468, len(cell), sum(map(ord, cell))])
    chain = urdf_np.Chain(hd.urdf_text(robot), is_file=False)
    model = model_of(cell, None)
    n = model.dof
    mid, half = (model.lower + model.upper) / 2, (model.upper - model.lower) / 2
    q = _grid(mid[:, None] + 0.6 * half[:, None] * rng.uniform(-1, 1, (n, count)), 30)
    dq = _grid(rng.normal(0, 0.3, (n, count)), 14)
    goals = []
    for kind, *rest in hd.hierarchy(robot, n):
        if kind == "jt":
            S = np.eye(n) if rest[0] is None else rest[0]
            k0 = S.shape[0]
            goals.append(dict(q=_grid(S @ q + rng.normal(0, 0.1, (k0, count)), 22), dq=_grid(rng.normal(0, 0.1, (k0, count)), 14),
                              ddq=_grid(rng.normal(0, 0.2, (k0, count)), 14)))
            continue
        pos, rot = np.empty((3, count)), np.empty((9, count))
        for b in range(count):
            _, x, R = chain.jacobian(q[:, b], rest[0], rest[1])
            ax = rng.normal(size=(1, 3))
            ax /= np.linalg.norm(ax)
            pos[:, b] = x + rng.uniform(-0.05, 0.05, 3)
            rot[:, b] = (R @ pkg.workloads._expmap(ax * rng.uniform(0, 0.2))[0]).ravel()
        goals.append(dict(pos=_grid(pos, 22), rot=_grid(rot, 22), v=_grid(rng.normal(0, 0.05, (3, count)), 14),
                          w=_grid(rng.normal(0, 0.05, (3, count)), 14), a=_grid(rng.normal(0, 0.1, (3, count)), 14),
                          alpha=_grid(rng.normal(0, 0.1, (3, count)), 14)))
    return q, dq, goals


def evaluate_tick(args):
    """the exact tick of one robot and the period after it: None when it is singular or sits on a threshold (b: the
    robot's place in the cell, the seed of its kappa_emp)"""
    cell, tasks, q, dq, goals, b, dps, full = args
    hp.mp.dps = dps
    model = model_of(cell, None)
    state = hp.new_state(model, tasks)
    before = hp.copy.deepcopy(state)
    tau, info, kin = hp.tick(model, tasks, state, q, dq, goals, gravity_comp=True)
    t = next(i for i, x in enumerate(tasks) if x["kind"] == "mft")
    if info[t]["sc"] > 0 or mhg.near_threshold(tasks, info, q, model):
        return None
    if not full:
        return {}
    kap = hp.kappa_emp(model, tasks, before, q, dq, goals, tau, info, kin, seed=[b, 0], gravity_comp=True)
    J, x, R = kin["frames"][t]
    V = J @ hp.M_(dq)
    return dict(tau=_f(tau), kappa=kap, x=_f(x), R=_f(R.ravel()), v=_f(V[:3]), w=_f(V[3:]),
                sim1=sim_row(model, q, dq, tau, 1, 1, True))


def build_tick_cell(cell, pool, dps=40):
    B = hd.TICK_CELLS[cell]["B"]
    tasks = tick_tasks(cell)
    q, dq, goals = tick_inputs(cell, 8 * B)
    rg = lambda b: [{k: v[:, b] for k, v in g.items()} for g in goals]
    ok = pool.map(evaluate_tick, [(cell, tasks, q[:, b], dq[:, b], rg(b), b, dps, False) for b in range(q.shape[1])], chunksize=4)
    keep = [b for b, r in enumerate(ok) if r is not None][:B]
    assert len(keep) == B, (cell, len(keep), B)
    rows = pool.map(evaluate_tick, [(cell, tasks, q[:, b], dq[:, b], rg(b), i, dps, True) for i, b in enumerate(keep)], chunksize=2)
    data = {f"{cell}.q": q[:, keep], f"{cell}.dq": dq[:, keep]}
    for t, (g, task) in enumerate(zip(goals, tasks)):
        for k, v in g.items():
            data[f"{cell}.{task['kind']}{t}_{k}"] = np.ascontiguousarray(v[:, keep])
    for k in ("tau", "x", "R", "v", "w"):
        data[f"{cell}.{k}"] = np.array([r[k] for r in rows]).T.copy()
    data[f"{cell}.kappa"] = np.float32([r["kappa"] for r in rows])
    _pack_sims(data, cell, rows, ["sim1"])
    return data


def build(jobs=16, cells=None):
    ctx = multiprocessing.get_context("fork")
    data = {}
    with ctx.Pool(min(jobs, 16)) as pool:
        for cell in cells or list(hd.DYN_CELLS) + list(hd.TICK_CELLS):
            data.update(build_dyn_cell(cell, pool) if cell in hd.DYN_CELLS else build_tick_cell(cell, pool))
            print(cell, "done", flush=True)
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    blob = serialise(build(a.jobs))
    if a.check:
        with open(hd.FIXTURE, "rb") as f:
            same = f.read() == blob
        print("fixture reproduced bit for bit" if same else "fixture DIFFERS from the committed file")
        sys.exit(0 if same else 1)
    with open(hd.FIXTURE, "wb") as f:
        f.write(blob)
    print(f"{os.path.relpath(hd.FIXTURE, ROOT)}: {len(blob)} bytes")


if __name__ == "__main__":
    main()
