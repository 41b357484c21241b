#!/usr/bin/env python3
"""Generates tests/golden/hp_force.npz: the cells of tests/hp_force_fixture.py (force and moment spaces, open and closed
loop, the sensor frame, integral gains, feedback and velocity saturation, on Panda C3 / C4, six_r, sliding_base and
planar_4r) with the exact answer of their control ticks from the 40-digit restatement tests/hp_reference.py: robots in
and around the singularity-blending region, the pose mix of tests/golden/make_hp_golden.py.

Per cell <c>, [C][B] as every other fixture (B robots, T ticks):
  what hp_singular.npz holds (make_hp_golden.py): <c>.q, .dq, the goals, .tau, .ratio, .alpha, .nsing, .c1, .c2, .types,
  .kappa, .clamped, .branch
  <c>.mft<t>_{f,m,sf,sm} [3][B]: goal force and moment, sensed force and moment in the sensor frame (the same every tick)
  <c>.mft_integ [T][12][B], <c>.jt_integ [T][k][B]: the exact integrators after every tick rounded to float64
  (position, orientation, force, moment; the JointTasks' in hierarchy order)
  <c>.kappa_integ [T][5][B]: hp_reference.kappa_emp's condition number of the integrators, per group (position,
  orientation, force, moment, JointTask)
  <c>.sat_f, .sat_m, .sat_v, .sat_w, .sat_jt [T][B]: the force / moment feedback limit, the linear / angular velocity
  saturation and a JointTask's per-joint saturation were active
  <c>.ff [T][B]: ||F_f||, the force-related argument of the singularity handler
The inputs are on the grids of make_hp_golden.py, the wrenches on 2^-14.

A robot within 1e-6 (relative) of a decision of any of its ticks is rejected and the next candidate taken: the decisions
of make_hp_golden.py, the four norm thresholds (force and moment feedback, linear and angular desired velocity) and
every joint's JointTask saturation.

Run:  python tests/golden/make_hp_force_golden.py [--check] [--jobs 16]   (deterministic; --check rebuilds in memory
and compares with the committed file bit for bit)
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

import hp_force_fixture as ff  # noqa: E402
import hp_reference as hp  # noqa: E402
import make_hp_golden as mg  # noqa: E402
from hp_fixture import hierarchy, product_model  # noqa: E402


def config_tasks(cfgs, specs):
    """task configs -> the tasks as hp_reference takes them, with the numbers of the force, integral and saturation
    laws"""
    out = mg.config_tasks(cfgs, specs, plain=False)
    for t, cfg in zip(out, cfgs):
        t["dt"] = float(cfg.loop_timestep)
        t["vsat"] = bool(cfg.use_velocity_saturation)
        if t["kind"] == "jt":
            k0 = cfg.task_dof
            t.update(ki=np.array(cfg.ki[:k0]), sat=np.array(cfg.saturation_velocity[:k0]))
            continue
        assert not cfg.passivity_enabled
        t.update(fdim=int(cfg.force_space_dimension), mdim=int(cfg.moment_space_dimension), faxis=np.array(cfg.force_axis[:]),
                 maxis=np.array(cfg.moment_axis[:]), in_frame=bool(cfg.parametrization_in_compliant_frame),
                 cl_force=bool(cfg.closed_loop_force), cl_moment=bool(cfg.closed_loop_moment), ki_pos=np.array(cfg.ki_pos[:]),
                 ki_ori=np.array(cfg.ki_ori[:]), kp_f=np.array(cfg.kp_force[:]), kv_f=np.array(cfg.kv_force[:]),
                 ki_f=np.array(cfg.ki_force[:]), kp_m=np.array(cfg.kp_moment[:]), kv_m=np.array(cfg.kv_moment[:]),
                 ki_m=np.array(cfg.ki_moment[:]), kff_f=float(cfg.kff_force), kff_m=float(cfg.kff_moment),
                 max_f=float(cfg.max_force_feedback), max_m=float(cfg.max_moment_feedback),
                 lin_vsat=float(cfg.linear_saturation_velocity), ang_vsat=float(cfg.angular_saturation_velocity),
                 sensor_rot=np.array(cfg.sensor_rot[:]), sensor_pos=np.array(cfg.sensor_pos[:]))
    return out


def truth_tasks(cell):
    import sai2_primitives_perso_amd as pkg

    c = ff.CELLS[cell]
    _, links = product_model(c["robot"])
    cfgs = ff.configs(cell, pkg.joint_task_config, pkg.motion_force_task_config, links)
    return config_tasks(cfgs, hierarchy(c["hier"], cfgs[0].robot_dof))


def candidates(cell, count):
    """make_hp_golden.candidates plus the wrenches of the MotionForceTask (from a generator of their own)"""
    qs, dq, goals = mg.candidates(cell, count, ff.CELLS)
    rng = np.random.default_rng([4321, len(cell), sum(map(ord, cell))])
    for g in goals:
        if "pos" in g:
            g.update(f=mg._grid(rng.normal(0, 4.0, (3, count)), 14), m=mg._grid(rng.normal(0, 0.4, (3, count)), 14),
                     sf=mg._grid(rng.normal(0, 4.0, (3, count)), 14), sm=mg._grid(rng.normal(0, 0.4, (3, count)), 14))
    return qs, dq, goals


def near_threshold(tasks, info, q, model):
    if mg.near_threshold(tasks, info, q, model):
        return True
    close = lambda v, thr: abs(float(v) / float(thr) - 1) < mg.BAND_TOL
    return any(close(v, thr) for inf in info for v, thr in inf.get("norms", []) + inf.get("jt_des", []))


def evaluate(args):
    """the exact ticks of one robot: None when it sits on a threshold"""
    cell, tasks, qs, dq, goals, b, dps = args
    hp.mp.dps = dps
    model = mg.model_of(ff.CELLS[cell]["robot"])
    state = hp.new_state(model, tasks)
    t = next(i for i, x in enumerate(tasks) if x["kind"] == "mft")
    rows = []
    for k in range(qs.shape[0]):
        before = hp.copy.deepcopy(state)
        tau, info, kin = hp.tick(model, tasks, state, qs[k], dq, goals)
        if near_threshold(tasks, info, qs[k], model) or not np.isfinite(float(hp.norm_inf(tau))):
            return None
        kap, kap_i = (hp.kappa_emp(model, tasks, before, qs[k], dq, goals, tau, info, kin, seed=[b, k], integ=True)
                      if dps == 40 else (0.0, [0.0] * 5))
        inf = info[t]
        ratio = np.zeros(6)
        ratio[: len(inf["ratios"])] = [float(x) for x in inf["ratios"]]
        groups = hp.integ_groups(tasks, info)
        rows.append(dict(tau=np.array([float(x) for x in tau]), ratio=ratio, alpha=float(inf["alpha"]), nsing=inf["sc"],
                         c1=inf["c1"], c2=inf["c2"], types=(inf["types"] + [0, 0])[:2], kappa=kap, clamped=inf.get("clamped", 0),
                         branch=inf.get("branch", 0), kappa_integ=np.array(kap_i), ff=inf["Ff_norm"],
                         mft_integ=np.array([float(x) for g in groups[:4] for x in g]), jt_integ=np.array([float(x) for x in groups[4]]),
                         sat_f=inf["sat_f"], sat_m=inf["sat_m"], sat_v=inf["sat_v"], sat_w=inf["sat_w"],
                         sat_jt=any(i.get("sat_jt", False) for i in info)))
    return rows


VECTORS = ("tau", "ratio", "types", "mft_integ", "jt_integ", "kappa_integ")
SCALARS = ("alpha", "nsing", "c1", "c2", "kappa", "clamped", "branch", "ff") + ff.SATS


def build_cell(cell, pool, dps=40):
    c = ff.CELLS[cell]
    tasks = truth_tasks(cell)
    B = c["B"]
    qs, dq, goals = candidates(cell, int(B * 1.25) + 8)
    jobs = [(cell, tasks, qs[:, :, b], dq[:, b], mg.robot_goals(goals, b), b, dps) for b in range(qs.shape[2])]
    res = pool.map(evaluate, jobs, chunksize=2)
    keep = [b for b, r in enumerate(res) if r is not None][:B]
    assert len(keep) == B, (cell, len(keep), B)
    data = {f"{cell}.q": qs[:, :, keep], f"{cell}.dq": dq[:, keep]}
    kinds = [t["kind"] for t in tasks]
    for t, g in enumerate(goals):
        for k, v in g.items():
            data[f"{cell}.{kinds[t]}{t}_{k}"] = np.ascontiguousarray(v[:, keep])
    rows = [res[b] for b in keep]
    T = c["ticks"]
    for key in VECTORS:
        data[f"{cell}.{key}"] = np.array([[np.asarray(r[k][key], dtype=float) for r in rows] for k in range(T)]).transpose(0, 2, 1).copy()
    for key in SCALARS:
        data[f"{cell}.{key}"] = np.array([[r[k][key] for r in rows] for k in range(T)], dtype=float)
    for key in ("kappa", "ratio", "kappa_integ", "ff"):  # (7 digits are plenty for a bound and a report)
        data[f"{cell}.{key}"] = np.float64(np.float32(data[f"{cell}.{key}"]))
    return data


def coverage(data):
    """what the fixture must exercise, over all cells: {name: count}"""
    cells = sorted({k.split(".")[0] for k in data})
    cov = dict(blend_ff=0, alpha0=0, type1=0, type2_ff=0, clamped=0, two=0, regular=0)
    cov.update({f"{s}_{x}": 0 for s in ff.SATS for x in ("on", "off")})
    for c in cells:
        a, ns, ty, f = data[f"{c}.alpha"], data[f"{c}.nsing"], data[f"{c}.types"], data[f"{c}.ff"]
        cov["blend_ff"] += int(((a > 0) & (a < 1) & (ns > 0) & (f > 0)).sum())
        cov["alpha0"] += int(((a == 0) & (ns > 0)).sum())
        cov["type1"] += int((ty == 1).sum())
        cov["type2_ff"] += int(((ty == 2).any(axis=1) & (f > 0)).sum())
        cov["clamped"] += int(((data[f"{c}.clamped"] > 0) & (a > 0) & (a < 1)).sum())
        cov["two"] += int((ns >= 2).sum())
        cov["regular"] += int((ns == 0).sum())
        opts = ff.CELLS[c]["opts"]
        mft = next(o for o, k in zip(opts, ff.kinds(c)) if k == "mft")
        has = dict(sat_f=mft.get("closed_loop_force"), sat_m=mft.get("closed_loop_moment"),
                   sat_v="velocity_saturation" in mft, sat_w="velocity_saturation" in mft,
                   sat_jt=any("velocity_saturation" in o for o, k in zip(opts, ff.kinds(c)) if k == "jt"))
        for s in ff.SATS:
            if has[s]:  # (inactive counts only where the law is on)
                cov[f"{s}_on"] += int((data[f"{c}.{s}"] > 0).sum())
                cov[f"{s}_off"] += int((data[f"{c}.{s}"] == 0).sum())
    return cov


def build(jobs=16, cells=None):
    ctx = multiprocessing.get_context("fork")
    data = {}
    with ctx.Pool(min(jobs, 16)) as pool:
        for cell in cells or ff.CELLS:
            data.update(build_cell(cell, pool))
            print(cell, "done", flush=True)
    if cells is None:
        cov = coverage(data)
        assert all(v > 0 for v in cov.values()), cov
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    blob = mg.serialise(build(a.jobs))
    if a.check:
        with open(ff.FIXTURE, "rb") as f:
            same = f.read() == blob
        print("fixture reproduced bit for bit" if same else "fixture DIFFERS from the committed file")
        sys.exit(0 if same else 1)
    with open(ff.FIXTURE, "wb") as f:
        f.write(blob)
    print(f"{os.path.relpath(ff.FIXTURE, ROOT)}: {len(blob)} bytes, coverage {coverage(np.load(ff.FIXTURE))}")


if __name__ == "__main__":
    main()
