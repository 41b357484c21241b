#!/usr/bin/env python3
"""Generates tests/golden/hp_singular.npz: robots in and around the singularity-blending region of a MotionForceTask,
with the exact answer of their control tick from the 40-digit restatement tests/hp_reference.py, for the Panda
hierarchies C3 (full decoupling, BIE, impedance, enforce_type_1, a 3-tick sequence) and C4, and the hierarchies of
tests/singular_poses.py on the robots of tests/robots.py.

Per cell <c> the fixture holds, [C][B] as every other fixture (B robots, T ticks):
  <c>.q [T][n][B], <c>.dq [n][B]; <c>.mft<t>_{pos,rot,v,w,a,alpha}, <c>.jt<t>_{q,dq,ddq}: the inputs
  <c>.tau [T][n][B]: the exact torques rounded to float64
  <c>.ratio [T][6][B]: s_i / s_0 of J N_prec; <c>.alpha, <c>.nsing, <c>.c1, <c>.c2 [T][B]; <c>.types [T][2][B] (0: none)
  <c>.kappa [T][B]: the empirical condition number hp_reference.kappa_emp; <c>.clamped [T][B]: tau_s components
  clamped to the effort limit; <c>.branch [T][B]: the joint-space torque of the singular directions (1: type 1, 2: type 2)
The inputs are drawn on coarse binary grids (q 2^-30, goal poses 2^-22, velocities 2^-14) so the fixture compresses;
the ratios and kappa_emp are stored rounded to float32 (they are reported and bounded, never compared to rounding).

A pose within 1e-6 (relative) of a decision threshold of its tick is rejected and the next one taken: s_min, s_max
(every ratio the split reads), s_abs_tol, the type-1 tolerance on |d . u_s| of both perturbation signs, the type-2
joint-limit angle, and the range tolerance of a JointTask's range basis. Every robot then has one branch.

Run:  python tests/golden/make_hp_golden.py [--check] [--jobs 16]   (deterministic; --check rebuilds in memory and
compares with the committed file bit for bit)
"""
import argparse
import io
import multiprocessing
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import hp_reference as hp  # noqa: E402
from hp_fixture import CELLS, hierarchy, product_configs, product_model, urdf_text  # noqa: E402

BAND_TOL = 1e-6


def truth_tasks(cell):
    """the hierarchy as hp_reference takes it: the numbers of the product's own task configs, the frame as a URDF link
    and a point in it"""
    import sai2_primitives_perso_amd as pkg

    c = CELLS[cell]
    _, links = product_model(c["robot"])
    cfgs = product_configs(cell, pkg.joint_task_config, pkg.motion_force_task_config, links)
    return config_tasks(cfgs, hierarchy(c["hier"], cfgs[0].robot_dof))


def config_tasks(cfgs, specs, plain=True):
    """task configs and their hierarchy specs -> the tasks as hp_reference takes them. plain: the motion law alone, as
    this fixture has it (tests/golden/make_hp_force_golden.py adds the numbers of the rest)"""
    n = cfgs[0].robot_dof
    out = []
    for cfg, spec in zip(cfgs, specs):
        common = dict(decoupling=int(cfg.dynamic_decoupling_type), bie=float(cfg.bie_threshold))
        if spec[0] == "jt":
            k0 = cfg.task_dof
            assert not plain or (not any(cfg.ki[:k0]) and not cfg.use_velocity_saturation)
            out.append(dict(kind="jt", S=np.array(cfg.joint_selection[: k0 * n]).reshape(k0, n), kp=np.array(cfg.kp[:k0]),
                            kv=np.array(cfg.kv[:k0]), **common))
            continue
        assert not plain or (not any(cfg.ki_pos) and not any(cfg.ki_ori) and not cfg.use_velocity_saturation)
        assert not plain or (cfg.force_space_dimension == 0 and cfg.moment_space_dimension == 0)
        assert not cfg.use_internal_otg
        out.append(dict(kind="mft", link=spec[1], point=np.array(spec[2], dtype=float), frot=np.eye(3),
                        P=np.array(cfg.partial_projection[:]).reshape(6, 6), rank=cfg.pos_range + cfg.ori_range,
                        kp_pos=np.array(cfg.kp_pos[:]), kv_pos=np.array(cfg.kv_pos[:]), kp_ori=np.array(cfg.kp_ori[:]),
                        kv_ori=np.array(cfg.kv_ori[:]), s_min=cfg.s_min, s_max=cfg.s_max, s_abs_tol=cfg.s_abs_tol,
                        type1_tol=cfg.type_1_tol, t2_ratio=cfg.type_2_torque_ratio, t2_angle=cfg.type_2_angle_threshold,
                        perturb=cfg.perturb_step_size, buffer=cfg.sh_buffer_size, kp1=cfg.kp_type_1, kv1=cfg.kv_type_1,
                        kv2=cfg.kv_type_2, enforce_type_1=bool(cfg.enforce_type_1_strategy),
                        enforce_handling=bool(cfg.enforce_handling_strategy), sv_sign=int(cfg.singular_vector_sign), **common))
    return out


def _grid(x, bits):
    return np.round(np.asarray(x, dtype=float) * 2.0 ** bits) / 2.0 ** bits


def candidates(cell, count, cells=None):
    """poses and goals of `count` candidate robots, in order (deterministic)"""
    import sai2_primitives_perso_amd as pkg
    import urdf_np

    c = (cells or CELLS)[cell]
    rng = np.random.default_rng([1234, len(cell), sum(map(ord, cell))])
    chain = urdf_np.Chain(urdf_text(c["robot"]), is_file=False)
    n = chain.dof
    if c["robot"] == "panda":
        q = pkg.workloads.sample_poses(rng, count, singular_fraction=0.85).T
    else:
        import singular_poses as sp

        bands = sp.TASKS[c["hier"]]["bands"]
        per = -(-count // len(bands))
        pools = [sp.poses(c["hier"], b, per, seed=5) for b in bands]
        k = np.arange(count)
        q = np.empty((n, count))
        for i in range(len(bands)):
            sel = (k % len(bands)) == i
            q[:, sel] = pools[i][:, k[sel] // len(bands)]
    q = _grid(q, 30)
    dq = _grid(rng.normal(0, 0.3, (n, count)), 14)
    spec = hierarchy(c["hier"], n)
    goals = []
    for kind, *rest in spec:
        if kind == "jt":
            S = np.eye(n) if rest[0] is None else rest[0]
            k0 = S.shape[0]
            goals.append(dict(q=_grid(S @ q + rng.normal(0, 0.1, (k0, count)), 22), dq=_grid(rng.normal(0, 0.1, (k0, count)), 14),
                              ddq=_grid(rng.normal(0, 0.2, (k0, count)), 14)))
            continue
        link, point = rest[0], rest[1]
        pos, rot = np.empty((3, count)), np.empty((9, count))
        for b in range(count):
            _, x, R = chain.jacobian(q[:, b], link, point)
            ax = rng.normal(size=(1, 3))
            ax /= np.linalg.norm(ax)
            pos[:, b] = x + rng.uniform(-0.05, 0.05, 3)
            rot[:, b] = (R @ pkg.workloads._expmap(ax * rng.uniform(0, 0.2))[0]).ravel()
        goals.append(dict(pos=_grid(pos, 22), rot=_grid(rot, 22), v=_grid(rng.normal(0, 0.05, (3, count)), 14),
                          w=_grid(rng.normal(0, 0.05, (3, count)), 14), a=_grid(rng.normal(0, 0.1, (3, count)), 14),
                          alpha=_grid(rng.normal(0, 0.1, (3, count)), 14)))
    qs = [q]
    for k in range(1, c["ticks"]):  # the sequence: q stepped a little along one direction per robot
        qs.append(_grid(q + k * 2e-3 * np.sign(rng.normal(size=(n, count))), 30))
    return np.array(qs), dq, goals


def robot_goals(goals, b):
    return [{k: v[:, b] for k, v in g.items()} for g in goals]


_MODELS = {}


def model_of(robot):
    if robot not in _MODELS:
        _MODELS[robot] = hp.Model(urdf_text(robot))
    return _MODELS[robot]


def near_threshold(tasks, info, q, model):
    """the robot's tick is within BAND_TOL (relative) of a decision"""
    close = lambda v, thr: abs(float(v) / thr - 1) < BAND_TOL
    for t, inf in zip(tasks, info):
        if t["kind"] == "jt":
            if any(close(r, 1e-3) for r in inf["range_ratio"]):
                return True
            continue
        r = inf["ratios"]
        if close(inf["s0"], t["s_abs_tol"]):
            return True
        if any(close(x, t["s_min"]) or close(x, t["s_max"]) for x in r[1: t["rank"]]):
            return True
        if any(close(x, t["type1_tol"]) for x in inf["d1"]):
            return True
        for i in range(model.dof):
            for lim in (model.lower[i], model.upper[i]):
                if close(abs(q[i] - lim), t["t2_angle"]):
                    return True
    return False


def evaluate(args):
    """the exact ticks of one robot: None when it sits on a threshold"""
    cell, tasks, qs, dq, goals, b, dps = args
    hp.mp.dps = dps
    model = model_of(CELLS[cell]["robot"])
    state = hp.new_state(model, tasks)
    rows = []
    for k in range(qs.shape[0]):
        before = hp.copy.deepcopy(state)
        tau, info, kin = hp.tick(model, tasks, state, qs[k], dq, goals)
        if near_threshold(tasks, info, qs[k], model) or not np.isfinite(float(hp.norm_inf(tau))):
            return None
        kap = hp.kappa_emp(model, tasks, before, qs[k], dq, goals, tau, info, kin, seed=[b, k]) if dps == 40 else 0.0
        t = next(i for i, x in enumerate(tasks) if x["kind"] == "mft")
        inf = info[t]
        ratio = np.zeros(6)
        ratio[: len(inf["ratios"])] = [float(x) for x in inf["ratios"]]
        types = (inf["types"] + [0, 0])[:2]
        rows.append(dict(tau=np.array([float(x) for x in tau]), ratio=ratio, alpha=float(inf["alpha"]), nsing=inf["sc"],
                         c1=inf["c1"], c2=inf["c2"], types=types, kappa=kap, clamped=inf.get("clamped", 0),
                         branch=inf.get("branch", 0)))
    return rows


def build_cell(cell, pool, dps=40):
    c = CELLS[cell]
    tasks = truth_tasks(cell)
    B = c["B"]
    qs, dq, goals = candidates(cell, int(B * 1.25) + 8)
    jobs = [(cell, tasks, qs[:, :, b], dq[:, b], robot_goals(goals, b), b, dps) for b in range(qs.shape[2])]
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
    for key in ("tau", "ratio", "types"):
        data[f"{cell}.{key}"] = np.array([[np.asarray(r[k][key], dtype=float) for r in rows] for k in range(T)]).transpose(0, 2, 1).copy()
    for key in ("alpha", "nsing", "c1", "c2", "kappa", "clamped", "branch"):
        data[f"{cell}.{key}"] = np.array([[r[k][key] for r in rows] for k in range(T)], dtype=float)
    for key in ("kappa", "ratio"):  # (7 digits are plenty for a bound and a report)
        data[f"{cell}.{key}"] = np.float64(np.float32(data[f"{cell}.{key}"]))
    return data


def coverage(data):
    """what the fixture must exercise, over all cells: {name: count}"""
    cells = sorted({k.split(".")[0] for k in data})
    cov = dict(blend=0, alpha0=0, type1=0, type2=0, clamped=0, two=0, regular=0)
    for c in cells:
        a, ns, ty = data[f"{c}.alpha"], data[f"{c}.nsing"], data[f"{c}.types"]
        cov["blend"] += int(((a > 0) & (a < 1) & (ns > 0)).sum())
        cov["alpha0"] += int(((a == 0) & (ns > 0)).sum())
        cov["type1"] += int((ty == 1).sum())
        cov["type2"] += int((ty == 2).sum())
        cov["clamped"] += int(((data[f"{c}.clamped"] > 0) & (a > 0) & (a < 1)).sum())
        cov["two"] += int((ns >= 2).sum())
        cov["regular"] += int((ns == 0).sum())
    return cov


def build(jobs=16, cells=None):
    ctx = multiprocessing.get_context("fork")
    data = {}
    with ctx.Pool(min(jobs, 16)) as pool:
        for cell in cells or CELLS:
            data.update(build_cell(cell, pool))
            print(cell, "done", flush=True)
    cov = coverage(data)
    assert all(v > 0 for v in cov.values()), cov
    return data


def serialise(data):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(data):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.ascontiguousarray(data[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, a.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    from hp_fixture import FIXTURE as OUT

    blob = serialise(build(a.jobs))
    if a.check:
        with open(OUT, "rb") as f:
            same = f.read() == blob
        print("fixture reproduced bit for bit" if same else "fixture DIFFERS from the committed file")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(blob)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(blob)} bytes, coverage {coverage(np.load(OUT))}")


if __name__ == "__main__":
    main()
