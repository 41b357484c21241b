"""The cells of the exact-answer fixture tests/golden/hp_force.npz (tests/golden/make_hp_force_golden.py writes it): the
force, integral and saturation laws of the MotionForceTask and the JointTask on the robots and hierarchies of
tests/hp_fixture.py, in and around the singularity-blending region. numpy and the product's config helpers only (no
mpmath), so the GPU tests can use it. hp_fixture.CELLS stays as it is; its helpers are used with this table. B is
never a multiple of 64 and spans two wavefronts (79-103 robots: what keeps the file under the size limit of a fixture).

A cell's options are those of tests/cases.py plus, for what that table has no name for: per-axis gains (a 3-vector where
cases.py takes a scalar), "gains_force" / "gains_moment" ((kp, kv, ki), scalars), "kff" ((force, moment)),
"max_feedback" ((force, moment)), "sensor" ((rotation 3x3, position)) and "ki" of a JointTask as (first, step)."""
import json
import os

import numpy as np

import hp_fixture as hf

FIXTURE = os.path.join(hf.HERE, "golden", "hp_force.npz")
# generic axes of unit length (0.36^2 + 0.48^2 + 0.8^2 = 1): no world axis is orthogonal to either
AXIS_A, AXIS_B = (0.36, -0.48, 0.8), (-0.6, 0.64, 0.48)


def _rot(c, s, axis):
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


# the sensor frame in the control frame: turned about z then x (Pythagorean angles), 6 cm off the control point
SENSOR = (_rot(0.6, 0.8, 2) @ _rot(0.28, 0.96, 0), (0.03, -0.02, 0.05))
_CLOSED = dict(closed_loop_force=True, closed_loop_moment=True, passivity=False, gains_force=(0.7, 10.0, 1.3),
               gains_moment=(0.9, 8.0, 1.1), kff=(0.95, 0.8))
_JT_PI_VSAT = {"ki": (3.0, 0.25), "velocity_saturation": 0.5}
CELLS = {
    "panda_c3_open": dict(robot="panda", hier="c3", ticks=1, B=103, opts=[
        dict(force_space_dimension=1, force_axis=(0, 0, 1), moment_space_dimension=2, moment_axis=(1, 0, 0)), {}]),
    "panda_c3_closed": dict(robot="panda", hier="c3", ticks=3, B=89, opts=[
        dict(_CLOSED, force_space_dimension=2, force_axis=AXIS_A, moment_space_dimension=1, moment_axis=AXIS_B,
             in_compliant_frame=True, sensor=SENSOR, max_feedback=(3.0, 0.3)), {}]),
    # closed-loop force in all three directions: no position space; the moment space is open loop, so that its
    # feed-forward is scaled by kff_moment under the *force* flag alone
    "panda_c3_force3": dict(robot="panda", hier="c3", ticks=2, B=83, opts=[
        dict(_CLOSED, force_space_dimension=3, moment_space_dimension=1, moment_axis=AXIS_B, closed_loop_moment=False,
             kff=(0.9, 0.5), max_feedback=(6.0, 10.0)), {}]),
    "panda_c3_pi_vsat": dict(robot="panda", hier="c3", ticks=3, B=87, opts=[
        dict(kp_pos=(100.0, 120.0, 80.0), kv_pos=(20.0, 0.0, 18.0), ki_pos=(4.0, 5.0, 6.0), kp_ori=(200.0, 150.0, 180.0),
             kv_ori=(28.0, 25.0, 30.0), ki_ori=(2.0, 2.5, 3.0), velocity_saturation=(0.2, 0.6)), _JT_PI_VSAT]),
    "panda_c4_force": dict(robot="panda", hier="c4", ticks=2, B=79, opts=[
        dict(_CLOSED, force_space_dimension=1, force_axis=AXIS_A, max_feedback=(3.0, 10.0)), {}, {}]),
    "six_r_mft6_force": dict(robot="six_r", hier="six_r_mft6", ticks=2, B=83, opts=[
        dict(_CLOSED, force_space_dimension=1, force_axis=AXIS_A, moment_space_dimension=1, moment_axis=AXIS_B,
             in_compliant_frame=True, sensor=SENSOR, max_feedback=(3.0, 0.3))]),
    "sliding_base_force": dict(robot="sliding_base", hier="sliding_base", ticks=1, B=89, opts=[
        {"velocity_saturation": 0.5}, dict(force_space_dimension=2, force_axis=AXIS_A, velocity_saturation=(0.2, 0.6)),
        {"velocity_saturation": 0.5}]),
    "planar_4r_force": dict(robot="planar_4r", hier="planar_4r", ticks=2, B=101, opts=[
        dict(_CLOSED, force_space_dimension=1, force_axis=(0.6, 0.8, 0), max_feedback=(3.0, 10.0)), {}]),
}
WRENCH = ("f", "m", "sf", "sm")
SATS = ("sat_f", "sat_m", "sat_v", "sat_w", "sat_jt")
INTEG_GROUPS = ("pos", "ori", "force", "moment", "jt")  # the rows of kappa_integ


def apply_opts(cfg, opts):
    import cases
    import sai2_primitives_perso_amd as pkg

    rest = {}
    for k, v in (opts or {}).items():
        mft = cfg.type == pkg.MOTION_FORCE_TASK
        if k in ("kp_pos", "kv_pos", "ki_pos", "kp_ori", "kv_ori", "ki_ori") and np.ndim(v) == 1:
            for i in range(3):
                getattr(cfg, k)[i] = v[i]
        elif k in ("gains_force", "gains_moment"):
            for name, x in zip(("kp", "kv", "ki"), v):
                for i in range(3):
                    getattr(cfg, f"{name}_{k[6:]}")[i] = x
        elif k == "kff":
            cfg.kff_force, cfg.kff_moment = v
        elif k == "max_feedback":
            cfg.max_force_feedback, cfg.max_moment_feedback = v
        elif k == "sensor":
            for i in range(9):
                cfg.sensor_rot[i] = np.asarray(v[0]).ravel()[i]
            for i in range(3):
                cfg.sensor_pos[i] = v[1][i]
        elif k == "ki" and not mft:
            for i in range(cfg.task_dof):
                cfg.ki[i] = v[0] + v[1] * i
        else:
            rest[k] = v
    return cases.apply_opts(cfg, rest)


def load(cell, z=None):
    return hf.load(cell, z, FIXTURE)


def kinds(cell):
    return hf.kinds(cell, CELLS)


def configs(cell, mk_jt, mk_mft, links=None):
    return hf.product_configs(cell, mk_jt, mk_mft, links, CELLS, apply_opts)


def make(cell, mk_jt, mk_mft, make_ctrl):
    """a controller (product or oracle) for the cell's robots: goals, goal wrench and sensed wrench loaded"""
    ctrl, d = hf.make(cell, mk_jt, mk_mft, make_ctrl, CELLS, FIXTURE, apply_opts)
    t = kinds(cell).index("mft")
    f, m, sf, sm = (np.ascontiguousarray(d[f"mft{t}_{k}"]) for k in WRENCH)
    ctrl.set_mft_goal_wrench(t, f, m)
    ctrl.set_mft_sensed_wrench(t, sf, sm)
    return ctrl, d


def integrators(ctrl, cell):
    """(MotionForceTask [12][B], all JointTasks' [k][B] in hierarchy order) as tests/plumbing.integrators reads them"""
    import plumbing

    ks = kinds(cell)
    rows = plumbing.integrators(ctrl, [(k, None) for k in ks])
    return rows[ks.index("mft")].copy(), np.concatenate([r for k, r in zip(ks, rows) if k == "jt"] or [np.zeros((0, ctrl.B))])


def run(ctrl, cell, d, tick=None):
    """the cell's ticks: per tick (tau, (singular directions, c1, c2), (MotionForceTask, JointTask integrators))"""
    return hf.run(ctrl, cell, d, tick, CELLS, lambda c: integrators(c, cell))


def integ_ratio(integ, d, k):
    """per group of INTEG_GROUPS and robot: the error of the integrators after tick k in units of eps * kappa_integ
    (0 where both the error and kappa_integ are 0)"""
    mft, jt = integ
    eps = np.finfo(float).eps
    out = np.zeros((5, mft.shape[1]))
    for g in range(5):
        got, ref = (mft[3 * g: 3 * g + 3], d["mft_integ"][k][3 * g: 3 * g + 3]) if g < 4 else (jt, d["jt_integ"][k])
        if ref.shape[0] == 0:
            continue
        err = np.abs(got - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)
        bound = eps * d["kappa_integ"][k][g]
        out[g] = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(float).tiny))
    return out


def report(update, key=None):
    """SAI2B_HP_REPORT=<file>: merge `update` into the JSON the file holds (under `key` when given)"""
    path = os.environ.get("SAI2B_HP_REPORT")
    if not path:
        return
    rep = {}
    if os.path.exists(path):
        with open(path) as f:
            rep = json.load(f)
    (rep.setdefault(key, {}) if key else rep).update(update)
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
