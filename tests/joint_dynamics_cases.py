"""Inputs of the joint-dynamics tests (tests/test_joint_dynamics_reference.py on the CPU, tests/test_gpu_joint_dynamics.py on
the GPU). Per robot and joint: armature in [0, 0.2], damping in [0, 5], friction in [0, 2] with e = 1e-3, torque limits in
[5, 30] against commanded torques N(0, 20^2) (a good share saturates), limits pulled 0 to 0.05 inside the model's, a third
of the robots starting 5 to 30 mrad (mm for a prismatic joint) beyond a limit of one joint, stop stiffness per joint in
[2e3, 1e4], stop damping 0.5. No |tau_i| lies within 1e-6 of its limit (a condition on the inputs, enforced here)."""
import zlib

import numpy as np

import contact_cases as cc
from joint_dynamics_reference import JointDynamicsReference, NEUTRAL, ROWS

ROBOTS = ("panda", "planar_4r", "six_r", "sliding_base")
EFFECTS = ("armature", "damping", "friction", "torque_limit", "limits")
V_EPS, STOP_DAMPING, K_RANGE = 1e-3, 0.5, (2e3, 1e4)
PERIODS, SUBSTEPS, DT = 5, 3, 0.001

model = cc.model


def draw(robot, B, seed=0):
    """-> dict model, q, dq, tau [n][B], rows [6][n][B], stop_stiffness [n], beyond [B] (robots that start beyond a limit)"""
    m = model(robot)
    n = int(m.dof)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), B, seed, 7])
    mlo, mhi = np.array(m.q_lower[:n])[:, None], np.array(m.q_upper[:n])[:, None]
    rows = np.empty((6, n, B))
    rows[0] = rng.uniform(0, 0.2, (n, B))
    rows[1] = rng.uniform(0, 5, (n, B))
    rows[2] = rng.uniform(0, 2, (n, B))
    rows[3] = rng.uniform(5, 30, (n, B))
    rows[4] = mlo + rng.uniform(0, 0.05, (n, B))
    rows[5] = mhi - rng.uniform(0, 0.05, (n, B))
    lo, hi = rows[4], rows[5]
    q = lo + (hi - lo) * rng.uniform(0.2, 0.8, (n, B))
    beyond = push_beyond(q, rows, rng)
    dq = rng.normal(0, 0.8, (n, B))
    tau = rng.normal(0, 20, (n, B))
    near = np.abs(np.abs(tau) - rows[3]) < 1e-6
    tau[near] *= 0.5
    return dict(model=m, robot=robot, n=n, q=np.ascontiguousarray(q), dq=dq, tau=tau, rows=rows, stop_stiffness=rng.uniform(*K_RANGE, n),
                beyond=beyond)


def push_beyond(q, rows, rng):
    """a third of the robots: one joint 5 to 30 mrad beyond one of its limits rows[4], rows[5]; q is changed in place"""
    n, B = q.shape
    beyond = rng.integers(0, 3, B) == 0
    joint, upper, by = rng.integers(0, n, B), rng.integers(0, 2, B) == 1, rng.uniform(0.005, 0.03, B)
    for b in np.flatnonzero(beyond):
        q[joint[b], b] = rows[5][joint[b], b] + by[b] if upper[b] else rows[4][joint[b], b] - by[b]
    return beyond


def select(case, effect):
    """rows and stop stiffness with only `effect` of EFFECTS on (the others neutral), or everything for 'all'"""
    n, B = case["rows"].shape[1:]
    rows = np.empty_like(case["rows"])
    for r, name in enumerate(ROWS):
        on = effect == "all" or effect == name or (effect == "limits" and name in ("q_lower", "q_upper"))
        rows[r] = case["rows"][r] if on else NEUTRAL[name]
    k = case["stop_stiffness"] if effect in ("all", "limits") else np.zeros(n)
    return rows, k


def keywords(rows, k):
    """the arguments of Controller.set_joint_dynamics for rows [6][n][B] and stop stiffness k [n]"""
    kw = {name: np.ascontiguousarray(rows[r]) for r, name in enumerate(ROWS)}
    kw.update(stop_stiffness=k, stop_damping=STOP_DAMPING, friction_velocity_eps=V_EPS)
    return kw


def reference(case, rows, k, plant=None, contact=None):
    B = case["q"].shape[1]
    return JointDynamicsReference(case["model"], B, rows, k, STOP_DAMPING, V_EPS, plant=plant, contact=contact)


def reference_run(case, rows, k, with_gravity, plant=None, contact=None, q=None, dq=None, periods=PERIODS):
    """PERIODS periods of SUBSTEPS substeps under the case's torques -> the reference at its final state"""
    ref = reference(case, rows, k, plant, contact)
    ref.set_state(case["q"] if q is None else q, case["dq"] if dq is None else dq)
    for _ in range(periods):
        ref.step(case["tau"], DT, SUBSTEPS, with_gravity)
    return ref


def clear_of_stops(case, rows, q_final):
    """no final q_i within 1e-9 of a stop: a condition on the inputs (the count of robots at a stop must not hang on a rounding)"""
    return not ((np.abs(q_final - rows[4]) < 1e-9) | (np.abs(q_final - rows[5]) < 1e-9)).any()
