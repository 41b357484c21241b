"""Inputs of the external-wrench tests (tests/test_external_wrench_reference.py on the CPU, tests/test_gpu_external_wrench.py
on the GPU): the five robots of contact_cases.ROBOTS (prismatic joints below and above revolute ones), the states, torques
and 5 periods x 3 substeps of contact_cases.draw, per robot a force with |F_i| <= 30 N and a couple with |M_i| <= 5 N m at
point (0.02, -0.01, 0.07) of the last link or of one inner link, in the world frame or the link's.

One-ulp condition (tests/test_external_wrench_reference.py asserts it on every cell drawn here, 257 robots per cell): a
start state one ulp off ends within 8.9e-16 rad and 2.8e-13 rad/s, worst cell planar_4r; under a tenth of the bounds the GPU
tests hold the state to (1e-12 rad, 1e-10 rad/s), so these ranges stand."""
import zlib

import numpy as np

import contact_cases as cc
from external_wrench_reference import LINK, WORLD, ExternalWrenchReference

ROBOTS = cc.ROBOTS
F_MAX, M_MAX = 30.0, 5.0
POINT = (0.02, -0.01, 0.07)
PERIODS, SUBSTEPS, DT = cc.PERIODS, cc.SUBSTEPS, cc.DT
FRAMES = {"world": WORLD, "link": LINK}
# one inner link per robot (0-based moving link), chosen with joints of both types at or below it where the robot has both
INNER = {"panda": 3, "planar_4r": 1, "six_r": 2, "sliding_base": 4, "rprp_4": 2}

model = cc.model


def links(robot):
    """the last link and the robot's inner link"""
    return (int(model(robot).dof) - 1, INNER[robot])


def cells():
    """(robot, link, frame name) of every cell"""
    return [(r, l, f) for r in ROBOTS for l in links(r) for f in FRAMES]


def draw(robot, B, link=None, frame="world", seed=0):
    """-> dict model, robot, link, frame, point, q, dq, tau [n][B], rows [7][B] (steps = -1: pushed until changed). The link and
    the frame are not part of the seed: every cell of a robot gets the same states, torques, forces and moments"""
    base = cc.draw(robot, B, 1, seed=seed, link=link)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), B, seed, 11])
    rows = np.empty((7, B))
    rows[0:3] = rng.uniform(-F_MAX, F_MAX, (3, B))
    rows[3:6] = rng.uniform(-M_MAX, M_MAX, (3, B))
    rows[6] = -1.0
    return dict(model=base["model"], robot=robot, link=base["link"], frame=frame, point=POINT, q=base["q"], dq=base["dq"], tau=base["tau"],
                rows=rows, contact=base)


def reference(case, plant=None, contact=None, rows=None):
    B = case["q"].shape[1]
    return ExternalWrenchReference(case["model"], B, case["link"], case["rows"] if rows is None else rows, case["point"], FRAMES[case["frame"]],
                                   plant=plant, contact=contact)


def reference_run(case, with_gravity, plant=None, contact=None, q=None, dq=None, rows=None, periods=PERIODS):
    """PERIODS periods of SUBSTEPS substeps of the plain step under the case's torques -> the reference at its final state"""
    ref = reference(case, plant, contact, rows)
    ref.set_state(case["q"] if q is None else q, case["dq"] if dq is None else dq)
    for _ in range(periods):
        ref.step(case["tau"], DT, SUBSTEPS, with_gravity)
    return ref


def keywords(case, rows=None, sensor_task=-1):
    """the arguments of Controller.set_external_wrench for the case"""
    r = case["rows"] if rows is None else rows
    return dict(link=case["link"], force=np.ascontiguousarray(r[0:3]), moment=np.ascontiguousarray(r[3:6]), steps=np.ascontiguousarray(r[6]),
                point=case["point"], frame=case["frame"], sensor_task=sensor_task)
