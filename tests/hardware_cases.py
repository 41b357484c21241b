"""Inputs of the hardware tests (tests/test_gpu_hardware.py): the 4-, 7- and 8-joint robots of the external-wrench tests with
their states, torques, contacts and wrenches (external_wrench_cases.draw), the per-robot actuator and sensor rows of each
effect, and a command that changes from period to period (the case's torques scaled per period and joint, inside the range
the one-ulp condition of external_wrench_cases was taken on: a constant command would hide a delay and a lag)."""
import zlib

import numpy as np

import external_wrench_cases as wc
import hardware_reference as hr

ROBOTS = ("planar_4r", "panda", "sliding_base")  # 4, 7 and 8 joints
BATCHES = (1, 5, 200, 4099)
PERIODS, SUBSTEPS, DT = wc.PERIODS, wc.SUBSTEPS, wc.DT
EFFECTS = ("lag", "gain", "noise", "all")
DEPTH = 3  # D of the "all" rows
SEED = 20261020

model = wc.model


def rows(robot, B, effect, sensor=False, depth=DEPTH):
    """-> (max_delay, actuator_rows, sensor_rows) with only `effect` on (delay: d cycling 0..depth over the batch; 'all': delay,
    lag, gain and noise together); sensor: bias, noise and filter on as well"""
    n = int(model(robot).dof)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), B, 23])
    act, sen = hr.ideal_rows(n, B)
    lag, gain, noise = rng.uniform(0.2, 0.9, (n, B)), rng.uniform(0.9, 1.1, (n, B)), rng.uniform(0.05, 0.5, (n, B))
    D = depth if effect in ("delay", "all") else 0
    if D:
        act[0] = np.arange(B) % (D + 1)
    if effect in ("lag", "all"):
        act[1 : 1 + n] = lag
    if effect in ("gain", "all"):
        act[1 + n : 1 + 2 * n] = gain
    if effect in ("noise", "all"):
        act[1 + 2 * n :] = noise
        act[1 + 2 * n, ::3] = 0.0  # some robots without noise on a joint, inside a wavefront that draws
    if sensor:
        sen[0:3], sen[3:6] = rng.uniform(-2, 2, (3, B)), rng.uniform(-0.2, 0.2, (3, B))
        sen[6:9], sen[9:12] = rng.uniform(0.05, 0.5, (3, B)), rng.uniform(0.005, 0.05, (3, B))
        sen[12] = rng.uniform(0.2, 1.0, B)
        sen[12, ::4] = 1.0
    return D, act, sen


def commands(case, periods=PERIODS):
    """[periods][n][B]: the case's torques scaled by a factor in [-1, 1] per period and joint"""
    n = case["tau"].shape[0]
    rng = np.random.default_rng([n, case["tau"].shape[1], 29])
    return case["tau"][None] * rng.uniform(-1.0, 1.0, (periods, n, 1))
