"""The cells of the link sweep (tests/test_link_sweep_reference.py on the CPU, tests/test_gpu_link_sweep.py on the GPU): the
per-robot payload, the contact of the simulated plant and the force sensor it drives take a batch-uniform link index, and
the rest of the suite holds them at the last link only, where every select over that index falls through to its default.
Here the index is an inner link. One table, so that the CPU file checks the conditioning of exactly what the GPU file runs."""
import numpy as np

import contact_cases as cc
import joint_dynamics_cases as jc

# ---- payload (controller and plant)
PAYLOAD_B = 130  # two full wavefronts and a ragged third; 17 or 33 wavefronts with 8 or 16 lanes a robot
PANDA_PAYLOAD_LINKS = (0, 1, 2, 3, 4, 5)
# (robot, payload link) of the robots other than the Panda: the slide of sliding_base, the boom of stanford_6, ...
OTHER_PAYLOAD_CELLS = (("planar_4r", 0), ("planar_4r", 1), ("six_r", 2), ("sliding_base", 0), ("sliding_base", 4), ("stanford_6", 2),
                       ("slider_7", 3))
PLANT_PAYLOAD_CELLS = (("panda", 0), ("panda", 3), ("stanford_6", 2))
# the cells the oracle itself is held to the 40-digit sum over bodies at
ORACLE_CELLS = (("panda", 0), ("panda", 3), ("stanford_6", 2), ("sliding_base", 0))

# ---- contact
CONTACT_B = 200  # three full wavefronts and eight robots
# (robot, contact link); rprp_4 is R P R P: link 2 has a prismatic joint inboard and outboard of it
CONTACT_LINKS = (("panda", 0), ("panda", 3), ("panda", 5), ("planar_4r", 1), ("six_r", 2), ("sliding_base", 0), ("sliding_base", 4),
                 ("rprp_4", 1), ("rprp_4", 2))
CONTACT_CELLS = tuple((r, l, k) for r, l in CONTACT_LINKS for k in (1, 4))
# one inner link per robot for the kinematics of the reference against the independent numpy chain
KINEMATICS_LINKS = (("panda", 3), ("planar_4r", 1), ("six_r", 2), ("sliding_base", 4), ("rprp_4", 2))
# Panda, four points: (contact link, link of the sensor task's control frame; None: sensor_task = -1)
SENSOR_CELLS = ((6, 4), (3, 6), (3, None), (6, None))
# Panda, four points, B = 130 (the size of the test this follows): (plant payload link, contact link)
MIXED_B = 130
MIXED_CELLS = ((3, 6), (6, 3))
OBSERVE_CELL = ("panda", 3, 4)

# every (robot, contact link, points, B) a GPU test of the sweep draws from tests/contact_cases.py
DRAWN_CELLS = tuple(sorted({(r, l, k, CONTACT_B) for r, l, k in CONTACT_CELLS} | {("panda", c, 4, CONTACT_B) for c, _ in SENSOR_CELLS}
                           | {("panda", c, 4, MIXED_B) for _, c in MIXED_CELLS} | {OBSERVE_CELL + (CONTACT_B,)}))


def mixed_case(contact_link):
    """the inputs of the mixed-link cells, as tests/test_gpu_joint_dynamics.py::test_all_four_instantiations builds its own: the
    contact case's poses (its planes are placed against them), a third pushed beyond the joint limits, every effect on"""
    B = MIXED_B
    con = cc.draw("panda", B, 4, link=contact_link)
    case = jc.draw("panda", B)
    case["q"], case["dq"] = con["q"].copy(), con["dq"]
    jc.push_beyond(case["q"], case["rows"], np.random.default_rng(B + 4))
    rows, k = jc.select(case, "all")
    return con, case, rows, k


def sensor_tasks(mk_mft, mk_jt, link, n=7):
    """the hierarchy whose first task carries the sensor: control frame on `link`, the sensor frame rotated and offset from it"""
    mft = mk_mft("m", link=link, frame_pos=(0.01, 0.02, 0.06), robot_dof=n)
    a = 0.4
    mft.sensor_rot[:] = [np.cos(a), -np.sin(a), 0, np.sin(a), np.cos(a), 0, 0, 0, 1]
    mft.sensor_pos[:] = [0.0, 0.01, -0.03]
    return [mft, mk_jt("j", robot_dof=n)]
