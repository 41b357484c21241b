"""Inputs of the inverse-kinematics tests (tests/test_ik_reference.py and tests/test_ik_law.py on the CPU, tests/test_gpu_ik.py on
the GPU): the four robots with a control frame each, record sets drawn with fixed seeds, and the packing of records for
tests/cpp/ik_driver.cpp. One table, so that the CPU files check the conditions (the reference converges, its share of exhausted
robots, the share of records without separation) of exactly what the GPU file runs, and the bound the CPU file measures is the one
the GPU file asserts.

A control frame is (URDF link name, position in that link, rotation in that link), as tests/ik_reference.py takes it."""
import zlib

import numpy as np

import collision_cases as cc
import sai2_primitives_perso_amd as pkg
from ik_reference import SEPARATION, IkReference, product_frame, rotation_exp

ROBOTS = cc.ROBOTS
BATCHES = (1, 63, 64, 65, 200)
PLANAR_AXES = 0b100011  # x, y, wz: the planar 4R moves in the x-y plane
# Agreement of q_out between implementations over a full near-seed solve, on robots whose weighted Jacobian keeps its smallest
# singular value >= SIGMA_MIN along the reference's path: measured on the CPU (tests/test_ik_law.py, g++ -O1 against numpy), worst
# 1.72e-12 (sliding base); the bound is ten times that (g++ and hipcc contract FMAs differently), floor 1e-12, never above 1e-9.
SIGMA_MIN = 0.05
Q_MEASURED_WORST = 1.72e-12
Q_BOUND = max(10 * Q_MEASURED_WORST, 1e-12)
assert Q_BOUND <= 1e-9
MAX_DROPPED = 0.02


def axes_of(robot):
    return PLANAR_AXES if robot == "planar_4r" else 63


def frame(robot):
    """the control frame of a robot's tests: on the last moving link, off its origin, turned for the 6R"""
    link = cc.moving_links(robot)[-1]
    rot = rotation_exp(np.array([[0.3, -0.2, 0.5]]))[0] if robot == "six_r" else None
    return link, (0.01, 0.02, 0.06), rot


def limits(robot):
    m = cc.model(robot)[0]
    n = int(m.dof)
    return np.array(m.q_lower[:n]), np.array(m.q_upper[:n])


_refs = {}


def reference(robot, **cfg):
    """IkReference of a robot at its control frame; axes default to the robot's"""
    cfg.setdefault("axes", axes_of(robot))
    key = (robot, tuple(sorted(cfg.items())))
    if key not in _refs:
        link, fp, fr = frame(robot)
        lo, hi = limits(robot)
        _refs[key] = IkReference(cc.model(robot)[2], link, fp, fr, lo, hi, **cfg)
    return _refs[key]


def task_configs(robot):
    """[MotionForceTask at the control frame, JointTask] for pkg.Controller, and the same for the oracle"""
    m, links, _ = cc.model(robot)
    n = int(m.dof)
    link, fp, fr = frame(robot)
    i, p, r = product_frame(pkg, links, link, fp, fr)
    return [pkg.motion_force_task_config("m", link=i, frame_pos=p, frame_rot=r, robot_dof=n), pkg.joint_task_config("j", robot_dof=n)]


def oracle(robot, B):
    import oracle_lib as ol

    m, links, _ = cc.model(robot)
    n = int(m.dof)
    link, fp, fr = frame(robot)
    i, p, r = product_frame(pkg, links, link, fp, fr)
    return ol.Oracle(m, [ol.motion_force_task("m", link=i, frame_pos=p, frame_rot=r, robot_dof=n)], B, threads=8)


def oracle_pose(robot, q):
    """x [3][B], R [B][3][3], J [B][6][n] of the control frame at q [n][B] by the CPU oracle"""
    n, B = q.shape
    o = oracle(robot, B)
    o.set_state(np.ascontiguousarray(q), np.zeros((n, B)))
    _, J, x, R = o.get_model(0)
    return x, R.T.reshape(B, 3, 3), np.transpose(J.reshape(6, n, B), (2, 0, 1))


def oracle_error(robot, goal_rows, q, axes=None):
    """pos, rot [B]: the selected components' norms of the law's error at q, the pose from the CPU oracle"""
    ref = reference(robot) if axes is None else reference(robot, axes=axes)
    x, R, _ = oracle_pose(robot, q)
    B = q.shape[1]
    e = ref.error(goal_rows[:3].T, goal_rows[3:12].T.reshape(B, 3, 3), x.T, R)
    _, ep, er = ref.norms(e)
    return ep, er


def _rng(robot, B, what, seed=0):
    return np.random.default_rng([zlib.crc32(robot.encode()), B, zlib.crc32(what.encode()), seed])


def near_seed(robot, B, seed=0, inner=0.9, near_limit=None, conditioned=True):
    """goals by the reference's FK of a q_t drawn in the inner 90 % of the limits, seeds q_t +- 0.3 rad (+- 0.05 m on a prismatic
    joint) -> dict goal [12][B], seed [n][B], q_t. near_limit: q_t within that many radians of a limit instead (each joint at its
    lower or its upper end). conditioned=False: the draws as they come, the near-singular records included (the 'raw' sets: held to
    the reference on flags, start and tolerance only)"""
    m = cc.model(robot)[0]
    n = int(m.dof)
    lo, hi = limits(robot)
    rng = _rng(robot, B, "near" if near_limit is None else "limit", seed)
    if near_limit is None:
        qt = lo[:, None] + (hi - lo)[:, None] * (0.5 + inner * (rng.random((n, B)) - 0.5))
    else:
        up = rng.random((n, B)) < 0.5
        off = near_limit * rng.random((n, B))
        qt = np.where(up, hi[:, None] - off, lo[:, None] + off)
    pert = np.array([0.05 if m.joint_type[i] else 0.3 for i in range(n)])
    s = np.clip(qt + pert[:, None] * (2 * rng.random((n, B)) - 1), lo[:, None], hi[:, None])
    ref = reference(robot)
    if near_limit is None and conditioned:
        # THE CONDITION ON THE INPUTS: the reference converges on every record within 40 iterations. About one q_t in a thousand
        # lies so close to a singular configuration (the 6R's elbow, the Panda's stretched arm) that the law needs more; such a
        # record is replaced by a fresh draw from the same distribution, until none is left.
        solver = reference(robot, **NEAR)
        todo = np.arange(B)
        while len(todo):
            out = solver.solve(ref.goal_rows(qt[:, todo]), s[:, todo])
            todo = todo[(out["flags"] & 1) == 0]
            qt[:, todo] = lo[:, None] + (hi - lo)[:, None] * (0.5 + inner * (rng.random((n, len(todo))) - 0.5))
            s[:, todo] = np.clip(qt[:, todo] + pert[:, None] * (2 * rng.random((n, len(todo))) - 1), lo[:, None], hi[:, None])
    return dict(goal=ref.goal_rows(qt), seed=np.ascontiguousarray(s), q_t=qt)


def far_seed(robot, B, seed=0):
    """goals as near_seed, seeds uniform in the limits"""
    lo, hi = limits(robot)
    case = near_seed(robot, B, seed)
    rng = _rng(robot, B, "far", seed)
    case["seed"] = np.ascontiguousarray(lo[:, None] + (hi - lo)[:, None] * rng.random((len(lo), B)))
    return case


def unreachable(robot, B):
    """goals 2 m beyond the workspace: the pose of q_t pushed 2 m past the arm's reach along its own direction from the base"""
    case = near_seed(robot, B, seed=7)
    g = case["goal"]
    reach = np.linalg.norm(g[:3], axis=0).max()
    d = g[:3] / np.linalg.norm(g[:3], axis=0)
    g[:3] = d * (reach + 2.0)
    if robot == "sliding_base":  # its prismatic base reaches along its axis: the goal leaves sideways as well
        g[:3] += 5.0
    return case


_solved = {}


def solved(robot, kind, B, **cfg):
    """(case, reference result) of a record set under a configuration, computed once and shared"""
    key = (robot, kind, B, tuple(sorted(cfg.items())))
    if key not in _solved:
        draw = dict(near=near_seed, far=far_seed, unreachable=unreachable, limit=lambda r, b: near_seed(r, b, near_limit=0.02),
                    raw=lambda r, b: near_seed(r, b, seed=21, conditioned=False))[kind]
        case = draw(robot, B)
        ref = reference(robot, **cfg)
        _solved[key] = (case, ref.solve(case["goal"], case["seed"], track_sigma=True))
    return _solved[key]


def separated(result):
    """the robots whose every decision is clear of its threshold; the share left out must stay under MAX_DROPPED"""
    ok = result["sep"] >= SEPARATION
    assert (~ok).mean() <= MAX_DROPPED, (~ok).mean()
    return ok


FAR = dict(max_iterations=100, restarts=8, seed=20261021)
NEAR = dict(max_iterations=40)


# ---- records for tests/cpp/ik_driver.cpp
INTS, IN, OUT = 19, 173, 14


def chain_constants(model):
    """E [dof][9], xyz [dof][3], joint types of a RobotModel: what sai2b_solve_ik copies into the law's block"""
    import urdf_np

    n = int(model.dof)
    E = np.array([urdf_np._rpy(list(model.joint_rpy[i])).reshape(9) for i in range(n)])
    return E, np.array([list(model.joint_xyz[i]) for i in range(n)]), np.array([model.joint_type[i] for i in range(n)])


def pack(robot, ref, goal, seed, rest=None, robots=None):
    """records of one configuration (an IkReference's cfg) for B robots -> (ints [B][INTS], values [B][IN])"""
    m, links, _ = cc.model(robot)
    n = int(m.dof)
    B = seed.shape[1]
    c = ref.cfg
    link, fp, fr = frame(robot)
    li, p, r = product_frame(pkg, links, link, fp, fr)
    E, xyz, jt = chain_constants(m)
    ints = np.zeros((B, INTS), dtype=np.int64)
    ints[:, 0:6] = n, li, c["max_iterations"], c["restarts"], int(c["use_limits"]), int(rest is not None)
    ints[:, 6:10] = c["seed"] & 0xFFFFFFFF, c["seed"] >> 32, c["first_robot"], c["draw_id"]
    ints[:, 10] = np.arange(B) if robots is None else robots
    ints[:, 11 : 11 + n] = jt
    v = np.zeros((B, IN))
    v[:, 0 : 9 * n], v[:, 72 : 72 + 3 * n] = E.reshape(-1), xyz.reshape(-1)
    v[:, 96 : 96 + n], v[:, 104 : 104 + n] = ref.lo, ref.hi
    v[:, 112:115], v[:, 115:124] = p, np.asarray(r).reshape(-1)
    v[:, 124:130], v[:, 130:136] = ref.w2, ref.sel
    v[:, 136:145] = [c[k] for k in ("tol_pos", "tol_rot", "mu0", "mu_min", "mu_max", "mu_down", "mu_up", "step_max", "rest_weight")]
    v[:, 145:157] = goal[:12].T
    if rest is not None:
        v[:, 157 : 157 + n] = rest.T
    v[:, 165 : 165 + n] = seed.T
    return (ints & 0xFFFFFFFF).astype(np.uint32).view(np.int32), v
