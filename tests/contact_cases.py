"""Inputs of the contact tests (tests/test_contact_reference.py on the CPU, tests/test_gpu_contact.py on the GPU): robots,
states, contact points and one plane per robot, drawn so that roughly a third of the robots are clear of the surface, a
third touch with some points only (four-point case; with one point they are split between the other two) and a third with
all. Ranges: d in [0, 0.5] s/m, mu in [0, 0.8], v_eps = 1e-3 m/s, joint speeds N(0, 0.8^2), and k in [1e3, 2e3] N/m: narrowed
from [1e3, 2e4] until the one-ulp condition of tests/test_contact_reference.py holds for every robot at B = 200 and 4 099.
What limits it is not the spring but friction: below v_eps the regularised Coulomb term is a damper of mu f_n / v_eps
(up to 1.6e4 N s/m at 2e4 N/m and 1 mm depth), which the explicit velocity update amplifies on the light outer links of
planar_4r and six_r (one-ulp start -> 5e-10 rad/s at k <= 1e4, 4e-12 at k <= 2e3).
Stiff contact (k from 1e4 to 1e6 N/m) is tested against the 40-digit plant instead, under a bound that prices the stiffness:
tests/hp_plant_fixture.py, tests/test_hp_plant.py on the CPU and tests/test_gpu_hp_plant.py on the GPU."""
import zlib

import numpy as np

import hp_fixture
import sai2_primitives_perso_amd as pkg
from contact_reference import ContactReference

ROBOTS = ("panda", "planar_4r", "six_r", "sliding_base", "rprp_4")
K_RANGE, D_RANGE, MU_RANGE, V_EPS = (1e3, 2e3), (0.0, 0.5), (0.0, 0.8), 1e-3
PLATE = 0.04  # half side of the four-point plate (m)
PERIODS, SUBSTEPS, DT = 5, 3, 0.001


def points(n_points):
    """one probe tip, or the four corners of a plate, in the contact link's frame"""
    if n_points == 1:
        return np.array([[0.02, -0.01, 0.07]])
    return np.array([[PLATE, PLATE, 0.05], [-PLATE, PLATE, 0.05], [-PLATE, -PLATE, 0.05], [PLATE, -PLATE, 0.05]])


def model(robot):
    m, _ = pkg.model_from_urdf(hp_fixture.urdf_text(robot), is_file=False)
    return m


def draw(robot, B, n_points, seed=0, link=None):
    """-> dict model, link, points, q, dq, tau [n][B], rows [9][B]. link: the contact link (default: the last one); it is not
    part of the seed, so every link of a robot gets the same states, torques, normals and gains, the planes placed against
    its own points"""
    m = model(robot)
    n = int(m.dof)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), B, n_points, seed])
    lo, hi = np.array(m.q_lower[:n]), np.array(m.q_upper[:n])
    q = np.ascontiguousarray((lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, n))).T)
    dq = rng.normal(0, 0.8, (n, B))
    tau = rng.normal(0, 5, (n, B))
    link, pts = n - 1 if link is None else int(link), points(n_points)
    assert 0 <= link < n
    rows = np.zeros((9, B))
    nrm = rng.normal(size=(3, B))
    rows[3:6] = nrm / np.linalg.norm(nrm, axis=0)
    rows[6] = rng.uniform(*K_RANGE, B)
    rows[7] = rng.uniform(*D_RANGE, B)
    rows[8] = rng.uniform(*MU_RANGE, B)
    ref = ContactReference(m, B, link, pts, rows, V_EPS)
    x, _, _ = ref.point_kinematics(q, dq)
    s = np.sort(np.einsum("ib,kib->kb", rows[3:6], x), axis=0)  # heights of the points along each robot's normal
    third = rng.integers(0, 3, B)
    if n_points == 1:
        third[third == 1] = 2 * rng.integers(0, 2, np.count_nonzero(third == 1))
    c = np.where(third == 0, s[0] - rng.uniform(0.01, 0.05, B), s[-1] + rng.uniform(0.001, 0.008, B))
    if n_points > 1:
        j = rng.integers(0, n_points - 1, B)
        a, b = s[j, np.arange(B)], s[j + 1, np.arange(B)]
        c = np.where(third == 1, a + rng.uniform(0.2, 0.8, B) * (b - a), c)
    tang = rng.normal(size=(3, B))
    tang -= np.sum(tang * rows[3:6], axis=0) * rows[3:6]
    rows[0:3] = c * rows[3:6] + 0.3 * tang
    return dict(model=m, robot=robot, link=link, points=pts, q=q, dq=dq, tau=tau, rows=rows, third=third)


def reference_run(case, with_gravity, plant=None, q=None, dq=None, rows=None):
    """PERIODS periods of SUBSTEPS substeps under the case's torques -> the ContactReference at its final state"""
    B = case["q"].shape[1]
    ref = ContactReference(case["model"], B, case["link"], case["points"], case["rows"] if rows is None else rows, V_EPS, plant=plant)
    ref.set_state(case["q"] if q is None else q, case["dq"] if dq is None else dq)
    for _ in range(PERIODS):
        ref.step(case["tau"], DT, SUBSTEPS, with_gravity)
    return ref


def settle_count(case, run):
    """The count of robots in contact must not hang on a rounding: robots that end with a normal force below 1e-9 N (or a
    point within 1e-12 m of the surface) in the reference are drawn away from the surface, and the reference is run again.
    `run(case) -> ContactReference at the final state`. A condition on the inputs, not a tolerance."""
    for _ in range(4):
        ref = run(case)
        rep = ref.report()
        fn, depth = rep["normal_force"], rep["depth"][: len(case["points"])]
        marginal = ((fn > 0) & (fn < 1e-9)).any(axis=0) | (np.abs(depth) < 1e-12).any(axis=0)
        if not marginal.any():
            return ref
        case["rows"][0:3, marginal] -= 0.1 * case["rows"][3:6, marginal]
    raise AssertionError("robots at the edge of the surface remain after four redraws")
