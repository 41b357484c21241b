"""The cells of the exact-plant fixture tests/golden/hp_plant.npz (tests/golden/make_hp_plant_golden.py writes it from
hp_reference.plant_step / plant_report) and the bound the simulated plant is held to: contact, joint dynamics, the external
wrench, the plant payload and the sensor rows, on all four written-out step bodies of csrc/sai2b_sim.hip. numpy and the
product's helpers only (no mpmath), so the GPU test can use it.

B = 67 robots a cell (one full wavefront and a ragged one). Inputs are values a float32 holds exactly and are stored as
float32; answers are float64, scales float32. Two variants: p1 (1 period of 1 substep: dq alone is stored, q = q0 + h dq)
and p2x3 (2 periods of 3 substeps: state, every status row, the sensed rows, per period the flags and the steps row).

The bound. Every checked block (CHECKS) has a per-robot scale: the largest change of that block, over 8 seeded runs of the
40-digit model, when every quantity a float64 implementation rounds is perturbed by a relative eps = 2^-52 (the state
entering every substep; world positions of contact points, control points and the bodies' centres of mass by eps of
their own size, and with them every lever arm x - p_i, in J_k, M and b alike; the point velocities, M, b by its sum of
absolute products, each torque term, the system matrix and the right-hand side by theirs, rotations by eps per entry), plus eps of the block's own size for the rounding of storing
it. Neither a kernel nor a float64 reference enters it. A block is within the bound when its error is at most C_PLANT
times that scale; a block whose scale is zero (a robot clear of the surface, inside its stops, not pushed) must be
exact. Flags, counters and the steps row are exact throughout: the generator redraws robots until no final |delta| is
under 1e-9 m, no final f_n in (0, 1e-6 N), no final q_i within 1e-9 of a stop and no |tau_i| within 1e-6 of its limit
without being exactly on it.

Stiffness. No cell had its stiffness narrowed: at k up to 1e6 N/m the float64 references stay under the bound and every
planted error of tests/test_hp_plant.py is over it (the scale prices the stiffness: it grows with k where the
references' errors do)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "hp_plant.npz")
EPS = np.finfo(float).eps
DT, B = 1e-3, 67
VARIANTS = (("p1", 1, 1), ("p2x3", 3, 2))  # name, substeps, periods
V_EPS, FRICTION_EPS, STOP_DAMPING = 1e-3, 1e-3, 0.5
PLATE = 0.04
FRAME_POINT = (0.01, 0.02, 0.06)  # the MotionForceTasks' control point, in the URDF frame of their link
SENSOR_POS = (0.0, 0.01, -0.03)
SENSOR_ROT = [np.cos(0.4), -np.sin(0.4), 0, np.sin(0.4), np.cos(0.4), 0, 0, 0, 1]
WRENCH_POINT = (0.02, -0.01, 0.07)
P = 16  # payloads: robot b carries payload b % 16
FLAGS = ("touching", "at_stop", "saturated", "pushed")

# the bound: every block within C_PLANT times its scale. Calibrated on the float64 references (ContactReference,
# JointDynamicsReference, ExternalWrenchReference composed as tests/test_gpu_external_wrench.py composes them) in
# tests/test_hp_plant.py::test_the_references_meet_the_exact_plant; the next power of two at least 4 x their worst.
# REFERENCE_WORST: their worst ratio per cell (over both variants and every check), with the check it came from.
C_PLANT = 16
REFERENCE_WORST = {  # (worst ratio, its check); 4 x 3.64 = 14.5 -> C_PLANT = 16
    "contact_far_stiff": (3.64, "p2x3/dq"),  # robot 1, the edge robot nearly at rest (|v_t| = 1e-3 v_eps); p1/dq 2.89
    "contact_inner_prismatic": (0.886, "p2x3/depth"),
    "joint_all": (0.801, "p2x3/stop_torque"),
    "joint_contact_8": (1.01, "p2x3/depth"),
    "joint_payload_contact": (1.02, "p2x3/contact_moment"),
    "wrench_world_inner": (0.989, "p2x3/ext_torque"),
    "wrench_link_shared_sensor": (1.48, "p2x3/sensed0_force"),
    "everything": (0.990, "p2x3/sensed0_force"),
}


def points(n_points):
    """one probe tip, or the four corners of a plate, in the URDF frame of the contact link"""
    if n_points == 1:
        return np.array([[0.02, -0.01, 0.07]])
    return np.array([[PLATE, PLATE, 0.05], [-PLATE, PLATE, 0.05], [-PLATE, -PLATE, 0.05], [PLATE, -PLATE, 0.05]])


def far_base():
    """a tilted base about 15 m from the world origin"""
    a = np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.array([9.0, -8.0, 9.0]), np.eye(3) + np.sin(0.8) * K + (1 - np.cos(0.8)) * K @ K


# links are 0-based moving links. tasks: the link of every MotionForceTask (a JointTask follows them); payload: the link
# of the plant's payload; contact: link, points, sensor task (-1: none), stiffness range (log-uniform); wrench: link,
# frame, sensor task. kernel: the body of csrc/sai2b_sim.hip the cell runs.
CELLS = {
    "contact_far_stiff": dict(robot="panda", base=far_base, kernel="sim_kernel<NoPayload, Contact>", tasks=[6], joint=False, payload=None,
                              contact=dict(link=6, n_points=4, sensor=0, k=(1e4, 1e6)), wrench=None),
    "contact_inner_prismatic": dict(robot="stanford_6", base=None, kernel="sim_kernel<Payload, Contact>", tasks=[5], joint=False, payload=4,
                                    contact=dict(link=3, n_points=1, sensor=0, k=(1e4, 1e6)), wrench=None),
    "joint_all": dict(robot="slider_7", base=None, kernel="sim_joint_kernel<NoPayload, NoContact>", tasks=[6], joint=True, payload=None,
                      contact=None, wrench=None),
    "joint_contact_8": dict(robot="sliding_base", base=None, kernel="sim_joint_kernel<NoPayload, Contact>", tasks=[7], joint=True, payload=None,
                            contact=dict(link=7, n_points=4, sensor=0, k=(1e4, 1e5)), wrench=None),
    "joint_payload_contact": dict(robot="six_r", base=None, kernel="sim_joint_kernel<Payload, Contact>", tasks=[5], joint=True, payload=5,
                                  contact=dict(link=5, n_points=1, sensor=-1, k=(1e4, 1e5)), wrench=None),
    "wrench_world_inner": dict(robot="rprp_4", base=None, kernel="sim_wrench_kernel<NoPayload, NoContact>", tasks=[2], joint=False, payload=None,
                               contact=None, wrench=dict(link=2, frame="world", sensor=0)),
    "wrench_link_shared_sensor": dict(robot="panda", base=None, kernel="sim_wrench_kernel<NoPayload, Contact>", tasks=[6], joint=False,
                                      payload=None, contact=dict(link=6, n_points=1, sensor=0, k=(1e4, 1e6)),
                                      wrench=dict(link=6, frame="link", sensor=0)),
    "everything": dict(robot="stanford_6", base=None, kernel="sim_joint_wrench_kernel<Payload, Contact>", tasks=[5, 3], joint=True, payload=4,
                       contact=dict(link=5, n_points=1, sensor=0, k=(1e4, 1e6)), wrench=dict(link=3, frame="link", sensor=1)),
}
JOINT_ROWS = ("armature", "damping", "friction", "torque_limit", "q_lower", "q_upper")


def link_name(robot, link):
    """URDF name of moving link `link` of the robots of tests/robots.py and of the Panda"""
    return f"link{link}" if robot == "sliding_base" else f"link{link + 1}"


def urdf_text(robot):
    import hp_fixture

    return hp_fixture.urdf_text(robot)


def payloads():
    """-> mass [16], com [3][16] (URDF link frame), inertia [6][16] (about the COM: xx yy zz xy xz yz); float32 values"""
    rng = np.random.default_rng(20261021)
    m, c, I = np.zeros(P), np.zeros((3, P)), np.zeros((6, P))
    m[1], c[:, 1] = 3.0, (0.2, 0.0, 0.05)
    for k in range(2, P):
        m[k] = rng.uniform(0.1, 3.0)
        v = rng.normal(size=3)
        c[:, k] = v / np.linalg.norm(v) * rng.uniform(0.02, 0.15)
        A = rng.normal(size=(3, 3))
        S = A @ A.T
        S *= rng.uniform(0.005, 0.05) / np.abs(S).max()
        I[:, k] = (S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2])
    f = lambda a: a.astype(np.float32).astype(float)
    return f(m), f(c), f(I)


def load(cell, z=None):
    """the cell's arrays of the fixture, keys without the cell prefix, everything as float64 but the flags"""
    z = np.load(FIXTURE) if z is None else z
    return {k.split(".", 1)[1]: (z[k] if z[k].dtype == np.uint8 else z[k].astype(float)) for k in z.files if k.split(".", 1)[0] == cell}


# ---- the checks and their ratios ----

def checks(cell):
    """[(check, answer key, row slice)] of the status and sensor blocks of a cell"""
    c = CELLS[cell]
    out = []
    if c["contact"]:
        out += [("depth", "depth", slice(None)), ("normal_force", "normal_force", slice(None)),
                ("contact_force", "wrench_world", slice(0, 3)), ("contact_moment", "wrench_world", slice(3, 6))]
    if c["joint"]:
        out += [("applied_torque", "applied_torque", slice(None)), ("stop_torque", "stop_torque", slice(None)),
                ("dissipative_torque", "dissipative_torque", slice(None))]
    if c["wrench"]:
        out += [("ext_force", "ext_wrench", slice(0, 3)), ("ext_moment", "ext_wrench", slice(3, 6)), ("ext_torque", "ext_torque", slice(None))]
    for t in sensor_tasks(cell):
        out += [(f"sensed{t}_force", f"sensed{t}", slice(0, 3)), (f"sensed{t}_moment", f"sensed{t}", slice(3, 6))]
    return out


def sensor_tasks(cell):
    c = CELLS[cell]
    return sorted({f["sensor"] for f in (c["contact"], c["wrench"]) if f and f["sensor"] >= 0})


def answer(d, key):
    """a stored exact answer, or one of the two derived ones: p1.q = q + h p1.dq, p2x3.applied_torque = the saturated tau"""
    if key == "p1.q":
        return d["q"] + DT * d["p1.dq"]
    if key == "p2x3.applied_torque":
        return np.minimum(np.maximum(d["tau"], -d["joint"][3]), d["joint"][3])
    return d[key]


def _ratio(err, scale):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / scale)


def state_ratios(q, dq, d, variant):
    """{q, dq: per robot, the error of a simulated state in units of its scale}. p1 stores no q: it is q0 + h dq, and its
    scale h s_dq + eps ||q||_inf (dq's own scale through the step, and the rounding of the sum); q None: not checked"""
    out = {"dq": _ratio(np.abs(dq - d[f"{variant}.dq"]).max(axis=0), d[f"{variant}.s_dq"])}
    if q is not None:
        ref = answer(d, f"{variant}.q")
        s = d[f"{variant}.s_q"] if variant != "p1" else DT * d["p1.s_dq"] + EPS * np.abs(ref).max(axis=0)
        out["q"] = _ratio(np.abs(q - ref).max(axis=0), s)
    return out


def status_ratios(cell, got, d):
    """got: {answer key: rows} of p2x3 (depth, normal_force, wrench_world, applied_torque, stop_torque, dissipative_torque,
    ext_wrench, ext_torque, sensed<t>) -> {check: per-robot ratio}"""
    out = {}
    for check, key, rows in checks(cell):
        ref = answer(d, f"p2x3.{key}")
        K = ref.shape[0]
        out[check] = _ratio(np.abs(got[key][:K][rows] - ref[rows]).max(axis=0), d[f"p2x3.s_{check}"])
    return out


def counters(d, period):
    """{flag: the exact count of robots} after period `period` of p2x3"""
    return {f: int(d["p2x3.flags"][period, i].sum()) for i, f in enumerate(FLAGS)}


# ---- building a plant (the product's controller, or the float64 references) on a cell ----

def product_model(cell, d):
    import sai2_primitives_perso_amd as pkg

    m, links = pkg.model_from_urdf(urdf_text(CELLS[cell]["robot"]), is_file=False)
    if "base_pos" in d:
        m = pkg.with_base_transform(m, d["base_pos"], d["base_rot"].reshape(3, 3))
    return m, links


def frame_of(links, robot, link, point=(0.0, 0.0, 0.0)):
    """a point of the URDF frame of moving link `link` -> (the point, the URDF frame's rotation) in the model's link frame"""
    import sai2_primitives_perso_amd as pkg

    idx, fp, fr = pkg.resolve_link_frame(links, link_name(robot, link), point)
    assert idx == link, (robot, link, idx)
    return fp, fr


def task_configs(cell, links, mk_mft, mk_jt, n):
    """a MotionForceTask with a sensor off its control point on every link of the cell's `tasks`, then a JointTask"""
    c = CELLS[cell]
    out = []
    for t, link in enumerate(c["tasks"]):
        fp, fr = frame_of(links, c["robot"], link, FRAME_POINT)
        cfg = mk_mft(f"m{t}", link, fp, fr, robot_dof=n)
        cfg.sensor_rot[:] = SENSOR_ROT
        cfg.sensor_pos[:] = SENSOR_POS
        out.append(cfg)
    return out + [mk_jt("j", robot_dof=n)]


def payload_rows(cell, links):
    """(link, mass [B], com [3][B], inertia [6][B]) of the plant payload in the model's link frame"""
    c = CELLS[cell]
    m, com, I6 = payloads()
    idx = np.arange(B) % P
    m, com, I6 = m[idx], com[:, idx], I6[:, idx]
    pos, R = frame_of(links, c["robot"], c["payload"])
    I = np.einsum("ij,jkb,lk->ilb", R, np.stack([I6[[0, 3, 4]], I6[[3, 1, 5]], I6[[4, 5, 2]]]), R)
    return (c["payload"], np.ascontiguousarray(m), np.ascontiguousarray(pos[:, None] + R @ com),
            np.ascontiguousarray(np.stack([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])))


def contact_args(cell, d, links):
    """(link, points [K][3] in the model's link frame, rows [9][B], sensor task)"""
    c = CELLS[cell]
    con = c["contact"]
    pts = np.array([frame_of(links, c["robot"], con["link"], p)[0] for p in points(con["n_points"])])
    return con["link"], pts, np.ascontiguousarray(d["contact"]), con["sensor"]


def wrench_args(cell, d, links):
    """(link, rows [7][B] with a link-frame wrench turned into the model's link frame, point there, frame, sensor task)"""
    c = CELLS[cell]
    w = c["wrench"]
    fp, fr = frame_of(links, c["robot"], w["link"], WRENCH_POINT)
    rows = np.array(d["wrench"])
    if w["frame"] == "link":
        rows[0:3], rows[3:6] = fr @ rows[0:3], fr @ rows[3:6]
    return w["link"], rows, fp, w["frame"], w["sensor"]


def joint_keywords(d):
    kw = {name: np.ascontiguousarray(d["joint"][r]) for r, name in enumerate(JOINT_ROWS)}
    kw.update(stop_stiffness=d["stop_k"], stop_damping=STOP_DAMPING, friction_velocity_eps=FRICTION_EPS)
    return kw


def controller(cell, d, on_device=None):
    """the product's controller of a cell with the cell's features set. on_device: a function numpy array -> device tensor,
    used for the wrench rows (a NaN in the steps row passes through device rows only) and the contact rows (a normal held by
    a float32 is a unit vector to 1e-8, host rows are refused beyond 1e-9; the law takes n as it is given)"""
    import sai2_primitives_perso_amd as pkg

    c = CELLS[cell]
    m, links = product_model(cell, d)
    n = int(m.dof)
    g = pkg.Controller(m, task_configs(cell, links, pkg.motion_force_task_config, pkg.joint_task_config, n), B)
    if c["payload"] is not None:
        link, mass, com, I6 = payload_rows(cell, links)
        g.set_link_payload(link, mass, com, I6, target="plant")
    if c["contact"]:
        link, pts, r, sensor = contact_args(cell, d, links)
        f = on_device or np.ascontiguousarray
        g.set_contact(link, pts, f(r[0:3]), f(r[3:6]), f(r[6]), f(r[7]), f(r[8]), sensor_task=sensor, friction_velocity_eps=V_EPS)
    if c["joint"]:
        g.set_joint_dynamics(**joint_keywords(d))
    if c["wrench"]:
        link, r, point, frame, sensor = wrench_args(cell, d, links)
        f = on_device or np.ascontiguousarray
        g.set_external_wrench(link, f(r[0:3]), f(r[3:6]), f(r[6]), point=tuple(point), frame=frame, sensor_task=sensor)
    return g


def run_p1(g, d):
    g.set_state(np.ascontiguousarray(d["q"]), np.ascontiguousarray(d["dq"]))
    g.sim_step(np.ascontiguousarray(d["tau"]), DT, 1, with_gravity=True)
    return g.get_state()
