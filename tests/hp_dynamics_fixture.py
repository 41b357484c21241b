"""The cells of the exact-dynamics fixture tests/golden/hp_dynamics.npz (tests/golden/make_hp_dynamics_golden.py writes
it) and the bounds a simulation step and a bias vector are held to: numpy and the product's helpers only (no mpmath),
so the GPU test can use it.

89 robots a dynamics cell, 97 a tick cell (two wavefronts, the second partial): exact float64 answers do not compress, and 9 dynamics cells of
12 such arrays at 150 robots would weigh 0.9 MB. For the same reason two answers are derived rather than stored, each
to within an ulp: b with gravity = b0 + g, and after one substep q = q0 + dt dq (exactly so in real arithmetic).

Dynamics cells: one robot (optionally on a base transform, stored in the fixture), B robots (never a multiple of 64).
Tick cells: a robot with a prismatic joint inside the chain and its hierarchy (the one tests/test_gpu_robots.py runs),
gravity compensation on, regular poses only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "hp_dynamics.npz")
EPS = np.finfo(float).eps
DT = 1e-3
# the three simulation variants of every dynamics cell: (name, substeps, with gravity, periods)
SIMS = (("sim1", 1, True, 1), ("sim3", 3, False, 1), ("sim5x2", 2, True, 5))


def _tilt():
    a = np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.array([0.4, -0.2, 0.35]), np.eye(3) + np.sin(0.8) * K + (1 - np.cos(0.8)) * K @ K


DYN_CELLS = {
    "panda": dict(robot="panda", base=None, B=89),
    "panda_tilted": dict(robot="panda", base=_tilt, B=89),
    "sliding_base": dict(robot="sliding_base", base=None, B=89),
    "planar_4r": dict(robot="planar_4r", base=None, B=89),
    "six_r": dict(robot="six_r", base=None, B=89),
    "rprp_4": dict(robot="rprp_4", base=None, B=89),
    "stanford_6": dict(robot="stanford_6", base=None, B=89),
    "slider_7": dict(robot="slider_7", base=None, B=89),
    # a 90 degree pitch: the base orientation folded into the first joint's rpy sits on the gimbal lock
    "stanford_6_pitch90": dict(robot="stanford_6", base=lambda: (np.array([0.1, -0.2, 0.5]), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])),
                               B=89),
}
TICK_CELLS = {"rprp_4_tick": dict(robot="rprp_4", B=97), "stanford_6_tick": dict(robot="stanford_6", B=97),
              "slider_7_tick": dict(robot="slider_7", B=97)}
NEW_ROBOTS = ("rprp_4", "stanford_6", "slider_7")


def urdf_text(robot):
    import hp_fixture

    return hp_fixture.urdf_text(robot)


def hierarchy(robot, n):
    """[(kind, link, point in link, partial | selection)]: a position MotionForceTask and the JointTask behind it; on
    slider_7 the three levels of C4 (position MotionForceTask, JointTask on the first and last joints, full JointTask)"""
    if robot == "rprp_4":
        return [("mft", "link4", (0.05, 0.0, 0.02), (np.eye(3), np.zeros((0, 3)))), ("jt", None)]
    if robot == "stanford_6":
        return [("mft", "link6", (0.05, 0.0, 0.02), (np.eye(3), np.zeros((0, 3)))), ("jt", None)]
    assert robot == "slider_7"
    sel = np.zeros((2, n))
    sel[0, 0] = sel[1, n - 1] = 1
    return [("mft", "link7", (0.0, 0.0, 0.1), (np.eye(3), np.zeros((0, 3)))), ("jt", sel), ("jt", None)]


def configs(robot, mk_jt, mk_mft, links, n):
    """the task configs of a tick cell, built by the given helpers (the product's, or the oracle's)"""
    import sai2_primitives_perso_amd as pkg

    out = []
    for k, spec in enumerate(hierarchy(robot, n)):
        if spec[0] == "jt":
            out.append(mk_jt(f"jt{k}", spec[1], robot_dof=n))
        else:
            link, fp, fr = pkg.resolve_link_frame(links, spec[1], spec[2])
            out.append(mk_mft(f"mft{k}", link, fp, fr, spec[3], robot_dof=n))
    return out


def load(cell, z=None):
    """the cell's arrays of the fixture, keys without the cell prefix (the float32 scales as float64)"""
    z = np.load(FIXTURE) if z is None else z
    return {k.split(".", 1)[1]: z[k].astype(float) for k in z.files if k.split(".", 1)[0] == cell}


def product_model(cell, d):
    """the product's model of a cell, its base transform applied from the fixture's own numbers"""
    import sai2_primitives_perso_amd as pkg

    robot = (DYN_CELLS.get(cell) or TICK_CELLS[cell])["robot"]
    m, links = (pkg.panda_model(), None) if robot == "panda" else pkg.model_from_urdf(urdf_text(robot), is_file=False)
    if "base_pos" in d:
        m = pkg.with_base_transform(m, d["base_pos"], d["base_rot"])
    return m, links


# ---- bounds (calibrated on the CPU oracle: tests/test_hp_dynamics.py) ----

# The bounds the CPU oracle and every GPU kernel are held to (measured on the oracle, worst robot of every cell):
# bias ||b - b*||_inf <= C_BIAS eps beta: worst 7.7 (rprp_4, gravity), 5.3 on the tilted Panda, 1.6 - 5.1 elsewhere
C_BIAS = 32
# a simulated state, in units of sim_ratio's scale: worst 0.38 (every dynamics cell), 0.43 on the tick cells
C_SIM = 16
# the MotionForceTask's frame: ||x - x*||_inf, ||R - R*||_max <= C_POSE eps max(||x*||_inf, 1), and its velocity
# ||J dq - (J dq)*||_inf <= C_POSE eps max(||(J dq)*||_inf, ||dq||_inf): worst 2.5 (rprp_4, R)
C_POSE = 16
# the control tick, in units of eps kappa_emp, the C of tests/test_hp_reference.py and test_gpu_hp_singular.C_ROUTE:
# worst 1.6 (rprp_4), 0.50 (slider_7), 0.44 (stanford_6)
C_TICK = 128


def answer(d, key):
    """a stored exact answer, or one of the two derived ones (bg, sim1.q)"""
    if key == "bg":
        return d["b0"] + d["g"]
    if key == "sim1.q":
        return d["q"] + DT * d["sim1.dq"]
    return d[key]


def bias_ratio(b, ref, beta):
    """per robot ||b - b*||_inf / (eps beta)"""
    return np.abs(b - ref).max(axis=0) / (EPS * beta)


def sim_ratio(q, dq, d, name, dtau=None):
    """per robot: the error of a simulated state to the exact one, in units of its scale
    eps (S ||q|| + h S ||dq|| + h^2 S X) for q and eps (S ||dq|| + h S X) for dq, S the number of semi-implicit steps,
    h the step, X = max over the steps of cond_2(M) ||M^-1 (tau - b)||_inf + ||M^-1||_2 beta (what one ulp of M and of b
    do to the acceleration). dtau: an error of the torques on top ([n][B]), priced at h sqrt(n) ||M^-1||_2 ||dtau||."""
    sub, periods = d[f"{name}.steps"]
    S, h = sub * periods, DT / sub
    q0, dq0, q1, dq1 = d["q"], d["dq"], answer(d, f"{name}.q"), d[f"{name}.dq"]
    nq = np.maximum(np.abs(q0).max(axis=0), np.abs(q1).max(axis=0))
    ndq = np.maximum(np.abs(dq0).max(axis=0), np.abs(dq1).max(axis=0))
    X = d[f"{name}.xscale"].astype(float)
    extra = 0.0
    if dtau is not None:
        extra = 2 * h * np.sqrt(q0.shape[0]) * d[f"{name}.minv"] * np.abs(dtau).max(axis=0)
    sdq = EPS * (S * ndq + h * S * X)
    sq = EPS * (S * nq + h * S * ndq + h * h * S * X)
    rdq = np.maximum(np.abs(dq - dq1).max(axis=0) - S * extra, 0) / sdq
    rq = np.maximum(np.abs(q - q1).max(axis=0) - S * h * extra, 0) / sq
    return np.maximum(rq, rdq)


# ---- driving a controller (the oracle, or the product) on a cell ----

def simulate(ctrl, d, name):
    """the variant `name` of SIMS from the cell's inputs, through ctrl.sim_step: the state after it"""
    sub, periods = (int(x) for x in d[f"{name}.steps"])
    grav = next(g for nm, _, g, _ in SIMS if nm == name)
    ctrl.set_state(np.ascontiguousarray(d["q"]), np.ascontiguousarray(d["dq"]))
    for _ in range(periods):
        ctrl.sim_step(np.ascontiguousarray(d["tau"]), DT, sub, with_gravity=grav)
    return ctrl.get_state()


def dynamics_ratios(ctrl, d, gravity=True):
    """{check: per-robot ratio to its bound} of a controller (oracle or product) on a dynamics cell"""
    ctrl.set_state(np.ascontiguousarray(d["q"]), np.ascontiguousarray(d["dq"]))
    out = dict(bias0=bias_ratio(ctrl.get_bias(False), d["b0"], d["beta0"]),
               biasg=bias_ratio(ctrl.get_bias(True), answer(d, "bg"), d["betag"]))
    if gravity:
        out["gravity"] = bias_ratio(ctrl.get_gravity(), d["g"], d["betag"])
    for name, *_ in SIMS:
        q, dq = simulate(ctrl, d, name)
        out[name] = sim_ratio(q, dq, d, name)
    return out


def bound(check):
    return C_TICK if check == "tau" else C_POSE if check in ("x", "R", "v") else C_BIAS if check.startswith(("bias", "gravity")) else C_SIM


def tick_controller(cell, d, mk_jt, mk_mft, make_ctrl):
    """a controller for a tick cell, gravity compensation on, state and goals loaded"""
    import sai2_primitives_perso_amd as pkg

    robot = TICK_CELLS[cell]["robot"]
    m, links = pkg.model_from_urdf(urdf_text(robot), is_file=False)
    n, B = m.dof, d["dq"].shape[1]
    cfgs = configs(robot, mk_jt, mk_mft, links, n)
    ctrl = make_ctrl(m, cfgs, B)
    ctrl.enable_gravity_compensation(True)
    ctrl.set_state(np.ascontiguousarray(d["q"]), np.ascontiguousarray(d["dq"]))
    for t, spec in enumerate(hierarchy(robot, n)):
        if spec[0] == "mft":
            ctrl.set_mft_goals(t, *[np.ascontiguousarray(d[f"mft{t}_{x}"]) for x in ("pos", "rot", "v", "w", "a", "alpha")])
        else:
            ctrl.set_jt_goals(t, *[np.ascontiguousarray(d[f"jt{t}_{x}"]) for x in ("q", "dq", "ddq")])
    return ctrl


def tick_ratio(tau, d):
    return np.abs(tau - d["tau"]).max(axis=0) / np.maximum(np.abs(d["tau"]).max(axis=0), 1.0) / (EPS * d["kappa"])


def pose_ratios(pos, rot, d, v=None, w=None):
    sx = EPS * np.maximum(np.abs(d["x"]).max(axis=0), 1.0)
    out = dict(x=np.abs(pos - d["x"]).max(axis=0) / sx, R=np.abs(rot - d["R"]).max(axis=0) / sx)
    if v is not None:
        ref = np.vstack([d["v"], d["w"]])
        sv = EPS * np.maximum(np.abs(ref).max(axis=0), np.abs(d["dq"]).max(axis=0))
        out["v"] = np.abs(np.vstack([v, w]) - ref).max(axis=0) / sv
    return out
