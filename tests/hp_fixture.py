"""The cells of the exact-answer fixture tests/golden/hp_singular.npz (tests/golden/make_hp_golden.py writes it) and how a
controller is built and driven on one: numpy and the product's config helpers only (no mpmath), so the GPU tests can
use it. Every cell is a robot, its hierarchy with the options of tests/cases.py on each task, a number of ticks and of
robots (never a multiple of 64)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "hp_singular.npz")
PANDA_URDF = os.path.join(HERE, "golden", "urdf", "panda_arm.urdf")
FULL, IMPEDANCE = 0, 2  # enum sai2b_decoupling
# per cell: the robot, its hierarchy ([kind, ...] as test_gpu_robots._setup builds it), option dict of tests/cases.py for
# every task, ticks, robots
CELLS = {
    "panda_c3": dict(robot="panda", hier="c3", opts=[{}, {}], ticks=1, B=181),
    "panda_c3_full": dict(robot="panda", hier="c3", opts=[{"decoupling": FULL}, {"decoupling": FULL}], ticks=1, B=157),
    "panda_c3_impedance": dict(robot="panda", hier="c3", opts=[{"decoupling": IMPEDANCE}, {"decoupling": IMPEDANCE}], ticks=1,
                               B=157),
    "panda_c3_type1": dict(robot="panda", hier="c3", opts=[{"enforce_type_1": True}, {}], ticks=1, B=157),
    "panda_c3_seq": dict(robot="panda", hier="c3", opts=[{}, {}], ticks=3, B=157),
    "panda_c4": dict(robot="panda", hier="c4", opts=[{}, {}, {}], ticks=1, B=157),
    "planar_4r": dict(robot="planar_4r", hier="planar_4r", opts=[{}, {}], ticks=1, B=157),
    "six_r": dict(robot="six_r", hier="six_r", opts=[{}, {}], ticks=1, B=157),
    "six_r_mft6": dict(robot="six_r", hier="six_r_mft6", opts=[{}], ticks=1, B=157),
    "sliding_base": dict(robot="sliding_base", hier="sliding_base", opts=[{}, {}, {}], ticks=1, B=157),
}


def urdf_text(robot):
    if robot == "panda":
        with open(PANDA_URDF) as f:
            return f.read()
    import robots

    return robots.TEXT[robot]()


def hierarchy(name, n):
    """[(kind, link name, point in link, partial | selection)] in hierarchy order"""
    import sai2_primitives_perso_amd as pkg

    if name in ("c3", "c4"):
        mft = ("mft", "link7", tuple(pkg.workloads.EE_FRAME_POS), None if name == "c3" else (np.eye(3), np.zeros((0, 3))))
        if name == "c3":
            return [mft, ("jt", None)]
        sel = np.zeros((2, n))
        sel[0, 0] = sel[1, 6] = 1
        return [mft, ("jt", sel), ("jt", None)]
    import singular_poses as sp

    t = sp.TASKS[name]
    if name == "planar_4r":
        partial = (np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[0, 0, 1.0]]))
    elif name == "six_r":
        partial = (np.eye(3), np.zeros((0, 3)))
    else:
        partial = None
    mft = ("mft", t["link"], t["point"], partial)
    if name == "six_r_mft6":
        return [mft]
    if name == "sliding_base":
        sel = np.zeros((2, n))
        sel[0, 0] = sel[1, 7] = 1
        return [("jt", sel), mft, ("jt", None)]
    return [mft, ("jt", None)]


def product_model(robot):
    import sai2_primitives_perso_amd as pkg

    if robot == "panda":
        return pkg.panda_model(), None
    return pkg.model_from_urdf(urdf_text(robot), is_file=False)


def product_configs(cell, mk_jt, mk_mft, links=None, cells=None, apply_opts=None):
    """the task configs of a cell, built by the given helpers (the product's, or the oracle's) and the cell's options
    (cells, apply_opts: another table of cells and its way to apply options, tests/hp_force_fixture.py)"""
    import cases
    import sai2_primitives_perso_amd as pkg

    c = (cells or CELLS)[cell]
    n = 7 if c["robot"] == "panda" else {"planar_4r": 4, "six_r": 6, "sliding_base": 8}[c["robot"]]
    out = []
    for k, spec in enumerate(hierarchy(c["hier"], n)):
        if spec[0] == "jt":
            cfg = mk_jt(f"jt{k}", spec[1], robot_dof=n)
        elif c["robot"] == "panda":
            cfg = mk_mft(f"mft{k}", partial=spec[3], robot_dof=n)
        else:
            link, fp, fr = pkg.resolve_link_frame(links, spec[1], spec[2])
            cfg = mk_mft(f"mft{k}", link, fp, fr, spec[3], robot_dof=n)
        (apply_opts or cases.apply_opts)(cfg, c["opts"][k])
        out.append(cfg)
    return out


def load(cell, z=None, fixture=None):
    """the cell's arrays of the fixture, keys without the cell prefix"""
    z = np.load(fixture or FIXTURE) if z is None else z
    return {k.split(".", 1)[1]: z[k] for k in z.files if k.split(".", 1)[0] == cell}


def kinds(cell, cells=None):
    c = (cells or CELLS)[cell]
    n = 7 if c["robot"] == "panda" else {"planar_4r": 4, "six_r": 6, "sliding_base": 8}[c["robot"]]
    return [s[0] for s in hierarchy(c["hier"], n)]


def make(cell, mk_jt, mk_mft, make_ctrl, cells=None, fixture=None, apply_opts=None):
    """a controller (product or oracle, by the helpers given) for the cell's robots, goals loaded, nothing ticked"""
    import oracle_lib as ol

    c = (cells or CELLS)[cell]
    model, links = product_model(c["robot"])
    cfgs = product_configs(cell, mk_jt, mk_mft, links, cells, apply_opts)
    d = load(cell, fixture=fixture)
    B = d["dq"].shape[1]
    ctrl = make_ctrl(ol.panda_model() if c["robot"] == "panda" and mk_jt is ol.joint_task else model, cfgs, B)
    for t, k in enumerate(kinds(cell, cells)):
        if k == "mft":
            g = [d[f"mft{t}_{x}"] for x in ("pos", "rot", "v", "w", "a", "alpha")]
            ctrl.set_mft_goals(t, *[np.ascontiguousarray(a) for a in g])
        else:
            ctrl.set_jt_goals(t, *[np.ascontiguousarray(d[f"jt{t}_{x}"]) for x in ("q", "dq", "ddq")])
    return ctrl, d


def run(ctrl, cell, d, tick=None, cells=None, after=None):
    """the cell's ticks: per tick (tau, (singular directions, c1, c2) of the MotionForceTask); after(ctrl): called behind
    every tick, its result appended to that tick's tuple"""
    t = kinds(cell, cells).index("mft")
    out = []
    for k in range(d["q"].shape[0]):
        ctrl.set_state(np.ascontiguousarray(d["q"][k]), np.ascontiguousarray(d["dq"]))
        tau = ctrl.tick() if tick is None else tick(ctrl)
        if hasattr(ctrl, "get_mft_singularity_state"):
            state = ctrl.get_mft_singularity_state(t)
        else:  # the oracle: singular directions from its split, the counts of its history
            _, _, ro = ctrl.get_mft_singularity(t)
            _, c1, c2 = ctrl.get_mft_sh_state(t)
            state = (ctrl.tasks[t].pos_range + ctrl.tasks[t].ori_range - ro, c1, c2)
        out.append((tau, tuple(np.asarray(s).astype(int) for s in state)) + (() if after is None else (after(ctrl),)))
    return out


def rel_err(tau, ref):
    """per robot ||tau - ref||_inf / max(||ref||_inf, 1) (arrays [n][B])"""
    return np.abs(tau - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def ratio_to_bound(tau, d, k):
    """per robot: the error of tick k in units of eps * kappa_emp"""
    return rel_err(tau, d["tau"][k]) / (np.finfo(float).eps * d["kappa"][k])


def bookkeeping_mismatch(state, d, k):
    """robots whose singular directions, c1 or c2 differ from the exact answer"""
    n, c1, c2 = state
    return np.flatnonzero((n != d["nsing"][k]) | (c1 != d["c1"][k]) | (c2 != d["c2"][k]))
