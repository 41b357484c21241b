"""The exact plant of tests/hp_reference.py (plant_step, plant_report) and its fixture tests/golden/hp_plant.npz (CPU):
the fixture is small and complete, regenerating a robot of every cell reproduces its rows bit for bit, 40 and 60 digits
agree, the float64 references (ContactReference, JointDynamicsReference, ExternalWrenchReference, composed as
tests/test_gpu_external_wrench.py composes them) meet every bound of tests/hp_plant_fixture.py with every flag, counter
and steps row exact (this is where C_PLANT is calibrated: REFERENCE_WORST), and the bound has teeth: each of eleven errors
planted in the exact model is over it in a named cell and reproduces the exact answer bit for bit where it cannot matter."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import external_wrench_reference as wr  # noqa: E402
import hp_plant_fixture as hf  # noqa: E402
import hp_reference as hp  # noqa: E402
import make_hp_plant_golden as mg  # noqa: E402
import oracle_lib as ol  # noqa: E402
import payload_cases as pc  # noqa: E402
from contact_reference import ContactReference  # noqa: E402
from joint_dynamics_reference import JointDynamicsReference  # noqa: E402

C_PLANT = hf.C_PLANT
CELLS = list(hf.CELLS)


@pytest.fixture(scope="module")
def z():
    return np.load(hf.FIXTURE)


def test_the_fixture_is_small_and_complete(z):
    assert os.path.getsize(hf.FIXTURE) <= 551_000  # the cap tests/test_hp_dynamics.py applies to its fixture
    bodies = {c["kernel"].split("<")[0] for c in hf.CELLS.values()}
    assert bodies == {"sim_kernel", "sim_wrench_kernel", "sim_joint_kernel", "sim_joint_wrench_kernel"}
    for cell in CELLS:
        d = hf.load(cell, z)
        c = hf.CELLS[cell]
        assert d["q"].shape[1] == hf.B == 67, cell
        for k in ("q", "dq", "tau", "joint", "contact", "wrench", "stop_k"):
            if k in d:
                assert z[f"{cell}.{k}"].dtype == np.float32, (cell, k)
        assert ("joint" in d) == c["joint"] and ("contact" in d) == bool(c["contact"]) and ("wrench" in d) == bool(c["wrench"]), cell
        for name in ["p1.s_dq", "p2x3.s_q", "p2x3.s_dq"] + [f"p2x3.s_{check}" for check, _, _ in hf.checks(cell)]:
            assert z[f"{cell}.{name}"].dtype == np.float32 and np.isfinite(d[name]).all(), (cell, name)
        assert (d["p1.s_dq"] > 0).all() and (d["p2x3.s_q"] > 0).all() and (d["p2x3.s_dq"] > 0).all(), cell
        for _, key, _ in hf.checks(cell):
            assert np.isfinite(hf.answer(d, f"p2x3.{key}")).all(), (cell, key)
        # every flag is up on some robots and down on others where the cell has the feature
        flags = d["p2x3.flags"]
        for i, (f, on) in enumerate(zip(hf.FLAGS, (c["contact"], c["joint"], c["joint"], c["wrench"]))):
            assert (0 < flags[:, i].sum(axis=1)).all() and (flags[:, i].sum(axis=1) < hf.B).all() if on else not flags[:, i].any(), (cell, f)
    # a wrench expires: pushed in the first period of p2x3 and not in the second
    for cell in ("wrench_world_inner", "wrench_link_shared_sensor", "everything"):
        f = hf.load(cell, z)["p2x3.flags"]
        assert ((f[0, 3] == 1) & (f[1, 3] == 0)).any(), cell
    # the robot drawn touching and moving out of its surface has left it by the end of p2x3, in every cell with a contact
    for cell in CELLS:
        if hf.CELLS[cell]["contact"]:
            b = mg.edges_of(cell).index(("contact", "lift_off"))
            d = hf.load(cell, z)
            assert d["p2x3.flags"][1, 0, b] == 0 and not d["p2x3.normal_force"][:, b].any(), cell


def _rows_equal(cell, d, b, exact, sc):
    for k, v in exact.items():
        if k.startswith("p") and k != "p2x3.applied_torque":
            assert np.array_equal(v, d[k][..., b]), (cell, k)
    assert np.array_equal(exact["flags"], d["p2x3.flags"][..., b]), cell
    if hf.CELLS[cell]["wrench"]:
        assert np.array_equal(exact["steps"], d["p2x3.steps"][..., b], equal_nan=True), cell
    for k, v in sc.items():
        assert np.float32(v) == np.float32(d[k][b]), (cell, k)


def test_regeneration_reproduces_the_fixture(z):
    """one robot a cell (the last: a drawn one), every array of its row and its scales, from the generator itself"""
    for cell in CELLS:
        d = hf.load(cell, z)
        b = hf.B - 1
        exact, sc = mg.row_of(cell, mg.inputs_of(d, b), b)
        assert exact["ok"], cell
        _rows_equal(cell, d, b, exact, sc)


def test_40_and_60_digits_agree(z):
    """one robot a cell: every answer within 1e-30 of its scale's magnitude (the scale of the bound over eps)"""
    raw = lambda v: np.array(v, dtype=object)
    for cell in CELLS:
        d = hf.load(cell, z)
        b = len(mg.edges_of(cell))  # the first drawn robot
        inp = mg.inputs_of(d, b)
        try:
            hp.mp.dps = 40
            a40 = mg.run(cell, inp, b, conv=raw)
            hp.mp.dps = 60
            a60 = mg.run(cell, inp, b, conv=raw)
        finally:
            hp.mp.dps = 40
        blocks = [("p1.s_dq", "p1.dq", slice(None)), ("p2x3.s_q", "p2x3.q", slice(None)), ("p2x3.s_dq", "p2x3.dq", slice(None))]
        blocks += [(f"p2x3.s_{check}", f"p2x3.{key}", rows) for check, key, rows in hf.checks(cell)]
        for name, key, rows in blocks:
            diff = max([abs(x - y) for x, y in zip(np.ravel(a40[key][rows]), np.ravel(a60[key][rows]))])
            assert diff <= 1e-30 * d[name][b] / hf.EPS, (cell, key, float(diff))
        assert np.array_equal(a40["flags"], a60["flags"])


# ---- the float64 references ----

def reference_run(cell, d):
    """the float64 references on a cell -> {p1.dq, p2x3.q, p2x3.dq, status rows of p2x3, flags [2][4][B], steps [2][B]}"""
    c = hf.CELLS[cell]
    m, links = hf.product_model(cell, d)
    n, B = int(m.dof), hf.B
    cfgs = hf.task_configs(cell, links, ol.motion_force_task, ol.joint_task, n)
    o = ol.Oracle(m, cfgs, B, threads=8)
    q0, dq0, tau = (np.ascontiguousarray(d[k]) for k in ("q", "dq", "tau"))

    def build():
        plant = cref = wref = jd = None
        if c["payload"] is not None:
            mass, com, I = hf.payloads()
            text = hf.urdf_text(c["robot"])
            plant = pc.PayloadOracles([pc.urdf_with_payload(text, c["payload"], mass[k], com[:, k], I[:, k]) for k in range(hf.P)], cfgs, B)
        if c["contact"]:
            link, pts, rows, _ = hf.contact_args(cell, d, links)
            cref = ContactReference(m, B, link, pts, rows, hf.V_EPS, plant=None if (c["joint"] or c["wrench"]) else plant)
        if c["wrench"]:
            link, rows, point, frame, _ = hf.wrench_args(cell, d, links)
            wref = wr.ExternalWrenchReference(m, B, link, rows, point, wr.LINK if frame == "link" else wr.WORLD,
                                              plant=None if c["joint"] else plant, contact=cref)
        if c["joint"]:
            jd = JointDynamicsReference(m, B, d["joint"], d["stop_k"], hf.STOP_DAMPING, hf.FRICTION_EPS, plant=plant,
                                        contact=wr.Combined(wref) if wref is not None else cref)
        return cref, wref, jd

    def period(cref, wref, jd, sub):
        if jd is not None and wref is not None:
            wref.joint_step(jd, tau, hf.DT, sub, True)
        elif jd is not None:
            jd.step(tau, hf.DT, sub, True)
        elif wref is not None:
            wref.step(tau, hf.DT, sub, True)
        else:
            cref.step(tau, hf.DT, sub, True)
        return (jd or wref or cref).get_state()

    out = {}
    cref, wref, jd = build()
    (jd or wref or cref).set_state(q0, dq0)
    out["p1.q"], out["p1.dq"] = period(cref, wref, jd, 1)
    cref, wref, jd = build()
    (jd or wref or cref).set_state(q0, dq0)
    flags, steps = np.zeros((2, 4, B), dtype=np.uint8), []
    for p in range(2):
        q, dq = period(cref, wref, jd, 3)
        got = {}
        cs = c["contact"]["sensor"] if c["contact"] else -1
        ws = c["wrench"]["sensor"] if c["wrench"] else -1
        if cref is not None:
            rep = cref.report(sensor=(o, cs) if cs >= 0 else None)
            got.update(depth=rep["depth"], normal_force=rep["normal_force"], wrench_world=rep["wrench_world"])
            flags[p, 0] = (rep["normal_force"] > 0).any(axis=0)
            assert rep["robots_in_contact"] == flags[p, 0].sum()
            if cs >= 0:
                got[f"sensed{cs}"] = rep["sensed"]
        if jd is not None:
            rep = jd.report()
            got.update(applied_torque=rep["applied_torque"], stop_torque=rep["stop_torque"], dissipative_torque=rep["dissipative_torque"])
            flags[p, 1], flags[p, 2] = (rep["stop_torque"] != 0).any(axis=0), jd.saturated
            assert rep["robots_at_stop"] == flags[p, 1].sum() and rep["robots_saturated"] == flags[p, 2].sum()
        if wref is not None:
            rep = wref.report(sensor=(o, ws) if ws >= 0 else None, q=q, dq=dq)
            got.update(ext_wrench=rep["wrench_world"], ext_torque=rep["torque"])
            flags[p, 3] = wref.active & (wref.rows[0:6] != 0).any(axis=0)
            assert rep["robots_pushed"] == flags[p, 3].sum()
            steps.append(wref.rows[6].copy())
            if ws >= 0:
                got[f"sensed{ws}"] = got[f"sensed{ws}"] + rep["sensed"] if ws == cs else rep["sensed"]
    out.update({"p2x3.q": q, "p2x3.dq": dq, "status": got, "flags": flags, "steps": np.array(steps)})
    return out


def all_ratios(cell, d, res):
    """{variant/check: per-robot ratios} of a result laid out as reference_run's"""
    out = {f"p1/{k}": v for k, v in hf.state_ratios(res.get("p1.q"), res["p1.dq"], d, "p1").items()}
    out.update({f"p2x3/{k}": v for k, v in hf.state_ratios(res["p2x3.q"], res["p2x3.dq"], d, "p2x3").items()})
    out.update({f"p2x3/{k}": v for k, v in hf.status_ratios(cell, res["status"], d).items()})
    return out


@pytest.mark.parametrize("cell", CELLS)
def test_the_references_meet_the_exact_plant(cell, z):
    """every block within C_PLANT of its scale, every flag, counter and steps row exact; the worst ratio printed is the one
    hp_plant_fixture.REFERENCE_WORST records and C_PLANT is set from (at least 4 x the worst, and the worst at most 8)"""
    d = hf.load(cell, z)
    res = reference_run(cell, d)
    ratios = all_ratios(cell, d, res)
    worst = max(ratios, key=lambda k: ratios[k].max())
    print(f"{cell}: worst {ratios[worst].max():.3f} ({worst}, robot {int(np.argmax(ratios[worst]))}); "
          + ", ".join(f"{k} {v.max():.2f}" for k, v in ratios.items()))
    assert np.array_equal(res["flags"], d["p2x3.flags"]), cell
    if hf.CELLS[cell]["wrench"]:
        assert np.array_equal(res["steps"], d["p2x3.steps"], equal_nan=True), cell
    for k, r in ratios.items():
        assert r.max() <= C_PLANT, (cell, k, int(np.argmax(r)), r.max())
    assert ratios[worst].max() <= 8 and 4 * ratios[worst].max() <= C_PLANT, (cell, worst, ratios[worst].max())
    rec = hf.REFERENCE_WORST[cell]
    assert rec[1] == worst and abs(rec[0] - ratios[worst].max()) <= 0.05 * rec[0] + 0.01, (cell, rec, worst, ratios[worst].max())


# ---- planted errors ----

def _planted(cell, d, robots, hook):
    """the planted model's answers on the given robots, as a result of reference_run's layout, and the cell cut to them"""
    hp.HOOKS.clear()
    hp.HOOKS[hook] = True
    try:
        rows = [mg.run(cell, mg.inputs_of(d, b), b) for b in robots]
    finally:
        hp.HOOKS.clear()
    stack = lambda k: np.stack([r[k] for r in rows], axis=-1)
    res = {"p1.dq": stack("p1.dq"), "p2x3.q": stack("p2x3.q"), "p2x3.dq": stack("p2x3.dq"), "flags": stack("flags"),
           "status": {k[5:]: stack(k) for k in rows[0] if k.startswith("p2x3.") and k not in ("p2x3.q", "p2x3.dq")}}
    if hf.CELLS[cell]["wrench"]:
        res["steps"] = stack("steps")
    cut = {k: (v[..., robots] if v.ndim and v.shape[-1] == hf.B else v) for k, v in d.items()}
    return res, cut, rows


# (hook, the cell that catches it, a cell where it cannot matter). The three robots of the catching cell are the first
# three drawn ones (behind the edge robots) unless the error needs a condition, then the first three drawn ones with it.
PLANTED = [
    ("diss_explicit", "joint_all", "contact_far_stiff"),  # 1: friction and damping at the old velocity, on the right-hand side
    ("rhs_no_armature", "joint_all", "contact_far_stiff"),  # 2: M dq for (M + diag(a)) dq
    ("upper_stop_minus", "joint_all", "contact_far_stiff"),  # 3: the upper stop damped with (1 - c dq)
    ("contact_outboard", "contact_inner_prismatic", "contact_far_stiff"),  # 4: joints outboard of the contact link
    ("contact_pris_as_rev", "contact_inner_prismatic", "contact_far_stiff"),  # 5: a prismatic joint as revolute in J^T F
    ("friction_along_v", "contact_far_stiff", "joint_all"),  # 6: friction along v, not v_t
    ("moment_about_link_origin", "contact_far_stiff", "wrench_world_inner"),  # 7: the reported moment about the link origin
    ("couple_on_prismatic", "wrench_world_inner", "wrench_link_shared_sensor"),  # 8: M_w on a prismatic joint's axis
    ("wrench_frame_period_start", "wrench_link_shared_sensor", "wrench_world_inner"),  # 9: the link frame of the period's start
    ("wrench_never_expires", "everything", "joint_all"),  # 10: steps = 1 still acting in the second period
    ("shared_sensor_no_wrench_moment", "wrench_link_shared_sensor", "everything"),  # 11: the wrench's moment out of the shared sum
]


def _needs(hook, cell, d):
    """robots on which the error can show at all"""
    f = d["p2x3.flags"]
    if hook == "upper_stop_minus":  # beyond the upper stop at the start
        return (d["q"] > d["joint"][5]).any(axis=0)
    if hook in ("contact_outboard", "contact_pris_as_rev", "friction_along_v", "moment_about_link_origin"):  # touching at the end
        return f[1, 0] == 1
    if hook == "wrench_never_expires":  # steps = 1
        return d["wrench"][6] == 1
    if hook in ("couple_on_prismatic", "wrench_frame_period_start", "shared_sensor_no_wrench_moment"):  # pushed at the end
        return f[1, 3] == 1
    return np.ones(hf.B, dtype=bool)


@pytest.mark.parametrize("hook, cell, inert", PLANTED)
def test_planted_errors_are_rejected(hook, cell, inert, z):
    d = hf.load(cell, z)
    first = len(mg.edges_of(cell))
    robots = [b for b in range(first, hf.B) if _needs(hook, cell, d)[b]][:3]
    assert len(robots) == 3, (hook, cell, robots)
    res, cut, _ = _planted(cell, d, robots, hook)
    ratios = all_ratios(cell, cut, res)
    worst = max(ratios, key=lambda k: ratios[k].max())
    exact = (res["flags"] == cut["p2x3.flags"]).all() and (hook != "wrench_never_expires" or np.array_equal(res["steps"], cut["p2x3.steps"]))
    print(f"{hook} in {cell}, robots {robots}: worst {ratios[worst].max():.3g} ({worst}); flags and steps {'exact' if exact else 'differ'}")
    assert ratios[worst].max() > C_PLANT, (hook, cell, ratios[worst].max())
    # where it cannot matter: the exact answer, bit for bit
    di = hf.load(inert, z)
    b = len(mg.edges_of(inert))
    _, _, rows = _planted(inert, di, [b], hook)
    _rows_equal(inert, di, b, rows[0], {})
