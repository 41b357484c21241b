"""GPU tests (-m gpu) of the external wrench on a link of the simulated plant (csrc/sai2b_sim.hip: sim_wrench_kernel<PL, CT>,
sim_joint_wrench_kernel<PL, CT>) against tests/external_wrench_reference.py. Inputs: tests/external_wrench_cases.py (Panda,
planar_4r, six_r, sliding_base with its prismatic first joint, rprp_4 with prismatic joints inside the chain; the last and
one inner link; world and link frame), contact and joint-dynamics inputs from contact_cases / joint_dynamics_cases. B = 1,
63, 65, 130 per robot (a single robot, a ragged wavefront, a second workgroup with one robot, two and a bit) and one Panda
case of 4 099.

1: state after 5 periods of 3 substeps, every robot within the bounds tests/test_gpu_sim.py holds the plain harness to
   (1e-12 rad, 1e-10 rad/s). Per robot and B: the plain form with every (link, frame, gravity), and the other seven forms
   (plant payload x contact x joint dynamics) each on one (link, frame, gravity), so that every value of each meets forms
   of every kind over the parametrisation.
2: status rows, sensor rows (alone on the wrench link's task and on another link's, shared with the contact's sensor: the
   sum, the two on different tasks; every (robot, B) runs all four pairings with a contact, test_plan_covers_... holds the
   plan to that) and the counter of those runs against the reference evaluated at the state the GPU ended
   in (the evaluation rule of tests/test_gpu_contact.py), 1e-12 max(1, largest magnitude of the reference's rows); and through
   the controller: after the step and one tick get_mft_status gives -F_w and -(M_w + (x - x_c) x F_w), 1e-10.
3: countdown. 4: balance. 5: routing. 6: device rows. 7: argument checks. 8: the resident loop, pushed and released."""
import ctypes as C
import functools

import numpy as np
import pytest

import contact_cases as cc
import external_wrench_cases as wc
import external_wrench_reference as wr
import joint_dynamics_cases as jc
import oracle_lib as ol
import payload_cases as pc
import plumbing
import sai2_primitives_perso_amd as pkg
from contact_reference import ContactReference
from sai2_primitives_perso_amd import _abi

pytestmark = pytest.mark.gpu

FRAME_POS = (0.01, 0.02, 0.06)
SENSOR_POS = (0.0, 0.01, -0.03)
SENSOR_ROT = [np.cos(0.4), -np.sin(0.4), 0, np.sin(0.4), np.cos(0.4), 0, 0, 0, 1]
Q_TOL, V_TOL = 1e-12, 1e-10


def _tasks(mk_mft, mk_jt, link, other, n):
    """task 0: a MotionForceTask on `link` with a sensor off its control point; task 1: one on link `other`; task 2: a JointTask"""
    out = []
    for name, l in (("m", link), ("o", other)):
        mft = mk_mft(name, link=l, frame_pos=FRAME_POS, robot_dof=n)
        mft.sensor_rot[:] = SENSOR_ROT
        mft.sensor_pos[:] = SENSOR_POS
        out.append(mft)
    return out + [mk_jt("j", robot_dof=n)]


def _other(link, n):
    return link - 1 if link == n - 1 else n - 1


def _steps(g, case, grav, periods=wc.PERIODS):
    g.set_state(case["q"], case["dq"])
    for _ in range(periods):
        g.sim_step(case["tau"], wc.DT, wc.SUBSTEPS, grav)
    return g.get_state()


def _sensed(g, task):
    return plumbing.device_rows(g, _abi.BUF_SENSED, task, 6)


CELLS = [(l, f, g) for l in (0, 1) for f in ("world", "link") for g in (False, True)]  # l: index into wc.links(robot)
FORMS = [(p, c, j) for p in (False, True) for c in (False, True) for j in (False, True)]
# (contact's sensor task, wrench's sensor task) of the runs with a contact: shared (the sum), different tasks, one of the two alone
SENSORS = [(0, 0), (0, 1), (0, -1), (-1, 1)]


def _plan(robot, B):
    """[(payload, contact, joint dynamics, link index, frame, gravity, contact's sensor task, wrench's sensor task)]. The runs with
    a contact are counted on their own, so that the four of a (robot, B) take the four pairings of SENSORS, and the shift moves
    each pairing through the four forms with a contact over the parametrisation; the runs without one alternate the wrench's
    sensor between the task on its link and the task on another link"""
    if B > 1000:
        shift, runs = 3, [f + CELLS[(k + 3) % 8] for k, f in enumerate(FORMS)]
    else:
        shift = wc.ROBOTS.index(robot) + (1, 63, 65, 130).index(B)
        runs = [FORMS[0] + c for c in CELLS] + [f + CELLS[(k + shift) % 8] for k, f in enumerate(FORMS[1:])]
    out, with_contact, without = [], 0, 0
    for run in runs:
        if run[1]:
            out.append(run + SENSORS[(with_contact + shift) % 4])
            with_contact += 1
        else:
            out.append(run + (-1, without % 2))
            without += 1
    return out


@functools.lru_cache(maxsize=None)
def _run(robot, B):
    """-> [record] of every run of _plan: GPU state, status and sensor rows, and the reference's"""
    n = int(wc.model(robot).dof)
    out = []
    ctx = {}
    for payload, contact, joint, li, frame, grav, cs, ws in _plan(robot, B):
        link = wc.links(robot)[li]
        case = wc.draw(robot, B, link, frame)
        other = _other(link, n)
        if link not in ctx:
            ctx[link] = (pkg.Controller(case["model"], _tasks(pkg.motion_force_task_config, pkg.joint_task_config, link, other, n), B),
                         ol.Oracle(case["model"], _tasks(ol.motion_force_task, ol.joint_task, link, other, n), B, threads=8))
        g, o = ctx[link]
        con = case["contact"]
        r = con["rows"]
        # the GPU
        if payload:
            g.set_link_payload(link, *pc.model_rows(robot, link, *pc.rows(B)), target="plant")
        else:
            g.clear_link_payload("plant")
        if contact:
            g.set_contact(link, con["points"], r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=cs, friction_velocity_eps=cc.V_EPS)
        else:
            g.clear_contact()
        jcase = jc.draw(robot, B)
        jrows, jk = jc.select(jcase, "all")
        if joint:
            g.set_joint_dynamics(**jc.keywords(jrows, jk))
        else:
            g.clear_joint_dynamics()
        g.set_external_wrench(**wc.keywords(case, sensor_task=ws))
        q, dq = _steps(g, case, grav)
        got = g.get_external_wrench_state()
        got.update(q=q, dq=dq, count_only=g.robots_pushed(), steps=g.get_external_wrench()[1][6],
                   sensed={t: _sensed(g, t) for t in {cs, ws} if t >= 0})
        # the reference's own run
        plant = pc.PayloadOracles(pc.texts(robot, link), o.tasks, B) if payload else None
        cref = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS) if contact else None
        wref = wc.reference(case, plant=None if joint else plant, contact=cref)
        if joint:
            jd = jc.reference(case, jrows, jk, plant=plant, contact=wr.Combined(wref))
            jd.set_state(case["q"], case["dq"])
            for _ in range(wc.PERIODS):
                wref.joint_step(jd, case["tau"], wc.DT, wc.SUBSTEPS, grav)
            qr, dqr = jd.get_state()
        else:
            wref.set_state(case["q"], case["dq"])
            for _ in range(wc.PERIODS):
                wref.step(case["tau"], wc.DT, wc.SUBSTEPS, grav)
            qr, dqr = wref.get_state()
        # the reference's rows at the state the GPU ended in
        at = wc.reference(case)
        rep = {t: at.report(sensor=(o, t), q=q, dq=dq) for t in (0, 1)}
        want = dict(wrench_world=rep[0]["wrench_world"], torque=rep[0]["torque"], robots_pushed=rep[0]["robots_pushed"], q=qr, dq=dqr, sensed={})
        if ws >= 0:
            want["sensed"][ws] = rep[ws]["sensed"]
        if contact and cs >= 0:
            cat = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS)
            cat.set_state(q, dq)
            crows = cat.report(sensor=(o, cs))["sensed"]
            want["sensed"][cs] = crows + rep[cs]["sensed"] if cs == ws else crows
            want["contact_alone"] = crows
        out.append((dict(payload=payload, contact=contact, joint=joint, link=link, frame=frame, gravity=grav, sensors=(cs, ws)), got, want))
    return out


CASES = [(r, B) for r in wc.ROBOTS for B in (1, 63, 65, 130)] + [("panda", 4099)]


def test_plan_covers_every_form_cell_and_sensor_pairing():
    """what the docstring claims of the plan, held here: every (robot, B) runs all eight forms and, with a contact, all four
    sensor pairings; over the parametrisation the shared sensor (the sum) meets each of the four forms with a contact, every
    form meets both links, both frames and both gravities, and the wrench's sensor stands alone on either task"""
    shared, cells = set(), {f: set() for f in FORMS}
    for robot, B in CASES:
        plan = _plan(robot, B)
        assert {run[:3] for run in plan} == set(FORMS)
        assert sorted(run[6:] for run in plan if run[1]) == sorted(SENSORS)
        assert {run[6:] for run in plan if not run[1]} == {(-1, 0), (-1, 1)}
        if B < 1000:
            assert {run[3:6] for run in plan if run[:3] == FORMS[0]} == set(CELLS)
        for run in plan:
            cells[run[:3]].add(run[3:6])
            if run[6:] == (0, 0):
                shared.add((run[0], run[2]))
    assert shared == {(p, j) for p in (False, True) for j in (False, True)}
    for f, seen in cells.items():
        assert {c[0] for c in seen} == {0, 1} and {c[1] for c in seen} == {"world", "link"} and {c[2] for c in seen} == {False, True}, f


@pytest.mark.parametrize("robot, B", CASES)
def test_state_follows_the_reference(robot, B):
    for what, got, want in _run(robot, B):
        eq, ev = np.abs(got["q"] - want["q"]).max(), np.abs(got["dq"] - want["dq"]).max()
        print(f"1 {robot} B={B} {what}: |dq| {eq:.2e} |ddq| {ev:.2e}")
        assert eq < Q_TOL and ev < V_TOL, (what, eq, ev)


@pytest.mark.parametrize("robot, B", CASES)
def test_status_sensor_rows_and_counter(robot, B):
    for what, got, want in _run(robot, B):
        errs = {}
        for key in ("wrench_world", "torque"):
            errs[key] = (np.abs(got[key] - want[key]).max(), 1e-12 * max(1.0, np.abs(want[key]).max()))
        for t, rows in want["sensed"].items():
            errs[f"sensed[{t}]"] = (np.abs(got["sensed"][t] - rows).max(), 1e-12 * max(1.0, np.abs(rows).max()))
        print(f"2 {robot} B={B} {what}: {errs}")
        assert all(e < tol for e, tol in errs.values()), (what, errs)
        cs, ws = what["sensors"]
        if cs >= 0 and cs == ws and B >= 63:  # the shared sensor: the contact's own reading is in the sum (some robots touch)
            assert np.abs(want["contact_alone"]).max() > 1e-3 and np.abs(want["sensed"][cs] - want["contact_alone"]).max() > 1.0
        # the rows that read the wrench are no zeros (the contact's alone may be: a robot clear of its plane)
        assert np.abs(want["wrench_world"]).max() > 1.0 and (ws < 0 or np.abs(want["sensed"][ws]).max() > 1.0)
        assert np.all(got["torque"][what["link"] + 1:] == 0)  # joints outboard of the link: exact zeros
        assert got["robots_pushed"] == got["count_only"] == want["robots_pushed"] == B
        assert np.all(got["steps"] == -1.0)


@pytest.mark.parametrize("sensor_link", [6, 4])
def test_sensed_wrench_reaches_the_task_through_a_tick(sensor_link):
    """Panda, the wrench in the link frame of link 6, the sensor task on that link and on link 4: after the step and one tick
    get_mft_status gives the world force -F_w and the world moment -(M_w + (x - x_c) x F_w) at the control point, 1e-10"""
    B = 65
    case = wc.draw("panda", B, 6, "link")
    mft = pkg.motion_force_task_config("m", link=sensor_link, frame_pos=FRAME_POS)
    mft.sensor_rot[:] = SENSOR_ROT
    mft.sensor_pos[:] = SENSOR_POS
    g = pkg.Controller(case["model"], [mft, pkg.joint_task_config("j")], B)
    g.set_external_wrench(**wc.keywords(case, sensor_task=0))
    g.set_state(case["q"], case["dq"])
    g.reinitialize()
    g.sim_step(case["tau"], wc.DT, wc.SUBSTEPS, True)
    q, dq = g.get_state()
    st_w = g.get_external_wrench_state()
    g.tick()
    st = g.get_mft_status(0)
    rep = wc.reference(case).report(q=q, dq=dq)
    Fw, Mw = st_w["wrench_world"][:3], st_w["wrench_world"][3:]
    assert np.abs(st_w["wrench_world"] - rep["wrench_world"]).max() < 1e-12 * wc.F_MAX
    want_m = -(Mw + np.cross(rep["x"] - st["pos"], Fw, axis=0))
    ef, em = np.abs(st["sensed_force"] + Fw).max(), np.abs(st["sensed_moment"] - want_m).max()
    print(f"2 through the controller, sensor on link {sensor_link}: force {ef:.2e} moment {em:.2e}")
    assert ef < 1e-10 and em < 1e-10
    assert np.abs(Fw).max() > 10 and np.abs(want_m).max() > 1


def _device(*arrays):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("joint", [False, True])
def test_countdown(joint):
    """steps = 0, 1, 3, -1, NaN over the robots of one batch, 5 periods: each robot follows the reference pushed for exactly 0,
    1, 3, 5, 0 periods, the row ends as 0, 0, 0, -1, NaN, the count of every call is exact, and a robot with steps = 0 stays
    within the state bounds of a context without the feature (not bit-equal: the other kernel contracts differently)"""
    B = 130
    case = wc.draw("panda", B, 6, "link")
    pattern = np.array([0.0, 1.0, 3.0, -1.0, np.nan])
    case["rows"][6] = pattern[np.arange(B) % 5]
    g = pkg.Controller(case["model"], [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    bare = pkg.Controller(case["model"], [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    jcase = jc.draw("panda", B)
    jrows, jk = jc.select(jcase, "all")
    wref = wc.reference(case)
    if joint:
        for c in (g, bare):
            c.set_joint_dynamics(**jc.keywords(jrows, jk))
        jd = jc.reference(case, jrows, jk, contact=wr.Combined(wref))
        jd.set_state(case["q"], case["dq"])
    else:
        wref.set_state(case["q"], case["dq"])
    kw = wc.keywords(case, sensor_task=0)
    kw["force"], kw["moment"], kw["steps"] = _device(kw["force"], kw["moment"], kw["steps"])  # a NaN passes through device rows only
    g.set_external_wrench(**kw)
    g.set_state(case["q"], case["dq"])
    bare.set_state(case["q"], case["dq"])
    for p in range(wc.PERIODS):
        g.sim_step(case["tau"], wc.DT, wc.SUBSTEPS, True)
        bare.sim_step(case["tau"], wc.DT, wc.SUBSTEPS, True)
        if joint:
            wref.joint_step(jd, case["tau"], wc.DT, wc.SUBSTEPS, True)
        else:
            wref.step(case["tau"], wc.DT, wc.SUBSTEPS, True)
        want = sum(int(s < 0 or s > p) for s in case["rows"][6] if not np.isnan(s))
        assert g.robots_pushed() == want == np.count_nonzero(wref.active), (p, g.robots_pushed(), want)
        st = g.get_external_wrench_state()
        assert not st["wrench_world"][:, ~wref.active].any() and not st["torque"][:, ~wref.active].any()
        assert not _sensed(g, 0)[:, ~wref.active].any() and _sensed(g, 0)[:, wref.active].all()
    q, dq = g.get_state()
    qr, dqr = jd.get_state() if joint else wref.get_state()
    eq, ev = np.abs(q - qr).max(), np.abs(dq - dqr).max()
    print(f"3 joint={joint}: |dq| {eq:.2e} |ddq| {ev:.2e}")
    assert eq < Q_TOL and ev < V_TOL
    end = g.get_external_wrench()[1][6]
    for k, v in enumerate((0.0, 0.0, 0.0, -1.0)):
        assert np.all(end[k::5] == v), (k, end[k::5])
    assert np.all(np.isnan(end[4::5])) and np.array_equal(end[:4], wref.rows[6][:4])
    qb, dqb = bare.get_state()
    off = np.arange(B) % 5 == 0
    assert np.abs(q[:, off] - qb[:, off]).max() < Q_TOL and np.abs(dq[:, off] - dqb[:, off]).max() < V_TOL
    assert np.abs(q[:, ~off & (np.arange(B) % 5 != 4)] - qb[:, ~off & (np.arange(B) % 5 != 4)]).max() > 1e-7  # the pushed ones did move


@pytest.mark.parametrize("robot", wc.ROBOTS)
def test_balance(robot):
    """robots at rest, tau = -tx from the reference, no gravity: nothing moves, |dq| < 1e-12 rad/s after one period"""
    B = 65
    for link in wc.links(robot):
        case = wc.draw(robot, B, link, "link")
        n = int(case["model"].dof)
        rest = np.zeros((n, B))
        tx = wc.reference(case).wrench(case["q"], rest)["tau"]
        g = pkg.Controller(case["model"], [pkg.joint_task_config("j", robot_dof=n)], B)
        g.set_external_wrench(**wc.keywords(case))
        g.set_state(case["q"], rest)
        g.sim_step(np.ascontiguousarray(-tx), wc.DT, wc.SUBSTEPS, False)
        q, dq = g.get_state()
        print(f"4 {robot} link {link}: |tx| up to {np.abs(tx).max():.1f}, |dq| {np.abs(dq).max():.2e}")
        assert np.abs(tx).max() > 5 and np.abs(dq).max() < 1e-12 and np.abs(q - case["q"]).max() < 1e-14


def test_routing():
    B = 130
    case = wc.draw("panda", B, 6, "world")
    mk = lambda: pkg.Controller(case["model"], [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    g, bare = mk(), mk()
    ids = (_abi.BUF_EXTERNAL_WRENCH, _abi.BUF_EXTERNAL_WRENCH_STATE)
    assert not any(g.device_buffer(i) for i in ids) and g.get_external_wrench()[0].link == -1 and g.robots_pushed() == 0
    st = g.get_external_wrench_state()
    assert not st["wrench_world"].any() and not st["torque"].any()
    free = _steps(bare, case, True)
    g.set_external_wrench(**wc.keywords(case, sensor_task=0))
    assert all(g.device_buffer(i) for i in ids)
    cfg, rows = g.get_external_wrench()
    assert (cfg.link, cfg.frame, cfg.sensor_task, tuple(cfg.point)) == (6, _abi.WRENCH_WORLD, 0, wc.POINT) and np.array_equal(rows, case["rows"])
    pushed = _steps(g, case, True)
    assert np.abs(pushed[0] - free[0]).max() > 1e-6 and g.robots_pushed() == B
    # sai2b_get_bias never sees the wrench: the bias of a context without one at the same state, bit for bit
    bare.set_state(*pushed)
    assert np.array_equal(g.get_bias(True), bare.get_bias(True)) and np.array_equal(g.get_state()[0], pushed[0])
    # nor does a tick: the torques of a context without one at the same state, bit for bit (its sensed rows given the same reading)
    bare.set_mft_sensed_wrench(0, *np.split(_sensed(g, 0), 2))
    for c in (g, bare):
        c.reinitialize()
    assert np.array_equal(g.tick(), bare.tick())
    # reset_robots and reinitialize keep the rows and steps (environment)
    timed = case["rows"].copy()
    timed[6] = 3.0
    g.set_external_wrench(**wc.keywords(case, rows=timed, sensor_task=0))
    g.sim_step(case["tau"], wc.DT, wc.SUBSTEPS, True)
    timed[6] = 2.0
    g.reset_robots(np.ones(B, dtype=np.uint8), case["q"], case["dq"])
    g.reinitialize()
    g.reinitialize_robots(np.ones(B, dtype=np.uint8))
    assert np.array_equal(g.get_external_wrench()[1], timed) and all(g.device_buffer(i) for i in ids)
    # set -> clear: the kernels and the states of a context that never had a wrench
    g.clear_external_wrench()
    assert not any(g.device_buffer(i) for i in ids) and g.get_external_wrench()[0].link == -1 and not g.get_external_wrench()[1].any()
    st = g.get_external_wrench_state()  # the status of the last step with a wrench does not outlive it
    assert st["robots_pushed"] == 0 and not st["wrench_world"].any() and not st["torque"].any()
    f = np.full((3, B), 2.5)
    g.set_mft_sensed_wrench(0, f, -f)
    again = _steps(g, case, True)
    assert np.array_equal(again[0], free[0]) and np.array_equal(again[1], free[1])
    assert np.array_equal(_sensed(g, 0), np.concatenate([f, -f]))  # no sensor writes after a clear
    # a later set finds the rows kept; a [3] force broadcasts over the batch, moment and steps default to 0 and -1
    g.set_external_wrench(6, [1.0, -2.0, 3.0])
    rows = g.get_external_wrench()[1]
    assert np.all(rows[0] == 1.0) and np.all(rows[1] == -2.0) and np.all(rows[2] == 3.0) and not rows[3:6].any() and np.all(rows[6] == -1.0)


def test_device_rows():
    """torch device tensors through the setter, and rows rewritten in place through SAI2B_BUF_EXTERNAL_WRENCH, give the bits of
    host arrays"""
    import torch

    B = 130
    case = wc.draw("panda", B, 3, "link")
    mk = lambda: pkg.Controller(case["model"], [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    host, dev, raw = mk(), mk(), mk()
    host.set_external_wrench(**wc.keywords(case))
    want = _steps(host, case, True)
    kw = wc.keywords(case)
    kw["force"], kw["moment"], kw["steps"] = _device(kw["force"], kw["moment"], kw["steps"])
    dev.set_external_wrench(**kw)
    assert np.array_equal(dev.get_external_wrench()[1], case["rows"])
    got = _steps(dev, case, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a device-resident producer: zero rows set, one step (nobody pushed), then the rows written in place
    raw.set_external_wrench(case["link"], np.zeros((3, B)), steps=np.zeros(B), point=case["point"], frame=case["frame"])
    raw.set_state(case["q"], case["dq"])
    raw.sim_step(case["tau"], wc.DT, wc.SUBSTEPS, True)
    assert raw.robots_pushed() == 0
    p = raw.device_buffer(_abi.BUF_EXTERNAL_WRENCH)

    class _Raw:  # zero-copy torch view of the library's wrench rows
        __cuda_array_interface__ = {"data": (int(p), False), "shape": (7, B), "typestr": "<f8", "version": 2}

    raw.synchronize()
    torch.as_tensor(_Raw(), device="cuda").copy_(torch.as_tensor(case["rows"], device="cuda"))
    torch.cuda.synchronize()
    got = _steps(raw, case, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and raw.robots_pushed() == B


def test_argument_checks():
    B = 65
    case = wc.draw("panda", B)
    g = pkg.Controller(case["model"], [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    g.set_external_wrench(**wc.keywords(case))
    rows = case["rows"]
    bad = lambda a, v: (lambda x: (x.__setitem__((..., 5), v), x)[1])(a.copy())
    F, M, S = rows[0:3], rows[3:6], rows[6]
    for f, m, s in ((bad(F, np.nan), M, S), (bad(F, np.inf), M, S), (F, bad(M, np.nan), S), (F, bad(M, -np.inf), S), (F, M, bad(S, np.nan))):
        with pytest.raises(ValueError):
            g.set_external_wrench(6, f, m, s)
    g.set_external_wrench(6, F, M, bad(S, np.inf))  # an infinite count is a count
    g.set_external_wrench(**wc.keywords(case))
    # each reason of sai2b_validate_external_wrench, through the setter
    for kw in (dict(link=7), dict(link=-1), dict(frame=2), dict(frame="tool"), dict(point=(0.0, np.nan, 0.0)), dict(sensor_task=1), dict(sensor_task=5)):
        args = dict(link=6, force=F)
        args.update(kw)
        with pytest.raises(ValueError):
            g.set_external_wrench(**args)
    cfg = _abi.ExternalWrenchConfig()
    g.lib.sai2b_default_external_wrench(C.byref(cfg), 6)
    assert g.lib.sai2b_set_external_wrench(g.h, C.byref(cfg), None, None, None, 0) == _abi.INVALID_ARGUMENT  # force is required
    assert g.lib.sai2b_set_external_wrench(None, C.byref(cfg), None, None, None, 0) == _abi.INVALID_ARGUMENT
    assert np.array_equal(g.get_external_wrench()[1], rows)  # a rejected call leaves the wrench as it was
    with pytest.raises(ValueError):
        g.set_external_wrench(6, np.zeros((3, B + 1)))


# ---- 8: the resident loop, pushed and released
LOOP_B, LOOP_PERIODS, LOOP_PUSHED, LOOP_FORCE = 64, 150, 50, (20.0, 0.0, 0.0)


def _loop_setup(B):
    inp = pkg.workloads.make_inputs(3, B=B, seed=11)
    rows = np.zeros((7, B))
    rows[0:3] = np.array(LOOP_FORCE)[:, None]
    rows[6] = LOOP_PUSHED
    return inp, rows


def _cpu_loop(inp, rows, q0=None, periods=LOOP_PERIODS):
    """oracle tick + the reference's step on the oracle's own state -> q, dq, control-point positions [periods + 1][3][B],
    position-error norms [periods + 1][B]"""
    B = inp["q"].shape[1]
    o = ol.Oracle(ol.panda_model(), [ol.motion_force_task("m"), ol.joint_task("j")], B, threads=8)
    ref = wr.ExternalWrenchReference(ol.panda_model(), B, pkg.workloads.EE_LINK, rows, pkg.workloads.EE_FRAME_POS, wr.WORLD, plant=o)
    o.set_state(inp["q"] if q0 is None else q0, np.zeros_like(inp["q"]))
    o.reinitialize()  # the goals are the pose the robots start in: they hold it, are pushed off it and come back
    xs, es = [], []
    for p in range(periods + 1):
        st = o.get_mft_status(0)
        xs.append(st["pos"].copy())
        es.append(st["pos_error_norm"].copy())
        if p < periods:
            ref.step(o.tick(), 0.001, 1, False)
    q, dq = o.get_state()
    return q, dq, np.stack(xs), np.stack(es)


# Measured on the CPU (B = 64, seed 11, 150 periods): the loop started one ulp off (numpy.nextafter on every q) ends 1.332e-15 rad
# and 4.594e-15 rad/s from the loop itself. Pushed, every control point moves along the force, monotonically, from 2.07e-6 m
# after one period to between 1.91 and 5.21 mm after 50. The position-error norm peaks at periods 125..126 (3.9 to 10.3 mm: the
# robots coast on after the release) and is below a tenth of its peak for good from period 516 on, for every robot.
CPU_ONE_ULP_Q, CPU_ONE_ULP_DQ, CPU_RECOVERED_AT = 1.332e-15, 4.594e-15, 516


def test_resident_loop_pushed_and_released():
    """64 Pandas, the headline hierarchy (MotionForceTask + JointTask) holding the pose they start in, tick -> sim_step(None) ->
    observe with nothing else on the host's side of the loop: a world-frame push of 20 N on the end-effector link at the
    control point for 50 periods (steps = 50: the kernel counts it down and releases), 150 periods in all, against the same
    loop on the CPU (oracle tick + tests/external_wrench_reference.py).
    Bound: 10 x the largest distance between that CPU loop and the CPU loop started one ulp off, measured on the CPU first:
    1.332e-15 rad and 4.594e-15 rad/s, so 1.332e-14 rad and 4.594e-14 rad/s. Also: every robot's control point moves along
    the force while pushed (period over period), the count of robots pushed is 64 for 50 calls and 0 afterwards, and the
    loop carried on, the position-error norm of every robot is below a tenth of its peak from period 518 on (the CPU
    loop: 516; the norm falls by about 1 % per period there, so rounding moves the crossing by one period at the most)."""
    B = LOOP_B
    inp, rows = _loop_setup(B)
    qc, dqc, xs_c, es_c = _cpu_loop(inp, rows)
    g = pkg.Controller(pkg.panda_model(), [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    g.set_state(inp["q"], np.zeros_like(inp["q"]))
    g.reinitialize()
    g.set_external_wrench(pkg.workloads.EE_LINK, rows[0:3], rows[3:6], rows[6], point=pkg.workloads.EE_FRAME_POS)
    g.set_observation(tasks=(0,), task_blocks=("pose", "error"))
    lay = g.observation_layout()
    pos, err = lay["pose0"].start, lay["error0"].start + 6
    xs, es, counts = [], [], []
    state_150 = None
    for p in range(CPU_RECOVERED_AT + 8):
        if p == LOOP_PERIODS:
            state_150 = g.get_state()
        g.tick(want_output=False)
        g.sim_step(None, 0.001, 1)
        out, _ = g.observe(done=False)
        xs.append(out[pos:pos + 3].copy())
        es.append(out[err].copy())
        if p < LOOP_PERIODS:
            counts.append(g.robots_pushed())
    q, dq = state_150
    eq, ev = np.abs(q - qc).max(), np.abs(dq - dqc).max()
    print(f"8 resident vs cpu after {LOOP_PERIODS} periods: |dq| {eq:.3e} (bound {10 * CPU_ONE_ULP_Q:.3e}) |ddq| {ev:.3e} (bound {10 * CPU_ONE_ULP_DQ:.3e})")
    xs, es = np.stack(xs), np.stack(es)
    F = np.array(LOOP_FORCE) / np.linalg.norm(LOOP_FORCE)
    along = np.einsum("pib,i->pb", xs - xs_c[0], F)  # xs[p]: after period p + 1
    peak = es.max(axis=0)
    print(f"8 along the force after 1 / 50 periods: {along[0].min():.3e} / {along[LOOP_PUSHED - 1].min():.3e}..{along[LOOP_PUSHED - 1].max():.3e} m, "
          f"peak error {peak.min():.3e}..{peak.max():.3e} at {es.argmax(axis=0).min() + 1}..{es.argmax(axis=0).max() + 1}, "
          f"largest error / peak from period {CPU_RECOVERED_AT + 2} on: {(es[CPU_RECOVERED_AT + 1:] / peak).max():.4f}")
    assert counts == [B] * LOOP_PUSHED + [0] * (LOOP_PERIODS - LOOP_PUSHED)
    assert np.all(along[0] > 0) and np.all(np.diff(along[:LOOP_PUSHED], axis=0) > 0) and along[LOOP_PUSHED - 1].min() > 1e-3
    assert np.abs(xs[:LOOP_PERIODS] - xs_c[1:]).max() < 1e-9 and np.abs(q - inp["q"]).max() > 1e-2
    assert np.all(es[CPU_RECOVERED_AT + 1:] < 0.1 * peak)
    assert not g.get_external_wrench()[1][6].any()  # the countdown ended at 0
    assert eq < 10 * CPU_ONE_ULP_Q and ev < 10 * CPU_ONE_ULP_DQ, (eq, ev)
