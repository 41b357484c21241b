"""GPU tests (-m gpu) of the actuator and force-sensor models (csrc/sai2b_hardware.hip: actuate_kernel, sense_kernel,
hardware_reset_kernel) against tests/hardware_reference.py. Inputs: tests/hardware_cases.py (planar_4r, Panda, sliding_base:
4, 7 and 8 joints; B = 1, 5, 200 and 4 099, which is no multiple of 64), periods of 1 ms with 3 substeps.

1: identity. 2: delay alone. 3: each effect alone and all together against the reference, on the plain plant and the eight
payload x contact x joint-dynamics forms with an external wrench: state, applied torque, sensed rows, the status rows of
contact, joint dynamics and wrench, and the counters. 4: the sensor stage. 5: reset. 6: reproducibility and
shards. 7: snapshot banks. 8: device rows and argument checks.

Evaluation rule of 3 and 4: the applied torques do not depend on the plant's state, so they are compared with the reference's
own; the ideal sensor reading does (a contact stiffness of 2e3 N/m turns a state error of 1e-12 into 2e-9 N), so, as
tests/test_gpu_contact.py does, the reference's reading of each period is evaluated at the state the GPU reached in it and
the sensor law is applied to that."""
import ctypes as C
import functools

import numpy as np
import pytest

import contact_cases as cc
import contact_loop as cl
import external_wrench_cases as wc
import external_wrench_reference as wr
import hardware_cases as hc
import hardware_reference as hr
import joint_dynamics_cases as jc
import oracle_lib as ol
import payload_cases as pc
import plumbing
import sai2_primitives_perso_amd as pkg
from contact_reference import ContactReference
from sai2_primitives_perso_amd import _abi, sharding

pytestmark = pytest.mark.gpu

FRAME_POS = (0.01, 0.02, 0.06)
SENSOR_POS = (0.0, 0.01, -0.03)
SENSOR_ROT = [np.cos(0.4), -np.sin(0.4), 0, np.sin(0.4), np.cos(0.4), 0, 0, 0, 1]
Q_TOL, V_TOL, ROW_TOL = 1e-12, 1e-10, 1e-12
CASES = [(r, B) for r in hc.ROBOTS for B in hc.BATCHES[:3]] + [("panda", 4099)]
FORMS = [None] + [(p, c, j) for p in (False, True) for c in (False, True) for j in (False, True)]  # None: the plain plant, no wrench
SENSORS = [(0, 0), (0, 1), (0, -1), (-1, 1)]  # (contact's sensor task, wrench's) of the runs with a contact


def _tasks(mk_mft, mk_jt, link, other, n):
    out = []
    for name, l in (("m", link), ("o", other)):
        mft = mk_mft(name, link=l, frame_pos=FRAME_POS, robot_dof=n)
        mft.sensor_rot[:] = SENSOR_ROT
        mft.sensor_pos[:] = SENSOR_POS
        out.append(mft)
    return out + [mk_jt("j", robot_dof=n)]


def _controller(case):
    n = int(case["model"].dof)
    return pkg.Controller(case["model"], _tasks(pkg.motion_force_task_config, pkg.joint_task_config, case["link"], case["link"] - 1, n), case["q"].shape[1])


def _sensed(g, task=0):
    return plumbing.device_rows(g, _abi.BUF_SENSED, task, 6)


def _tau(g):
    return plumbing.device_rows(g, _abi.BUF_TAU, -1, g.dof)


def _applied(g):
    return plumbing.device_rows(g, _abi.BUF_TAU_APPLIED, -1, g.dof)


def _to_device(g, which, rows):
    """host rows into a ctx buffer, ordered behind the ctx stream"""
    g.synchronize()
    hip = C.CDLL(pkg._abi.LIB_PATH).hipMemcpy
    hip.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert hip(g.device_buffer(which, -1), rows.ctypes.data, rows.nbytes, 1) == 0  # hipMemcpyHostToDevice


# ---------------------------------------------------------------------------------------------- 1: identity
@pytest.mark.parametrize("B", hc.BATCHES)
def test_identity(B):
    """C3 closed loop with contact sensed on task 0, 20 periods (position control sinking, force control from period 10): a
    context with the default hardware and the ideal rows against a twin that never sets it, bit for bit every period"""
    inp = cl.inputs(B)
    rows = inp["rows"].copy()
    rows[2] += cl.DEPTH0 + 0.0005  # the planes half a millimetre above the start heights: every robot presses from the first period
    recs = []
    for hardware in (False, True):
        cfgs = cl.configs(pkg.motion_force_task_config, pkg.joint_task_config)
        g = pkg.Controller(pkg.panda_model(), cfgs, B)
        g.set_contact(cl.LINK, cl.POINT, rows[0:3], rows[3:6], rows[6], rows[7], rows[8], sensor_task=0, friction_velocity_eps=cl.V_EPS)
        if hardware:
            g.set_hardware(sensor_task=0)
        rec = []

        def after_step(g=g, rec=rec, hardware=hardware):
            st = g.get_contact_state()
            rec.append(dict(state=np.concatenate(g.get_state()), tau=_tau(g), sensed=_sensed(g), depth=st["depth"], force=st["normal_force"],
                            wrench=st["wrench_world"], touching=st["robots_in_contact"], applied=_applied(g) if hardware else None))

        cl.run(g, cfgs[0], inp, 20, after_step, lambda: 0, switch_at=10)
        recs.append(rec)
        if hardware:
            st = g.get_hardware_state()
            assert np.all(st["period"] == 20) and np.all(st["episode"] == 0)
    assert len(recs[0]) == len(recs[1]) == 20
    for p, (a, b) in enumerate(zip(*recs)):
        for key in ("state", "tau", "sensed", "depth", "force", "wrench"):
            assert np.array_equal(a[key], b[key]), (p, key)
        assert a["touching"] == b["touching"] and np.array_equal(b["applied"], b["tau"]), p
    assert np.abs(recs[1][-1]["sensed"]).max() > 0.1 and np.abs(recs[1][-1]["tau"]).max() > 0.1


# ---------------------------------------------------------------------------------------------- 2: delay alone
@pytest.mark.parametrize("robot, B, depth, periods", [(r, B, 3, 9) for r in hc.ROBOTS for B in hc.BATCHES] + [(r, 5, 8, 19) for r in hc.ROBOTS])
def test_delay_alone(robot, B, depth, periods):
    """alpha 1, k 1, sigma 0: the applied torque of period n is, bit for bit, the command of period max(n - d_b, 0); D = 3 with
    d_b cycling 0..3 over 9 periods (the history wraps twice), D = 8 with d_b = 8 over 19"""
    case = wc.draw(robot, B)
    n = case["tau"].shape[0]
    act, _ = hr.ideal_rows(n, B)
    act[0] = np.arange(B) % (depth + 1) if depth == 3 else depth
    g = _controller(case)
    g.set_hardware(act, None, max_delay=depth)
    g.set_state(case["q"], case["dq"])
    cmds = hc.commands(case, periods)
    cols = np.arange(B)
    for p in range(periods):
        g.sim_step(cmds[p], hc.DT, hc.SUBSTEPS, False)
        got = g.get_hardware_state()
        want = cmds[np.maximum(p - act[0].astype(int), 0), :, cols].T
        assert np.array_equal(got["applied_torque"], want), p
        assert np.all(got["period"] == p + 1)
    assert not np.array_equal(cmds[0], cmds[1])


# ---------------------------------------------------------------------------------------------- 3: against the reference
def _plan(robot, B):
    """[(form, effect, gravity, contact's sensor task, wrench's sensor task)]: all nine forms, the effect moving through them
    with (robot, B) so that over the parametrisation every effect meets every form; the runs with a contact take the four
    sensor pairings"""
    shift = hc.ROBOTS.index(robot) + hc.BATCHES.index(B)
    out, with_contact = [], 0
    for k, form in enumerate(FORMS):
        effect = hc.EFFECTS[(k + shift) % 4]
        if form is not None and form[1]:
            cs, ws = SENSORS[(with_contact + shift) % 4]
            with_contact += 1
        else:
            cs, ws = -1, (k + shift) % 2
        out.append((form, effect, bool((k + shift) % 2), cs, ws))
    return out


def test_plan_covers_every_effect_on_every_form():
    seen = {(f, e) for robot, B in CASES for f, e, *_ in _plan(robot, B)}
    assert seen == {(f, e) for f in FORMS for e in hc.EFFECTS}
    for robot, B in CASES:
        assert sorted(run[3:] for run in _plan(robot, B) if run[0] is not None and run[0][1]) == sorted(SENSORS)


@functools.lru_cache(maxsize=None)
def _run(robot, B):
    case = wc.draw(robot, B)
    n, link = int(case["model"].dof), case["link"]
    g = _controller(case)
    o = ol.Oracle(case["model"], _tasks(ol.motion_force_task, ol.joint_task, link, link - 1, n), B, threads=8)
    con = case["contact"]
    r = con["rows"]
    cmds = hc.commands(case)
    out = []
    for form, effect, grav, cs, ws in _plan(robot, B):
        payload, contact, joint = form if form is not None else (False, False, False)
        if payload:
            g.set_link_payload(link, *pc.model_rows(robot, link, *pc.rows(B)), target="plant")
        else:
            g.clear_link_payload("plant")
        if contact:
            g.set_contact(link, con["points"], r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=cs, friction_velocity_eps=cc.V_EPS)
        else:
            g.clear_contact()
        jrows, jk = jc.select(jc.draw(robot, B), "all")
        if joint:
            g.set_joint_dynamics(**jc.keywords(jrows, jk))
        else:
            g.clear_joint_dynamics()
        if form is not None:
            g.set_external_wrench(**wc.keywords(case, sensor_task=ws))
        else:
            g.clear_external_wrench()
            ws = -1
        D, act, sen = hc.rows(robot, B, effect, sensor=True)
        g.set_hardware(act, sen, max_delay=D, sensor_task=0, seed=hc.SEED)
        hw = hr.HardwareReference(n, B, D, act, sen, seed=hc.SEED)
        # the reference's plant
        plant = pc.PayloadOracles(pc.texts(robot, link), o.tasks, B) if payload else None
        cref = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS) if contact else None
        rows0 = case["rows"] if form is not None else np.zeros_like(case["rows"])
        wref = wc.reference(case, plant=None if joint else plant, contact=cref, rows=rows0)
        jd = None
        if joint:
            jd = jc.reference(case, jrows, jk, plant=plant, contact=wr.Combined(wref))
            jd.set_state(case["q"], case["dq"])
        else:
            wref.set_state(case["q"], case["dq"])
        at = wc.reference(case, rows=rows0)
        due = cs == 0 or ws == 0
        manual = np.full((6, B), 0.25)
        g.set_mft_sensed_wrench(0, manual[:3], manual[3:])
        g.set_state(case["q"], case["dq"])
        rec = dict(applied=[], sensed=[], clipped=[])
        for p in range(hc.PERIODS):
            g.sim_step(cmds[p], hc.DT, hc.SUBSTEPS, grav)
            q, dq = g.get_state()
            applied = hw.actuate(cmds[p])
            if joint:
                wref.joint_step(jd, applied, hc.DT, hc.SUBSTEPS, grav)
            else:
                wref.step(applied, hc.DT, hc.SUBSTEPS, grav)
            want_s = manual
            if due:
                ideal = np.zeros((6, B))
                if ws == 0:
                    ideal = ideal + at.report(sensor=(o, 0), q=q, dq=dq)["sensed"]
                if cs == 0:
                    cat = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS)
                    cat.set_state(q, dq)
                    ideal = ideal + cat.report(sensor=(o, 0))["sensed"]
                want_s = hw.sense(ideal)
            hw.advance()
            rec["applied"].append((_applied(g), applied))
            rec["sensed"].append((_sensed(g), want_s))
            if joint:
                rec["clipped"].append((g.get_joint_dynamics_state()["applied_torque"], np.clip(applied, -jrows[3], jrows[3])))
        st = g.get_hardware_state()
        qr, dqr = jd.get_state() if joint else wref.get_state()
        # the status rows the plant left after the last period, against the references evaluated at the state the GPU ended in:
        # [(name, got, want, tolerance)] and [(name, got count, wanted count)]
        status, counts = [], []
        if form is not None:
            got_w, rep_w = g.get_external_wrench_state(), at.report(q=q, dq=dq)
            for key in ("wrench_world", "torque"):
                status.append((f"wrench {key}", got_w[key], rep_w[key], ROW_TOL * max(1.0, np.abs(rep_w[key]).max())))
            counts.append(("robots pushed", got_w["robots_pushed"], rep_w["robots_pushed"]))
        if contact:
            cat = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS)
            cat.set_state(q, dq)
            rep_c, got_c = cat.report(sensor=(o, cs) if cs >= 0 else None), g.get_contact_state()
            tol = ROW_TOL * max(1.0, np.abs(rep_c["wrench_world"][:3]).max(), rep_c["normal_force"].max())
            for key in ("depth", "normal_force"):
                status.append((f"contact {key}", got_c[key], rep_c[key], tol))
            # the moment rows are about the sensor task's control point: compared where the contact has one
            rows_w = slice(0, 6) if cs >= 0 else slice(0, 3)
            status.append(("contact wrench_world", got_c["wrench_world"][rows_w], rep_c["wrench_world"][rows_w], tol))
            counts.append(("robots in contact", got_c["robots_in_contact"], rep_c["robots_in_contact"]))
        if joint:
            at_j = jc.reference(case, jrows, jk)
            at_j.load(q, dq, applied)
            rep_j, got_j = at_j.report(), g.get_joint_dynamics_state()
            for key in ("applied_torque", "stop_torque", "dissipative_torque"):
                status.append((f"joint {key}", got_j[key], rep_j[key], ROW_TOL * max(1.0, np.abs(rep_j[key]).max())))
            counts += [("robots saturated", got_j["robots_saturated"], rep_j["robots_saturated"]), ("robots at a stop", got_j["robots_at_stop"], rep_j["robots_at_stop"])]
        out.append((dict(form=form, effect=effect, gravity=grav, sensors=(cs, ws), due=due), rec,
                    dict(q=q, dq=dq, qr=qr, dqr=dqr, st=st, status=status, counts=counts)))
    return out


@pytest.mark.parametrize("robot, B", CASES)
def test_effects_follow_the_reference(robot, B):
    for what, rec, end in _run(robot, B):
        eq, ev = np.abs(end["q"] - end["qr"]).max(), np.abs(end["dq"] - end["dqr"]).max()
        ea = max(np.abs(a - b).max() for a, b in rec["applied"])
        es = max(np.abs(a - b).max() / max(1.0, np.abs(b).max()) for a, b in rec["sensed"])
        ec = max([np.abs(a - b).max() for a, b in rec["clipped"]] or [0.0])
        print(f"3 {robot} B={B} {what}: |dq| {eq:.2e} |ddq| {ev:.2e} applied {ea:.2e} sensed {es:.2e} saturated {ec:.2e}")
        assert eq < Q_TOL and ev < V_TOL, (what, eq, ev)
        assert ea < ROW_TOL and es < ROW_TOL and ec < ROW_TOL, (what, ea, es, ec)
        errs = {name: (float(np.abs(got - want).max()), tol) for name, got, want, tol in end["status"]}
        print(f"3 {robot} B={B} {what}: status rows {errs} counts {end['counts']}")
        assert all(e < tol for e, tol in errs.values()), (what, errs)
        assert all(got == want for _, got, want in end["counts"]), (what, end["counts"])
        form = what["form"]
        assert len(errs) == (0 if form is None else 2 + 3 * form[1] + 3 * form[2])
        assert np.all(end["st"]["period"] == hc.PERIODS) and np.all(end["st"]["episode"] == 0)
        if not what["due"]:  # a reading set by hand is left alone, bit for bit
            assert all(np.array_equal(a, b) for a, b in rec["sensed"])
        # the effect is visible: the applied torques are not the command
        assert np.abs(rec["applied"][-1][1] - hc.commands(wc.draw(robot, B))[-1]).max() > 1e-3


# ---------------------------------------------------------------------------------------------- 4: the sensor stage
@pytest.mark.parametrize("cs, ws, contact", [(0, -1, True), (-1, 0, False), (0, 0, True), (-1, 1, True), (1, -1, True)])
def test_sensor_stage(cs, ws, contact):
    """bias, noise and filter on the contact's reading, the wrench's and their sum, with the ideal actuator rows: the twin
    without hardware is then bit-equal in state, its sensed rows are the ideal reading of every period, and the measured rows
    follow the reference's sensor law applied to them. Neither writes task 0: the stage is not launched (launch counter) and
    the rows stay as set by hand"""
    B = 200
    case = wc.draw("panda", B)
    con = case["contact"]
    r = con["rows"]
    _, _, sen = hc.rows("panda", B, "gain", sensor=True)
    g, twin = _controller(case), _controller(case)
    hw = hr.HardwareReference(7, B, 0, None, sen, seed=77)
    manual = np.full((6, B), -0.5)
    for c in (g, twin):
        if contact:
            c.set_contact(case["link"], con["points"], r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=cs, friction_velocity_eps=cc.V_EPS)
        c.set_external_wrench(**wc.keywords(case, sensor_task=ws))
        c.set_mft_sensed_wrench(0, manual[:3], manual[3:])
        c.set_state(case["q"], case["dq"])
    g.set_hardware(None, sen, sensor_task=0, seed=77)
    due = cs == 0 or ws == 0
    cmds = hc.commands(case)
    for p in range(hc.PERIODS):
        before = (g.counters()[0], twin.counters()[0])
        g.sim_step(cmds[p], hc.DT, hc.SUBSTEPS, True)
        twin.sim_step(cmds[p], hc.DT, hc.SUBSTEPS, True)
        assert (g.counters()[0] - before[0], twin.counters()[0] - before[1]) == (3 if due else 2, 1)
        assert all(np.array_equal(a, b) for a, b in zip(g.get_state(), twin.get_state()))
        ideal, got = _sensed(twin), _sensed(g)
        if due:
            want = hw.sense(ideal)
            err = np.abs(got - want).max()
            assert err < ROW_TOL * max(1.0, np.abs(want).max()), (p, err)
            assert np.abs(got - ideal).max() > 0.05
        else:
            assert np.array_equal(got, manual) and np.array_equal(ideal, manual)
        for t in {cs, ws} - {0, -1}:  # another task's sensor rows are the ideal ones
            assert np.array_equal(_sensed(g, t), _sensed(twin, t))
        hw.advance()
    if due:
        assert np.abs(ideal).max() > 1.0


def test_measured_force_trips_done_force():
    """a constructed case: the ideal force stays under the limit, the sensor's bias lifts the measured one over it"""
    B = 130
    case = wc.draw("panda", B)
    rows = case["rows"].copy()
    rows[0:3] = np.array([[3.0], [0.0], [0.0]])
    rows[3:6] = 0.0
    _, sen = hr.ideal_rows(7, B)
    sen[0, ::2] = 20.0  # every other robot's sensor reads 20 N too much along x
    done = {}
    for hardware in (False, True):
        g = _controller(case)
        g.set_external_wrench(**wc.keywords(case, rows=rows, sensor_task=0))
        g.set_observation(force_tasks=[0], max_sensed_force=10.0)
        if hardware:
            g.set_hardware(None, sen, sensor_task=0)
        g.set_state(case["q"], case["dq"])
        g.sim_step(case["tau"], hc.DT, hc.SUBSTEPS, True)
        done[hardware] = g.observe(out=False)[1]
    assert not np.any(done[False] & _abi.DONE_FORCE)
    assert np.array_equal((done[True] & _abi.DONE_FORCE) != 0, np.arange(B) % 2 == 0)


# ---------------------------------------------------------------------------------------------- 5: reset
def test_reset():
    """after 4 periods a scattered mask is reset with new states, then 4 more periods: selected robots follow the reference
    restarted with n = 0, e = 1 (their applied torques, and their state under a plant reference started at the new state);
    unselected robots are bit-equal to a context that never made the call; reinitialize_robots leaves the clocks alone.
    A wrench is sensed on task 0 through a sensor with bias, noise and a filter (alpha_s < 1 for three robots in four): a third
    context with the same actuators and the same reset but an ideal sensor is bit-equal in state and holds the ideal reading of
    every period, and the measured rows follow the reference's sensor law on it, re-initialised at n = 0 for the reset robots"""
    B = 200
    case = wc.draw("panda", B)
    D, act, sen = hc.rows("panda", B, "all", sensor=True)
    mask = (np.arange(B) % 3 == 0) | (np.arange(B) == B - 1)
    new = wc.draw("panda", B, seed=1)
    g, twin, ideal = _controller(case), _controller(case), _controller(case)
    hw = hr.HardwareReference(7, B, D, act, sen, seed=5)
    cmds = hc.commands(case, 8)
    for c in (g, twin, ideal):
        c.set_external_wrench(**wc.keywords(case, sensor_task=0))
        c.set_hardware(act, None if c is ideal else sen, max_delay=D, sensor_task=0, seed=5)
        c.set_state(case["q"], case["dq"])

    def sensor_follows(p):
        """g's measured rows against the sensor law on the ideal context's reading; the two are in the same state"""
        assert all(np.array_equal(x, y) for x, y in zip(g.get_state(), ideal.get_state())), p
        reading = _sensed(ideal)
        want_s, got_s = hw.sense(reading), _sensed(g)
        assert np.abs(got_s - want_s).max() < ROW_TOL * max(1.0, np.abs(want_s).max()), p
        return reading, want_s

    for p in range(4):
        for c in (g, twin, ideal):
            c.sim_step(cmds[p], hc.DT, hc.SUBSTEPS, False)
        hw.actuate(cmds[p])
        sensor_follows(p)
        hw.advance()
    g_before = hw.g.copy()
    g.reinitialize_robots(mask.astype(np.uint8))
    st = g.get_hardware_state()
    assert np.all(st["period"] == 4) and np.all(st["episode"] == 0)
    launches = g.counters()[0]
    g.reset_robots(mask.astype(np.uint8), new["q"], new["dq"])
    assert g.counters()[0] - launches == 2
    ideal.reset_robots(mask.astype(np.uint8), new["q"], new["dq"])
    hw.reset(mask)
    st = g.get_hardware_state()
    assert np.array_equal(st["period"], np.where(mask, 0, 4)) and np.array_equal(st["episode"], mask.astype(int))
    o = wc.reference(case)  # the plant under the same wrench, started at the new states
    o.set_state(new["q"], new["dq"])
    filtered = sen[12] < 1.0
    assert np.count_nonzero(filtered & mask) > 10 and np.count_nonzero(filtered & ~mask) > 10
    for p in range(4, 8):
        for c in (g, twin, ideal):
            c.sim_step(cmds[p], hc.DT, hc.SUBSTEPS, False)
        want = hw.actuate(cmds[p])
        reading, want_s = sensor_follows(p)
        if p == 4:  # period 0 of the new episode: the filter starts from its input; a robot that was not reset filters on
            z = hr.normals(hw.n, hw.e, hr.SENSOR, hw.robot, 5, 6)
            y = (reading + sen[0:6]) + sen[6:12] * z
            assert np.array_equal(want_s[:, mask], y[:, mask])
            old = (g_before + sen[12] * (y - g_before))[:, filtered & ~mask]
            assert np.abs(want_s[:, filtered & ~mask] - old).max() < 1e-13 and np.abs(old - y[:, filtered & ~mask]).max() > 1e-3
        hw.advance()
        o.step(want, hc.DT, hc.SUBSTEPS, False)
        got, other = g.get_hardware_state()["applied_torque"], twin.get_hardware_state()["applied_torque"]
        assert np.abs(got - want).max() < ROW_TOL
        assert np.array_equal(got[:, ~mask], other[:, ~mask]) and np.abs(got[:, mask] - other[:, mask]).max() > 1e-3
    (q, dq), (qt, dqt), (qr, dqr) = g.get_state(), twin.get_state(), o.get_state()
    assert np.array_equal(q[:, ~mask], qt[:, ~mask]) and np.array_equal(dq[:, ~mask], dqt[:, ~mask])
    assert np.abs(q - qr)[:, mask].max() < Q_TOL and np.abs(dq - dqr)[:, mask].max() < V_TOL
    st = g.get_hardware_state()
    assert np.array_equal(st["period"], np.where(mask, 4, 8)) and np.array_equal(st["episode"], mask.astype(int))


# ---------------------------------------------------------------------------------------------- 6: reproducibility, shards
def _noisy_run(case, act, sen, D, seed, cols=slice(None), first_robot=None, world_rank=None):
    sub = dict(case, q=np.ascontiguousarray(case["q"][:, cols]), dq=np.ascontiguousarray(case["dq"][:, cols]))
    g = _controller(sub)
    if world_rank is not None:
        sharding.set_hardware(g, *world_rank, case["q"].shape[1], act, sen, max_delay=D, seed=seed)
    else:
        g.set_hardware(act, sen, max_delay=D, seed=seed)
    g.set_state(sub["q"], sub["dq"])
    cmds = hc.commands(case)
    applied = []
    for p in range(hc.PERIODS):
        g.sim_step(np.ascontiguousarray(cmds[p][:, cols]), hc.DT, hc.SUBSTEPS, True)
        applied.append(g.get_hardware_state()["applied_torque"])
    return np.concatenate([*g.get_state(), *applied])


def test_reproducibility_and_shards():
    B = 4099
    case = wc.draw("panda", B)
    D, act, sen = hc.rows("panda", B, "all")
    a, b, c = (_noisy_run(case, act, sen, D, s) for s in (11, 11, 12))
    assert np.array_equal(a, b) and np.abs(a - c).max() > 1e-3
    lo, hi = sharding.shard_bounds(B, 2, 0)
    assert (lo, hi) == (0, 2050) and sharding.shard_bounds(B, 2, 1) == (2050, 4099)
    parts = [_noisy_run(case, act, sen, D, 11, slice(*sharding.shard_bounds(B, 2, r)), world_rank=(2, r)) for r in (0, 1)]
    assert np.array_equal(np.concatenate(parts, axis=1), a)


# ---------------------------------------------------------------------------------------------- 7: snapshot banks
def _loop_ctx(case, D, act, sen, seed=3):
    con = case["contact"]
    r = con["rows"]
    mft = pkg.motion_force_task_config("m", link=case["link"], frame_pos=FRAME_POS)
    mft.sensor_rot[:] = SENSOR_ROT
    mft.sensor_pos[:] = SENSOR_POS
    g = pkg.Controller(case["model"], [mft, pkg.joint_task_config("j")], case["q"].shape[1])
    g.set_contact(case["link"], con["points"], r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=0, friction_velocity_eps=cc.V_EPS)
    g.set_hardware(act, sen, max_delay=D, sensor_task=0, seed=seed)
    g.set_state(case["q"], case["dq"])
    g.reinitialize()
    return g


def _period(g):
    g.tick(want_output=False)
    g.sim_step(None, hc.DT, hc.SUBSTEPS, True)


def _everything(g):
    st = g.get_hardware_state()
    return np.concatenate([*g.get_state(), _tau(g), st["applied_torque"], _sensed(g), st["period"][None].astype(float), st["episode"][None].astype(float)])


def _differing_rows(a, b):
    """rows of _everything (q 0-6, dq 7-13, tau 14-20, applied 21-27, sensed 28-33, period 34, episode 35) that differ"""
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return np.flatnonzero(~np.all(a == b, axis=1)).tolist()


def test_snapshot():
    B = 200
    case = wc.draw("panda", B)
    D, act, sen = hc.rows("panda", B, "all", sensor=True)
    g, twin = _loop_ctx(case, D, act, sen), _loop_ctx(case, D, act, sen)
    what = _abi.SNAP_EPISODE | _abi.SNAP_ENVIRONMENT
    bank = g.snapshot_bank(B, what)
    assert {"hw_history", "hw_filter", "hw_applied", "hw_clock", "hw_actuator", "hw_sensor"} <= {r["block"] for r in g.snapshot_layout(what)}
    for _ in range(3):
        _period(g), _period(twin)
    assert _differing_rows(_everything(g), _everything(twin)) == []
    bank.save()
    blob = bank.export()
    for _ in range(5):
        _period(g)
    g.reset_robots((np.arange(B) % 2).astype(np.uint8), case["q"] * 0.9, None)
    _period(g)
    bank.load()
    for p in range(5):
        _period(g), _period(twin)
        assert _differing_rows(_everything(g), _everything(twin)) == [], p
    # a masked load: the selected robots go back to period 3, the others run on
    mask = np.arange(B) % 4 == 1
    before = _everything(g)
    bank.load(mask=mask.astype(np.uint8))
    after = _everything(g)
    assert _differing_rows(after[:, ~mask], before[:, ~mask]) == [] and np.all(after[-2, mask] == 3) and np.all(after[-2, ~mask] == 8)
    # a clone of slot 0 into every robot: one state, every robot its own noise from there on
    bank.load(slots=np.zeros(B, dtype=np.int32))
    q0, _ = g.get_state()
    assert np.all(q0 == q0[:, :1])
    _period(g)
    q1, _ = g.get_state()
    assert np.unique(q1[0]).size > B // 2
    # export / import into a fresh context: it continues as the twin did from period 3
    fresh, again = _loop_ctx(case, D, act, sen), _loop_ctx(case, D, act, sen)
    fbank = fresh.snapshot_bank(B, what)
    fbank.import_(blob)
    fbank.load()
    for _ in range(3):
        _period(again)
    for p in range(2):
        _period(fresh), _period(again)
        assert _differing_rows(_everything(fresh), _everything(again)) == [], p
    # another depth: the layout has changed, the first differing block is the history
    g.set_hardware(act, sen, max_delay=D + 1, sensor_task=0, seed=3)
    with pytest.raises(Exception, match="hw_history"):
        bank.load()
    other = _loop_ctx(case, D + 2, act, sen)
    with pytest.raises(Exception, match="hw_history"):
        other.snapshot_bank(B, what).import_(blob)


# ---------------------------------------------------------------------------------------------- 8: device rows, arguments
def test_device_rows_and_rewrites():
    import torch

    B = 130
    case = wc.draw("panda", B)
    D, act, sen = hc.rows("panda", B, "all", sensor=True)
    cmds = hc.commands(case)
    host, dev = _controller(case), _controller(case)
    host.set_hardware(act, sen, max_delay=D, seed=8)
    with torch.cuda.stream(torch.cuda.Stream()):  # a caller stream of its own: the stream contract orders the copies
        ta, ts = torch.from_numpy(act).cuda(), torch.from_numpy(sen).cuda()
        dev.set_hardware(ta, ts, max_delay=D, seed=8)
        ta.zero_(), ts.zero_()  # the caller may overwrite its tensors right after the call
    for c in (host, dev):
        c.set_state(case["q"], case["dq"])
        c.sim_step(cmds[0], hc.DT, hc.SUBSTEPS, False)
    assert np.array_equal(host.get_hardware_state()["applied_torque"], dev.get_hardware_state()["applied_torque"])
    cfg, a, s = dev.get_hardware()
    assert np.array_equal(a, act) and np.array_equal(s, sen) and (cfg.max_delay, cfg.seed, cfg.sensor_task) == (D, 8, -1)
    with pytest.raises(ValueError):
        dev.set_hardware(torch.from_numpy(act).cuda(), sen, max_delay=D)  # host and device rows mixed
    # rows rewritten in place between steps take effect at the next step; a NaN delay acts as 0
    act2 = act.copy()
    act2[0] = np.nan
    act2[1 + 7 : 1 + 14] = 2.0
    act2[1 + 14 :] = 0.0
    act2[1:8] = 1.0
    _to_device(dev, _abi.BUF_HARDWARE_ACTUATOR, act2)
    dev.sim_step(cmds[1], hc.DT, hc.SUBSTEPS, False)
    assert np.array_equal(dev.get_hardware_state()["applied_torque"], 2.0 * cmds[1])


def test_argument_checks_leave_the_context_as_it_was():
    B = 65
    case = wc.draw("panda", B)
    D, act, sen = hc.rows("panda", B, "all", sensor=True)
    g = _controller(case)
    for buf in (_abi.BUF_HARDWARE_ACTUATOR, _abi.BUF_HARDWARE_SENSOR, _abi.BUF_TAU_APPLIED):
        assert not g.device_buffer(buf)
    st = g.get_hardware_state()
    assert not st["applied_torque"].any() and not st["period"].any()
    ia, isen = hr.ideal_rows(7, B)
    cfg, a, s = g.get_hardware()
    assert np.array_equal(a, ia) and np.array_equal(s, isen) and (cfg.max_delay, cfg.sensor_task) == (0, -1)
    g.set_hardware(act, sen, max_delay=D, sensor_task=0, seed=4)
    g.set_state(case["q"], case["dq"])
    g.sim_step(case["tau"], hc.DT, hc.SUBSTEPS, False)
    before = g.get_hardware_state()

    def edit(rows, r, v, col=3):
        out = rows.copy()
        out[r, col] = v
        return out

    bad = [
        (dict(actuator_rows=edit(act, 0, 1.5)), "delay"), (dict(actuator_rows=edit(act, 0, D + 1.0)), "delay"),
        (dict(actuator_rows=edit(act, 0, -1.0)), "delay"), (dict(actuator_rows=edit(act, 0, np.nan)), "delay"),
        (dict(actuator_rows=edit(act, 2, 0.0)), "alpha"), (dict(actuator_rows=edit(act, 2, 1.01)), "alpha"),
        (dict(actuator_rows=edit(act, 2, np.nan)), "alpha"),
        (dict(actuator_rows=edit(act, 9, -0.1)), "gain"), (dict(actuator_rows=edit(act, 9, np.inf)), "gain"),
        (dict(actuator_rows=edit(act, 16, -0.1)), "sigma"), (dict(actuator_rows=edit(act, 16, np.nan)), "sigma"),
        (dict(sensor_rows=edit(sen, 1, np.inf)), "bias"), (dict(sensor_rows=edit(sen, 7, -1.0)), "sensor noise"),
        (dict(sensor_rows=edit(sen, 7, np.nan)), "sensor noise"), (dict(sensor_rows=edit(sen, 12, 0.0)), "alpha_s"),
        (dict(sensor_rows=edit(sen, 12, 1.5)), "alpha_s"),
        (dict(max_delay=9), "max_delay"), (dict(max_delay=-1), "max_delay"), (dict(sensor_task=2), "sensor_task"), (dict(sensor_task=1), None),
    ]
    for kw, word in bad:
        args = dict(actuator_rows=act, sensor_rows=sen, max_delay=D, sensor_task=0, seed=4)
        args.update(kw)
        if word is None:  # task 1 is a MotionForceTask too: accepted; put the first configuration back
            continue
        with pytest.raises((ValueError, RuntimeError), match=word):
            g.set_hardware(**args)
        cfg, a, s = g.get_hardware()
        assert (cfg.max_delay, cfg.sensor_task, cfg.seed) == (D, 0, 4) and np.array_equal(a, act) and np.array_equal(s, sen)
        now = g.get_hardware_state()
        assert all(np.array_equal(now[k], before[k]) for k in before) and g.device_buffer(_abi.BUF_TAU_APPLIED)
    # set / clear / set again: cleared, the context runs what a context without the feature runs
    twin = _controller(case)
    twin.set_state(*g.get_state())
    g.clear_hardware()
    assert not g.device_buffer(_abi.BUF_TAU_APPLIED) and not g.get_hardware_state()["period"].any()
    launches = g.counters()[0]
    for c in (g, twin):
        c.sim_step(case["tau"], hc.DT, hc.SUBSTEPS, False)
    assert g.counters()[0] - launches == 1 and all(np.array_equal(x, y) for x, y in zip(g.get_state(), twin.get_state()))
    g.set_hardware(act, sen, max_delay=D, sensor_task=0, seed=4)
    assert np.all(g.get_hardware_state()["period"] == 0)
    g.sim_step(case["tau"], hc.DT, hc.SUBSTEPS, False)
    ref = hr.HardwareReference(7, B, D, act, sen, seed=4)
    assert np.abs(g.get_hardware_state()["applied_torque"] - ref.actuate(case["tau"])).max() < ROW_TOL
