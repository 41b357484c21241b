"""GPU tests (-m gpu) of the contact model of the simulated plant and its force / moment sensor (csrc/sai2b_sim.hip:
sim_kernel<PL, Contact>) against tests/contact_reference.py. Inputs: tests/contact_cases.py (Panda, planar_4r, six_r,
sliding_base with its prismatic first joint, rprp_4 with prismatic joints inside the chain; B = 200 and 4 099, a ragged
last wavefront; one and four points; every robot its own plane; the stiffness range is the one the one-ulp condition of
tests/test_contact_reference.py holds for).

A: state after 5 periods of 3 substeps under fixed random torques, with and without gravity and a plant payload (all four
   instantiations), every robot within the bounds tests/test_gpu_sim.py holds the contact-free harness to.
B: sensor rows (SAI2B_BUF_SENSED of the sensor task), get_contact_state and robots_in_contact after those steps:
   1e-12 max(1, largest force in the batch), the count exact. The rows are a function of the final state, and the
   regularised friction has a slope of mu f_n / v_eps (up to 1e5 N per m/s here) in it: the 1e-10 rad/s that A allows
   between the two final states would be worth 1e-5 N. So the reference evaluates its rows at the state the GPU ended
   in (what the rows claim to describe), and the count is also held to the reference's own run.
C: routing (set / clear / buffer id / far planes / device-resident producer / k = 0).
D: the closed loop the feature exists for (tests/contact_loop.py: example 09's scenario with a real surface), resident on
   the device against a host round trip of the sensor reading and against the all-CPU loop.
E: example 07's hierarchy on a four-point plate pressed flat and then tilted by a moment goal, resident on the device:
   the sensed moment rows and the world moment against contact_reference under the bounds of B."""
import functools

import numpy as np
import pytest

import contact_cases as cc
import contact_loop as cl
from contact_reference import ContactReference
import oracle_lib as ol
import payload_cases as pc
import plumbing
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

pytestmark = pytest.mark.gpu

FRAME_POS = (0.01, 0.02, 0.06)
SENSOR_POS = (0.0, 0.01, -0.03)
SENSOR_ROT = [np.cos(0.4), -np.sin(0.4), 0, np.sin(0.4), np.cos(0.4), 0, 0, 0, 1]


def _tasks(mk_mft, mk_jt, link, n):
    mft = mk_mft("m", link=link, frame_pos=FRAME_POS, robot_dof=n)
    mft.sensor_rot[:] = SENSOR_ROT
    mft.sensor_pos[:] = SENSOR_POS
    return [mft, mk_jt("j", robot_dof=n)]


def _gpu(case, B):
    n = int(case["model"].dof)
    return pkg.Controller(case["model"], _tasks(pkg.motion_force_task_config, pkg.joint_task_config, case["link"], n), B)


def _set_contact(g, case, rows=None, sensor_task=0):
    r = case["rows"] if rows is None else rows
    g.set_contact(case["link"], case["points"], r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=sensor_task, friction_velocity_eps=cc.V_EPS)


def _steps(g, case, grav):
    g.set_state(case["q"], case["dq"])
    for _ in range(cc.PERIODS):
        g.sim_step(case["tau"], cc.DT, cc.SUBSTEPS, grav)
    return g.get_state()


@functools.lru_cache(maxsize=None)
def _run(robot, B, n_points):
    """-> [(payload, gravity, gpu dict, reference dict)] for the four combinations"""
    case = cc.draw(robot, B, n_points)
    n = int(case["model"].dof)
    g = _gpu(case, B)
    sensor_oracle = ol.Oracle(case["model"], _tasks(ol.motion_force_task, ol.joint_task, case["link"], n), B, threads=8)
    out = []
    for payload in (False, True):
        if payload:
            # the payloads are defined in the URDF link's frame (payload_cases.texts): the model's link frame has the axis on z
            g.set_link_payload(case["link"], *pc.model_rows(robot, case["link"], *pc.rows(B)), target="plant")
        for grav in (False, True):
            def run(c):
                plant = pc.PayloadOracles(pc.texts(robot, case["link"]), sensor_oracle.tasks, B) if payload else None
                return cc.reference_run(c, grav, plant=plant)

            ref = cc.settle_count(case, run)
            own = ref.report()
            _set_contact(g, case)
            q, dq = _steps(g, case, grav)
            at_gpu_state = cc.ContactReference(case["model"], B, case["link"], case["points"], case["rows"], cc.V_EPS)
            at_gpu_state.set_state(q, dq)
            rep = at_gpu_state.report(sensor=(sensor_oracle, 0))
            rep["q"], rep["dq"] = ref.get_state()
            rep["count_of_own_run"] = own["robots_in_contact"]
            got = g.get_contact_state()
            got.update(q=q, dq=dq, sensed=plumbing.device_rows(g, _abi.BUF_SENSED, 0, 6), count_only=g.robots_in_contact())
            out.append((payload, grav, got, rep))
    return out


CASES = [(r, B, k) for r in cc.ROBOTS for B in (200, 4099) for k in (1, 4)]


@pytest.mark.parametrize("robot, B, n_points", CASES)
def test_state_follows_the_reference(robot, B, n_points):
    for payload, grav, got, ref in _run(robot, B, n_points):
        eq, ev = np.abs(got["q"] - ref["q"]).max(), np.abs(got["dq"] - ref["dq"]).max()
        print(f"A {robot} B={B} points={n_points} payload={payload} gravity={grav}: |dq| {eq:.2e} |ddq| {ev:.2e} "
              f"in contact {ref['robots_in_contact']}")
        assert B // 4 < ref["robots_in_contact"] < B
        assert eq < 1e-12 and ev < 1e-10, (payload, grav, eq, ev)


@pytest.mark.parametrize("robot, B, n_points", CASES)
def test_sensor_and_status_rows(robot, B, n_points):
    for payload, grav, got, ref in _run(robot, B, n_points):
        tol = 1e-12 * max(1.0, np.abs(ref["wrench_world"][:3]).max(), ref["normal_force"].max())
        errs = {k: np.abs(got[k] - ref[k]).max() for k in ("depth", "normal_force", "wrench_world", "sensed")}
        print(f"B {robot} B={B} points={n_points} payload={payload} gravity={grav}: tol {tol:.2e} {errs}")
        assert all(e < tol for e in errs.values()), (payload, grav, errs, tol)
        assert got["robots_in_contact"] == ref["robots_in_contact"] == got["count_only"] == ref["count_of_own_run"]
        assert np.all(got["depth"][n_points:] == 0) and np.all(got["normal_force"][n_points:] == 0)


def test_routing():
    B = 200
    case = cc.draw("panda", B, 4)
    g, bare = _gpu(case, B), _gpu(case, B)
    assert not g.device_buffer(_abi.BUF_CONTACT) and g.get_contact()[0].n_points == 0 and g.robots_in_contact() == 0
    free = _steps(bare, case, True)
    # set -> clear: the kernel and the states of a context that never had contact
    _set_contact(g, case)
    assert g.device_buffer(_abi.BUF_CONTACT)
    cfg, rows = g.get_contact()
    assert (cfg.link, cfg.n_points, cfg.sensor_task) == (case["link"], 4, 0) and np.array_equal(rows, case["rows"])
    touched = _steps(g, case, True)
    assert np.abs(touched[0] - free[0]).max() > 1e-6 and g.robots_in_contact() > B // 4
    # sai2b_get_bias never sees the contact: the bias of a context without one at the same state, bit for bit
    bare.set_state(*touched)
    assert np.array_equal(g.get_bias(True), bare.get_bias(True)) and np.array_equal(g.get_state()[0], touched[0])
    g.clear_contact()
    assert not g.device_buffer(_abi.BUF_CONTACT) and g.get_contact()[0].n_points == 0
    st = g.get_contact_state()  # the status of the last step with a contact does not outlive it
    assert st["robots_in_contact"] == 0 and not st["normal_force"].any() and not st["depth"].any() and not st["wrench_world"].any()
    again = _steps(g, case, True)
    assert np.array_equal(again[0], free[0]) and np.array_equal(again[1], free[1])
    # planes a metre clear of every robot: the contact-FREE oracle within the bounds of A, nobody in contact
    far = case["rows"].copy()
    x, _, _ = cc.ContactReference(case["model"], B, case["link"], case["points"], far, cc.V_EPS).point_kinematics(case["q"], case["dq"])
    far[0:3] = far[3:6] * (np.einsum("ib,kib->kb", far[3:6], x).min(axis=0) - 1.0)  # one metre under the lowest point
    _set_contact(g, case, far)
    got = _steps(g, case, True)
    o = ol.Oracle(case["model"], [ol.joint_task("j", robot_dof=7)], B, threads=8)
    o.set_state(case["q"], case["dq"])
    for _ in range(cc.PERIODS):
        o.sim_step(case["tau"], cc.DT, cc.SUBSTEPS, True)
    qo, vo = o.get_state()
    assert np.abs(got[0] - qo).max() < 1e-12 and np.abs(got[1] - vo).max() < 1e-10
    st = g.get_contact_state()
    assert st["robots_in_contact"] == 0 and np.all(st["normal_force"] == 0) and np.all(st["depth"][:4] < -0.9)
    assert np.all(plumbing.device_rows(g, _abi.BUF_SENSED, 0, 6) == 0)
    # k = 0 rows are inert: those robots move as the free ones, the others as before
    half = case["rows"].copy()
    half[6, ::2] = 0
    _set_contact(g, case, half)
    got = _steps(g, case, True)
    assert np.abs(got[0][:, ::2] - free[0][:, ::2]).max() < 1e-12 and np.abs(got[1][:, ::2] - free[1][:, ::2]).max() < 1e-10
    assert np.array_equal(got[0][:, 1::2], touched[0][:, 1::2])
    assert np.all(g.get_contact_state()["normal_force"][:, ::2] == 0)
    # a device-resident producer rewriting the rows through the buffer id between two steps is obeyed by the second
    import torch

    _set_contact(g, case, far)
    g.set_state(case["q"], case["dq"])
    g.sim_step(case["tau"], cc.DT, cc.SUBSTEPS, True)
    assert g.robots_in_contact() == 0
    p = g.device_buffer(_abi.BUF_CONTACT)

    class _Raw:  # zero-copy torch view of the library's contact rows
        __cuda_array_interface__ = {"data": (int(p), False), "shape": (9, B), "typestr": "<f8", "version": 2}

    g.synchronize()
    torch.as_tensor(_Raw(), device="cuda").copy_(torch.as_tensor(case["rows"], device="cuda"))
    torch.cuda.synchronize()
    g.set_state(case["q"], case["dq"])
    for _ in range(cc.PERIODS):
        g.sim_step(case["tau"], cc.DT, cc.SUBSTEPS, True)
    got = g.get_state()
    assert np.array_equal(got[0], touched[0]) and np.array_equal(got[1], touched[1])
    # sai2b_set_mft_sensed_wrench keeps working on the sensor task: last writer wins
    f = np.full((3, B), 2.5)
    g.set_mft_sensed_wrench(0, f, -f)
    assert np.array_equal(plumbing.device_rows(g, _abi.BUF_SENSED, 0, 6), np.concatenate([f, -f]))
    # tensors as arguments, and the validation of host arrays
    r = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (case["rows"][0:3], case["rows"][3:6], case["rows"][6], case["rows"][7], case["rows"][8])]
    g.set_contact(case["link"], case["points"], *r, sensor_task=0)
    assert np.array_equal(g.get_contact()[1], case["rows"])
    rows = case["rows"]
    bad = lambda a, v: (lambda x: (x.__setitem__((..., 5), v), x)[1])(a.copy())
    for args in ((rows[0:3], rows[3:6] * 1.001, rows[6]), (bad(rows[0:3], np.nan), rows[3:6], rows[6]), (rows[0:3], rows[3:6], bad(rows[6], -1.0)),
                 (rows[0:3], rows[3:6], rows[6], bad(rows[7], -0.1)), (rows[0:3], rows[3:6], rows[6], rows[7], bad(rows[8], np.inf))):
        with pytest.raises(ValueError):
            g.set_contact(case["link"], case["points"], *args)
    for link, pts, sensor in ((7, case["points"], 0), (6, np.zeros((5, 3)), 0), (6, case["points"], 1)):
        with pytest.raises(ValueError):
            g.set_contact(link, pts, rows[0:3], rows[3:6], rows[6], sensor_task=sensor)
    assert np.array_equal(g.get_contact()[1], case["rows"])  # a rejected call leaves the contact as it was


def _gpu_loop(inp, B, sensor_task):
    cfgs = cl.configs(pkg.motion_force_task_config, pkg.joint_task_config)
    g = pkg.Controller(pkg.panda_model(), cfgs, B)
    r = inp["rows"]
    g.set_contact(cl.LINK, cl.POINT, r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=sensor_task, friction_velocity_eps=cl.V_EPS)
    return g, cfgs


def test_closed_force_loop_resident_against_round_trip_and_cpu():
    """B = 64, 300 periods (the one-ulp condition holds there for the CPU loop: 1e-15 / 2e-14, asserted in
    tests/test_contact_reference.py): the resident loop (tick, sim_step(None), nothing else: the simulation kernel writes
    the sensor task's sensed rows), the loop with the sensor detached and the reading computed on the host from the
    fetched state by contact_reference and uploaded with set_mft_sensed_wrench, and the all-CPU loop (oracle tick +
    contact_reference) end within the closed-loop bounds of test_gpu_closed_loop_follows_oracle (1e-9, 1e-8)."""
    B, periods = 64, 300
    inp = cl.inputs(B)
    cpu = cl.CpuLoop(inp, B)
    qc, vc, sc = cpu.run(inp, periods)
    assert sc is not None and 30 < sc < periods - 100 and cpu.in_contact() == B  # contact, then a stretch of force control
    # resident
    g, cfgs = _gpu_loop(inp, B, 0)
    qr, vr, sr = cl.run(g, cfgs[0], inp, periods, lambda: None, g.robots_in_contact)
    assert sr == sc and g.robots_in_contact() == B
    # sensor detached, reading through the host
    g2, cfgs2 = _gpu_loop(inp, B, -1)
    o2 = ol.Oracle(ol.panda_model(), cl.configs(ol.motion_force_task, ol.joint_task), B, threads=8)
    ref2 = ContactReference(ol.panda_model(), B, cl.LINK, cl.POINT, inp["rows"], cl.V_EPS, threads=8)

    def round_trip():
        ref2.set_state(*g2.get_state())
        rep = ref2.report(sensor=(o2, 0))
        g2.set_mft_sensed_wrench(0, np.ascontiguousarray(rep["sensed"][:3]), np.ascontiguousarray(rep["sensed"][3:]))

    qh, vh, sh = cl.run(g2, cfgs2[0], inp, periods, round_trip, g2.robots_in_contact)
    assert sh == sc
    for name, (q, v) in (("round trip", (qh, vh)), ("cpu", (qc, vc))):
        eq, ev = np.abs(qr - q).max(), np.abs(vr - v).max()
        print(f"D resident vs {name}: |dq| {eq:.2e} |ddq| {ev:.2e} (switch at period {sc})")
        assert eq < 1e-9 and ev < 1e-8, (name, eq, ev)
    assert np.abs(qr - inp["q"]).max() > 1e-3  # they did move


# The CPU loop (tests/contact_loop.py, B = 64) settles slowly: after the impact a few robots swing about the goal force for
# seconds. Largest |f_n - 5 N| over the batch, final state / over the previous 1 000 periods: 5 000 periods 0.60 / 2.9 N,
# 10 000: 1.46 / 1.66, 16 000: 0.11 / 0.34, 20 000: 0.049 / 0.073, 24 000: 0.014 / 0.022, 30 000: 0.0004 / 0.004. Settled is
# taken as: within 0.1 N (2 % of the goal) over the previous 1 000 periods, first met at 20 000.
CPU_SETTLE_PERIODS, CPU_FORCE_DISTANCE = 20000, 0.049479


def test_closed_force_loop_resident_settles():
    """B = 1 024 resident for as many periods as the CPU loop needs to settle (20 000, see above; its largest distance of
    the sensed normal force from -5 N is then 0.049479 N): every robot ends in contact and within twice that distance (the
    factor two covers the different robots of the larger batch, not rounding). The all-CPU loop on these 1 024 robots ends
    at 0.088 N."""
    B = 1024
    inp = cl.inputs(B)
    g, cfgs = _gpu_loop(inp, B, 0)
    _, _, s = cl.run(g, cfgs[0], inp, CPU_SETTLE_PERIODS, lambda: None, g.robots_in_contact)
    st = g.get_contact_state()
    dist = np.abs(st["normal_force"][0] + cl.GOAL_FORCE)
    print(f"D settle: switch at {s}, in contact {st['robots_in_contact']} / {B}, largest |f_n - 5| {dist.max():.4f} N (CPU: {CPU_FORCE_DISTANCE})")
    assert s is not None and st["robots_in_contact"] == B
    assert dist.max() <= 2 * CPU_FORCE_DISTANCE


def test_plate_pressed_flat_then_tilted_by_a_moment_goal():
    """tests/contact_loop.py, plate scenario (example 07's hierarchy: full MotionForceTask parametrised in its compliant
    frame, force along its z, moments about its x and y, closed loop both, passivity on, sensor at the link origin 0.22 m
    behind the control point, so that sensor_pos enters the moment rows), four contact points, B = 200 resident on the
    device: sinking until every plate touches, 400 periods pressed flat with 10 N and zero goal moment, 400 periods
    with a goal moment of 0.25 N m about the frame's x. The rows the simulation kernel wrote after the last step
    (SAI2B_BUF_SENSED of the task, get_contact_state) against contact_reference at the state the GPU ended in, under the
    bounds of B: 1e-12 max(1, largest force in the batch). Not vacuous: the plates carry moments (median sensed |m| above
    0.05 N m), some robots stand on two or three corners only, and a one-point reading (the net force applied at the
    plate's centre) misses the moment rows by orders of magnitude."""
    B = 200
    inp = cl.plate_inputs(B)
    cfgs = cl.plate_configs(pkg.motion_force_task_config, pkg.joint_task_config)
    g = pkg.Controller(pkg.panda_model(), cfgs, B)
    r = inp["rows"]
    g.set_contact(cl.LINK, cl.PLATE_POINTS, r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=0, friction_velocity_eps=cl.V_EPS)
    q, dq, s = cl.run_plate(g, cfgs[0], inp, lambda: None, g.robots_in_contact)
    got = g.get_contact_state()
    sensed = plumbing.device_rows(g, _abi.BUF_SENSED, 0, 6)
    o = ol.Oracle(ol.panda_model(), cl.plate_configs(ol.motion_force_task, ol.joint_task), B, threads=8)
    ref = ContactReference(ol.panda_model(), B, cl.LINK, cl.PLATE_POINTS, r, cl.V_EPS, threads=8)
    ref.set_state(q, dq)
    rep = ref.report(sensor=(o, 0))
    tol = 1e-12 * max(1.0, np.abs(rep["wrench_world"][:3]).max(), rep["normal_force"].max())
    errs = dict(sensed_force=np.abs(sensed[:3] - rep["sensed"][:3]).max(), sensed_moment=np.abs(sensed[3:] - rep["sensed"][3:]).max(),
                world_moment=np.abs(got["wrench_world"][3:] - rep["wrench_world"][3:]).max(),
                normal_force=np.abs(got["normal_force"] - rep["normal_force"]).max())
    touching = (rep["normal_force"] > 0).sum(axis=0)
    m = np.linalg.norm(rep["sensed"][3:], axis=0)
    print(f"E: switch at {s}, in contact {got['robots_in_contact']} / {B}, corners touching {np.bincount(touching, minlength=5)}, "
          f"median |m_s| {np.median(m):.3f} N m, tol {tol:.2e}, {errs}")
    assert got["robots_in_contact"] == rep["robots_in_contact"] and got["robots_in_contact"] > B // 2
    assert np.median(m) > 0.05 and np.count_nonzero((touching > 0) & (touching < 4)) > 0
    assert all(e < tol for e in errs.values()), (errs, tol)
    # what a one-point implementation would report: the net force applied at the control point, no moment about it
    Rc = o.get_model(0)[3].reshape(3, 3, B)
    f_c = np.einsum("jib,jb->ib", Rc, rep["wrench_world"][:3])
    one_point = np.cross(np.array(cfgs[0].sensor_pos[:])[:, None], f_c, axis=0)  # m_s = R_s^T (-(x_c - o_s) x sum F), sensor_rot = 1
    assert np.median(np.abs(one_point - rep["sensed"][3:]).max(axis=0)) > 1e6 * tol
