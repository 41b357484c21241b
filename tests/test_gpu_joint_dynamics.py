"""GPU tests (-m gpu) of the joint dynamics of the simulated plant (csrc/sai2b_sim.hip: sim_joint_kernel<PL, CT>) against
tests/joint_dynamics_reference.py. Inputs: tests/joint_dynamics_cases.py (Panda, planar_4r, six_r, sliding_base with its
prismatic first joint; B = 1, 63, 65, 130 and one case of 4 099; the ranges are those the one-ulp condition of
tests/test_joint_dynamics_reference.py holds for).

1: state after 5 periods of 3 substeps, with and without gravity, every effect alone with the others neutral and then all
   together (a swapped row shows), within the bounds tests/test_gpu_sim.py holds the plain harness to (1e-12, 1e-10).
2: all four instantiations (plain, plant payload, contact with one and four points, both): state, contact status and
   sensor rows with the bounds and the evaluation rule of tests/test_gpu_contact.py.
3: status rows and both counters against the reference at the state the GPU ended in: 1e-12 max(1, |x|max), counts exact.
4: routing (neutral rows against sim_kernel, clear, get_bias, reset_robots).  5: host arrays against device tensors.
6: closed loops."""
import functools

import numpy as np
import pytest

import contact_cases as cc
import joint_dynamics_cases as jc
import joint_dynamics_reference as jr
import oracle_lib as ol
import payload_cases as pc
import plumbing
import sai2_primitives_perso_amd as pkg
from contact_reference import ContactReference
from sai2_primitives_perso_amd import _abi

pytestmark = pytest.mark.gpu

CASES = [(r, B) for r in jc.ROBOTS for B in (1, 63, 65, 130)] + [("panda", 4099)]
STATUS = ("applied_torque", "stop_torque", "dissipative_torque")


def _gpu(case, B):
    return pkg.Controller(case["model"], [pkg.joint_task_config("j", robot_dof=case["n"])], B)


def _steps(g, case, grav, periods=jc.PERIODS):
    g.set_state(case["q"], case["dq"])
    for _ in range(periods):
        g.sim_step(case["tau"], jc.DT, jc.SUBSTEPS, grav)
    return g.get_state()


@functools.lru_cache(maxsize=None)
def _run(robot, B):
    """-> [(effect, gravity, gpu dict, reference dict)]: every effect alone, then all, with and without gravity"""
    case = jc.draw(robot, B)
    g = _gpu(case, B)
    out = []
    for effect in jc.EFFECTS + ("all",):
        rows, k = jc.select(case, effect)
        g.set_joint_dynamics(**jc.keywords(rows, k))
        for grav in (False, True):
            q, dq = _steps(g, case, grav)
            got = g.get_joint_dynamics_state()
            got.update(q=q, dq=dq, saturated_only=g.robots_saturated(), at_stop_only=g.robots_at_stop())
            ref = jc.reference_run(case, rows, k, grav)
            qr, dqr = ref.get_state()
            at_gpu_state = jc.reference(case, rows, k)
            at_gpu_state.load(q, dq, case["tau"])
            rep = at_gpu_state.report()
            rep.update(q=qr, dq=dqr, clear=jc.clear_of_stops(case, rows, qr))
            out.append((effect, grav, got, rep))
    return out


@pytest.mark.parametrize("robot, B", CASES)
def test_state_follows_the_reference(robot, B):
    for effect, grav, got, ref in _run(robot, B):
        eq, ev = np.abs(got["q"] - ref["q"]).max(), np.abs(got["dq"] - ref["dq"]).max()
        print(f"1 {robot} B={B} {effect} gravity={grav}: |dq| {eq:.2e} |ddq| {ev:.2e} saturated {ref['robots_saturated']} "
              f"at a stop {ref['robots_at_stop']}")
        assert eq < 1e-12 and ev < 1e-10, (effect, grav, eq, ev)
    if B >= 63:  # the effects are there: a good share saturates, about a third stands at a stop
        by = {(e, gr): r for e, gr, _, r in _run(robot, B)}
        assert by[("all", True)]["robots_saturated"] > B // 2 and by[("torque_limit", True)]["robots_saturated"] > B // 2
        assert B // 8 < by[("limits", True)]["robots_at_stop"] < B and by[("damping", True)]["robots_at_stop"] == 0


@pytest.mark.parametrize("robot, B", CASES)
def test_status_rows_and_counters(robot, B):
    for effect, grav, got, ref in _run(robot, B):
        assert ref["clear"], "a final q within 1e-9 of a stop: draw other inputs"
        for key in STATUS:
            tol = 1e-12 * max(1.0, np.abs(ref[key]).max())
            err = np.abs(got[key] - ref[key]).max()
            print(f"3 {robot} B={B} {effect} gravity={grav} {key}: {err:.2e} (tol {tol:.2e})")
            assert err < tol, (effect, grav, key, err, tol)
        assert got["robots_saturated"] == ref["robots_saturated"] == got["saturated_only"], (effect, grav)
        assert got["robots_at_stop"] == ref["robots_at_stop"] == got["at_stop_only"], (effect, grav)


# ---- 2: the four instantiations
FRAME_POS = (0.01, 0.02, 0.06)
SENSOR_POS = (0.0, 0.01, -0.03)
SENSOR_ROT = [np.cos(0.4), -np.sin(0.4), 0, np.sin(0.4), np.cos(0.4), 0, 0, 0, 1]


def _tasks(mk_mft, mk_jt, link, n):
    mft = mk_mft("m", link=link, frame_pos=FRAME_POS, robot_dof=n)
    mft.sensor_rot[:] = SENSOR_ROT
    mft.sensor_pos[:] = SENSOR_POS
    return [mft, mk_jt("j", robot_dof=n)]


@pytest.mark.parametrize("robot, n_points", [("panda", 1), ("panda", 4), ("sliding_base", 4), ("planar_4r", 1)])
def test_all_four_instantiations(robot, n_points):
    B = 130
    con = cc.draw(robot, B, n_points)
    case = jc.draw(robot, B)
    n, link = case["n"], con["link"]
    # the contact case's poses (its planes are placed against them), a third pushed beyond the joint limits of this case
    case["q"], case["dq"] = con["q"].copy(), con["dq"]
    jc.push_beyond(case["q"], case["rows"], np.random.default_rng(B + n_points))
    rows, k = jc.select(case, "all")
    g = pkg.Controller(case["model"], _tasks(pkg.motion_force_task_config, pkg.joint_task_config, link, n), B)
    sensor_oracle = ol.Oracle(case["model"], _tasks(ol.motion_force_task, ol.joint_task, link, n), B, threads=8)
    g.set_joint_dynamics(**jc.keywords(rows, k))
    r = con["rows"]
    for payload in (False, True):
        if payload:
            g.set_link_payload(link, *pc.model_rows(robot, link, *pc.rows(B)), target="plant")
        for contact in (False, True):
            if contact:
                g.set_contact(link, con["points"], r[0:3], r[3:6], r[6], r[7], r[8], sensor_task=0, friction_velocity_eps=cc.V_EPS)
            else:
                g.clear_contact()
            plant = pc.PayloadOracles(pc.texts(robot, link), sensor_oracle.tasks, B) if payload else None
            cref = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS) if contact else None
            ref = jc.reference_run(case, rows, k, True, plant=plant, contact=cref)
            q, dq = _steps(g, case, True)
            qr, dqr = ref.get_state()
            eq, ev = np.abs(q - qr).max(), np.abs(dq - dqr).max()
            at = jc.reference(case, rows, k)
            at.load(q, dq, case["tau"])
            rep, got = at.report(), g.get_joint_dynamics_state()
            print(f"2 {robot} points={n_points} payload={payload} contact={contact}: |dq| {eq:.2e} |ddq| {ev:.2e} at a stop "
                  f"{rep['robots_at_stop']} saturated {rep['robots_saturated']}")
            assert eq < 1e-12 and ev < 1e-10, (payload, contact, eq, ev)
            for key in STATUS:
                assert np.abs(got[key] - rep[key]).max() < 1e-12 * max(1.0, np.abs(rep[key]).max()), (payload, contact, key)
            assert (got["robots_saturated"], got["robots_at_stop"]) == (rep["robots_saturated"], rep["robots_at_stop"])
            if contact:  # the evaluation rule of tests/test_gpu_contact.py: the rows describe the state the GPU ended in
                cat = ContactReference(case["model"], B, link, con["points"], r, cc.V_EPS)
                cat.set_state(q, dq)
                crep, cgot = cat.report(sensor=(sensor_oracle, 0)), g.get_contact_state()
                cgot["sensed"] = plumbing.device_rows(g, _abi.BUF_SENSED, 0, 6)
                tol = 1e-12 * max(1.0, np.abs(crep["wrench_world"][:3]).max(), crep["normal_force"].max())
                errs = {key: np.abs(cgot[key] - crep[key]).max() for key in ("depth", "normal_force", "wrench_world", "sensed")}
                print(f"2 contact rows: tol {tol:.2e} {errs} in contact {crep['robots_in_contact']}")
                assert all(e < tol for e in errs.values()), (payload, errs, tol)
                assert cgot["robots_in_contact"] == crep["robots_in_contact"] and 0 < crep["robots_in_contact"] < B


# ---- 4: routing
def test_routing():
    B = 130
    case = jc.draw("panda", B)
    n = case["n"]
    g, bare = _gpu(case, B), _gpu(case, B)
    assert not g.device_buffer(_abi.BUF_JOINT_DYNAMICS) and not g.device_buffer(_abi.BUF_JOINT_DYNAMICS_STATE)
    cfg0, rows0 = g.get_joint_dynamics()
    assert np.array_equal(rows0, jr.rows_array(n, B)) and list(cfg0.friction_velocity_eps[:n]) == [1e-2] * n
    st = g.get_joint_dynamics_state()
    assert st["robots_saturated"] == 0 and st["robots_at_stop"] == 0 and not any(st[key].any() for key in STATUS)
    free = _steps(bare, case, True)
    # neutral rows through sim_joint_kernel against sim_kernel on the twin
    g.set_joint_dynamics()
    assert g.device_buffer(_abi.BUF_JOINT_DYNAMICS) and g.device_buffer(_abi.BUF_JOINT_DYNAMICS_STATE)
    assert np.array_equal(g.get_joint_dynamics()[1], rows0)
    neutral = _steps(g, case, True)
    assert np.abs(neutral[0] - free[0]).max() < 1e-12 and np.abs(neutral[1] - free[1]).max() < 1e-10
    st = g.get_joint_dynamics_state()
    assert np.array_equal(st["applied_torque"], case["tau"]) and not st["stop_torque"].any() and not st["dissipative_torque"].any()
    assert st["robots_saturated"] == 0 and st["robots_at_stop"] == 0
    # everything on: another trajectory; sai2b_get_bias is the one of a context without, bit for bit
    rows, k = jc.select(case, "all")
    g.set_joint_dynamics(**jc.keywords(rows, k))
    cfg, back = g.get_joint_dynamics()
    assert np.array_equal(back, rows) and np.array_equal(np.array(cfg.stop_stiffness[:n]), k)
    assert list(cfg.stop_damping[:n]) == [jc.STOP_DAMPING] * n and list(cfg.friction_velocity_eps[:n]) == [jc.V_EPS] * n
    assert np.array_equal(plumbing.device_rows(g, _abi.BUF_JOINT_DYNAMICS, -1, 6 * n).reshape(6, n, B), rows)
    moved = _steps(g, case, True)
    assert np.abs(moved[0] - free[0]).max() > 1e-6 and g.robots_saturated() > B // 2 and g.robots_at_stop() > B // 8
    bare.set_state(*moved)
    assert np.array_equal(g.get_bias(True), bare.get_bias(True)) and np.array_equal(g.get_state()[0], moved[0])
    # reset_robots on a mask keeps every robot's rows and status; an unselected robot's next step is that of a twin without a reset
    twin = _gpu(case, B)
    twin.set_joint_dynamics(**jc.keywords(rows, k))
    assert all(np.array_equal(a, b) for a, b in zip(_steps(twin, case, True), moved))
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    before = g.get_joint_dynamics_state()
    g.reset_robots(mask, case["q"], np.zeros_like(case["dq"]))
    after = g.get_joint_dynamics_state()
    assert np.array_equal(g.get_joint_dynamics()[1], rows) and all(np.array_equal(before[key], after[key]) for key in before)
    g.reinitialize()
    assert np.array_equal(g.get_joint_dynamics()[1], rows)
    g.sim_step(case["tau"], jc.DT, jc.SUBSTEPS, True)
    twin.sim_step(case["tau"], jc.DT, jc.SUBSTEPS, True)
    (qa, va), (qb, vb) = g.get_state(), twin.get_state()
    keep = mask == 0
    assert np.array_equal(qa[:, keep], qb[:, keep]) and np.array_equal(va[:, keep], vb[:, keep])
    assert not np.array_equal(qa[:, ~keep], qb[:, ~keep])
    # clear: sim_kernel again, bit-equal to a context that never set joint dynamics; the status does not outlive it
    g.clear_joint_dynamics()
    assert not g.device_buffer(_abi.BUF_JOINT_DYNAMICS) and not g.device_buffer(_abi.BUF_JOINT_DYNAMICS_STATE)
    st = g.get_joint_dynamics_state()
    assert st["robots_saturated"] == 0 and st["robots_at_stop"] == 0 and not any(st[key].any() for key in STATUS)
    again = _steps(g, case, True)
    assert np.array_equal(again[0], free[0]) and np.array_equal(again[1], free[1])


def test_model_values_and_broadcast():
    """a scalar, [n] and [n][B] are broadcast; torque_limit="model" and limits="model" take the context's model"""
    B = 65
    case = jc.draw("six_r", B)
    n, m = case["n"], case["model"]
    g = _gpu(case, B)
    d = np.linspace(0.5, 3.0, n)
    g.set_joint_dynamics(armature=0.05, damping=d, friction=case["rows"][2], torque_limit="model", limits="model", stop_stiffness=5e3)
    cfg, rows = g.get_joint_dynamics()
    assert np.all(rows[0] == 0.05) and np.array_equal(rows[1], np.broadcast_to(d[:, None], (n, B))) and np.array_equal(rows[2], case["rows"][2])
    for r, field in ((3, m.effort), (4, m.q_lower), (5, m.q_upper)):
        assert np.array_equal(rows[r], np.broadcast_to(np.array(field[:n])[:, None], (n, B)))
    assert list(cfg.stop_stiffness[:n]) == [5e3] * n


# ---- 5: host arrays and device tensors
def test_device_tensors_give_the_same_bits():
    import torch

    B = 130
    case = jc.draw("sliding_base", B)
    rows, k = jc.select(case, "all")
    host, dev = _gpu(case, B), _gpu(case, B)
    kw = jc.keywords(rows, k)
    host.set_joint_dynamics(**kw)
    dev.set_joint_dynamics(**{key: torch.from_numpy(v).cuda() if key in jr.ROWS else v for key, v in kw.items()})
    assert np.array_equal(host.get_joint_dynamics()[1], rows) and np.array_equal(dev.get_joint_dynamics()[1], rows)
    a, b = _steps(host, case, True), _steps(dev, case, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    sa, sb = host.get_joint_dynamics_state(), dev.get_joint_dynamics_state()
    assert all(np.array_equal(sa[key], sb[key]) for key in sa)
    # only some rows given, as tensors: the others are neutral
    dev.set_joint_dynamics(damping=torch.from_numpy(rows[1]).cuda())
    want = jr.rows_array(case["n"], B, damping=rows[1])
    assert np.array_equal(dev.get_joint_dynamics()[1], want)


def test_host_array_validation():
    """the host-array checks of sai2b_set_joint_dynamics, each with its message; a rejected call leaves the context as it was"""
    B = 63
    case = jc.draw("panda", B)
    rows, k = jc.select(case, "all")
    g = _gpu(case, B)
    g.set_joint_dynamics(**jc.keywords(rows, k))

    def bad(r, v):
        a = rows[r].copy()
        a[3, 5] = v
        return {jr.ROWS[r]: a}

    for kw, message in ((bad(0, -1e-3), "armature must be finite and >= 0"), (bad(0, np.inf), "armature must be finite and >= 0"),
                        (bad(1, -1.0), "damping must be finite and >= 0"), (bad(1, np.nan), "damping must be finite and >= 0"),
                        (bad(2, -0.1), "friction must be finite and >= 0"), (bad(2, np.inf), "friction must be finite and >= 0"),
                        (bad(3, 0.0), "torque_limit must be > 0"), (bad(3, -5.0), "torque_limit must be > 0"), (bad(3, np.nan), "torque_limit must be > 0"),
                        (bad(4, np.nan), "must not be NaN"), (bad(5, np.nan), "must not be NaN"),
                        (dict(q_lower=rows[5], q_upper=rows[5]), "q_lower must be below q_upper"),
                        (dict(q_lower=rows[5], q_upper=rows[4]), "q_lower must be below q_upper"),
                        (bad(4, np.inf), "q_lower must be below q_upper"), (bad(5, -np.inf), "q_lower must be below q_upper")):
        with pytest.raises(ValueError, match=message):
            g.set_joint_dynamics(**kw)
    for kw in (dict(stop_stiffness=-1.0), dict(stop_damping=np.nan), dict(friction_velocity_eps=0.0)):
        with pytest.raises(ValueError, match="joint dynamics: "):
            g.set_joint_dynamics(**kw)
    with pytest.raises(ValueError):
        g.set_joint_dynamics(damping=np.zeros((case["n"], B + 1)))
    g.set_joint_dynamics(torque_limit=bad(3, np.inf)[jr.ROWS[3]], q_lower=bad(4, -np.inf)["q_lower"], q_upper=bad(5, np.inf)["q_upper"])  # infinities that are allowed
    g.set_joint_dynamics(**jc.keywords(rows, k))
    with pytest.raises(ValueError):
        g.set_joint_dynamics(**bad(1, -1.0))
    assert np.array_equal(g.get_joint_dynamics()[1], rows)


# ---- 6: closed loops
def _loop_pair(B, seed=11):
    inp = pkg.workloads.make_inputs(3, B=B, seed=seed)
    to = [ol.motion_force_task("m"), ol.joint_task("j")]
    tg = [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")]
    return inp, ol.Oracle(ol.panda_model(), to, B, threads=8), pkg.Controller(pkg.panda_model(), tg, B)


def _start(c, inp):
    c.set_state(inp["q"], np.zeros_like(inp["q"]))
    c.reinitialize()
    c.set_mft_goals(0, inp["mft0"]["pos"], inp["mft0"]["rot"], None, None, None, None)
    c.set_jt_goals(1, inp["jt1"]["q"], None, None)


def _cpu_loop(o, ref, inp, periods):
    """the oracle's tick plus the reference's step"""
    _start(o, inp)
    ref.set_state(*o.get_state())
    for _ in range(periods):
        tau = o.tick()
        ref.step(tau, 0.001, 1)
        o.set_state(*ref.get_state())
    return ref.get_state()


def test_closed_loop_resident_follows_the_cpu_loop():
    """64 Pandas, the headline hierarchy, 300 periods resident (tick, sim_step(None)) with friction, damping, armature and the
    model's torque limits on, against the same loop on the CPU, under the bound of test_gpu_closed_loop_follows_oracle"""
    B, periods = 64, 300
    inp, o, g = _loop_pair(B)
    rng = np.random.default_rng(3)
    m = ol.panda_model()
    rows = jr.rows_array(7, B, armature=rng.uniform(0, 0.2, (7, B)), damping=rng.uniform(0, 5, (7, B)), friction=rng.uniform(0, 2, (7, B)),
                         torque_limit=np.array(m.effort[:7]))
    ref = jr.JointDynamicsReference(m, B, rows, friction_velocity_eps=jc.V_EPS)
    qc, vc = _cpu_loop(o, ref, inp, periods)
    g.set_joint_dynamics(armature=rows[0], damping=rows[1], friction=rows[2], torque_limit="model", friction_velocity_eps=jc.V_EPS)
    assert np.array_equal(g.get_joint_dynamics()[1], rows)
    _start(g, inp)
    for _ in range(periods):
        g.tick(want_output=False)
        g.sim_step(None, 0.001, 1)
    qg, vg = g.get_state()
    eq, ev = np.abs(qg - qc).max(), np.abs(vg - vc).max()
    print(f"6 resident vs cpu: |dq| {eq:.2e} |ddq| {ev:.2e}")
    assert eq < 1e-9 and ev < 1e-8
    assert np.abs(qg - inp["q"]).max() > 1e-3  # they did move


def test_joint_driven_into_its_upper_stop():
    """Joint 4 of every robot is sent 0.2 rad beyond its upper stop by a JointTask goal; the stop holds it: q_4 ends beyond hi
    by less than t_4 / k_4 (the most the saturated actuator can press the spring in) plus one per cent, a margin the CPU
    loop itself meets, and every robot stands at the stop."""
    B, periods, j = 64, 1500, 3
    m = ol.panda_model()
    t, k = np.array(m.effort[:7]), 2e4
    rng = np.random.default_rng(4)
    hi = np.full((7, B), np.inf)
    hi[j] = rng.uniform(-1.2, -0.8, B)
    q0 = np.tile(np.array([0.0, -0.5, 0.0, -1.8, 0.0, 1.6, 0.5])[:, None], (1, B)) + rng.uniform(-0.05, 0.05, (7, B))
    goal = q0.copy()
    goal[j] = hi[j] + 0.2
    rows = jr.rows_array(7, B, damping=1.0, torque_limit=t, q_upper=hi)
    kw = dict(damping=1.0, torque_limit="model", q_upper=hi, stop_stiffness=k, stop_damping=0.5)
    limit = t[j] / k * 1.01

    def run(c, step):
        c.set_state(q0, np.zeros_like(q0))
        c.reinitialize()
        c.set_jt_goals(0, goal, None, None)
        for _ in range(periods):
            step()
        return c.get_state()[0][j] - hi[j]

    o = ol.Oracle(m, [ol.joint_task("j")], B, threads=8)
    ref = jr.JointDynamicsReference(m, B, rows, k, 0.5)

    def cpu_step():
        ref.set_state(*o.get_state())
        ref.step(o.tick(), 0.001, 1)
        o.set_state(*ref.get_state())

    over_cpu = run(o, cpu_step)
    assert 0 < over_cpu.min() and over_cpu.max() < limit and ref.report()["robots_at_stop"] == B
    g = pkg.Controller(pkg.panda_model(), [pkg.joint_task_config("j")], B)
    g.set_joint_dynamics(**kw)

    def gpu_step():
        g.tick(want_output=False)
        g.sim_step(None, 0.001, 1)

    over = run(g, gpu_step)
    print(f"6 stop: beyond hi by {over.min():.2e} .. {over.max():.2e} rad (cpu {over_cpu.min():.2e} .. {over_cpu.max():.2e}), limit {limit:.2e}")
    assert 0 < over.min() and over.max() < limit
    assert g.robots_at_stop() == B
