"""CPU tests of tests/contact_reference.py, the reference the GPU contact tests are held to: it is checked against known
answers (which pins the specification itself), against an independent numpy kinematics, and the inputs of the GPU tests
are checked for the conditioning their bounds assume."""
import numpy as np
import pytest

import contact_cases as cc
import hp_fixture
import oracle_lib as ol
import sai2_primitives_perso_amd as pkg
import urdf_np
from contact_reference import ContactReference, force_law


def _states(robot, B, seed):
    case = cc.draw(robot, B, 4, seed)
    return case, ContactReference(case["model"], B, case["link"], case["points"], case["rows"], cc.V_EPS)


@pytest.mark.parametrize("robot", cc.ROBOTS)
def test_point_kinematics_agree_with_independent_numpy_chain(robot):
    """x_k and J_k from the oracle against tests/urdf_np.py (xml.etree + the URDF's own semantics): 1e-12. The model's
    link frames have the joint axis folded onto z, the URDF's need not: the points are carried over by the loader's own
    sai2b_urdf_resolve_frame (frame of the named URDF link in the model's moving link)."""
    B = 12
    case, ref = _states(robot, B, 1)
    chain = urdf_np.Chain(hp_fixture.urdf_text(robot), is_file=False)
    name = chain.moving[case["link"]]["child"]
    _, links = pkg.model_from_urdf(hp_fixture.urdf_text(robot), is_file=False)
    idx, pos, R = pkg.resolve_link_frame(links, name)
    assert idx == case["link"]
    in_urdf_link = [R.T @ (c - pos) for c in case["points"]]
    x, J, v = ref.point_kinematics(case["q"], case["dq"])
    for b in range(B):
        for k, c in enumerate(in_urdf_link):
            Jn, xn, _ = chain.jacobian(case["q"][:, b], name, c)
            assert np.abs(xn - x[k, :, b]).max() < 1e-12
            assert np.abs(Jn[:3] - J[k, :, :, b]).max() < 1e-12
            assert np.abs(Jn[:3] @ case["dq"][:, b] - v[k, :, b]).max() < 1e-12


@pytest.mark.parametrize("robot", ["panda", "rprp_4"])
def test_contact_torque_is_minus_the_gradient_of_the_elastic_potential(robot):
    """d = mu = 0: sum_k J_k^T F_k = -dV/dq with V = 1/2 k sum_k max(0, delta_k)^2, by central differences of V over q
    through the oracle's forward kinematics. Step s = 1e-6 rad (m): the truncation error is s^2 / 6 |V'''| with
    V''' ~ k (|J| |H| + ...) <= 2e4 * O(10) -> ~ 3e-8, the rounding error eps V / s ~ 2e-16 * 1 / 1e-6 = 2e-10 per
    unit of V (V <= 1/2 * 2e4 * 0.1^2 = 100) -> 2e-8; V is only C1 where a point crosses delta = 0, so the planes are
    moved until every |delta| > 1e-4 >> s |J|. Bound: 1e-6 max(1, largest contact torque)."""
    B = 40
    case, ref = _states(robot, B, 2)
    rows = ref.rows
    rows[7:9] = 0
    q, zero = case["q"], np.zeros_like(case["q"])
    for _ in range(8):
        d = ref.forces(q, zero)["delta"]
        near = (np.abs(d) <= 1e-4).any(axis=0)
        if not near.any():
            break
        rows[0:3, near] += 3e-4 * rows[3:6, near]
    assert not near.any()

    def V(qq):
        x, _, _ = ref.point_kinematics(qq, zero)
        return 0.5 * rows[6] * sum(np.maximum(0.0, np.sum(rows[3:6] * (rows[0:3] - xk), axis=0)) ** 2 for xk in x)

    tau = ref.forces(q, zero)["tau"]
    assert np.count_nonzero(np.abs(tau).max(axis=0) > 0) > B // 3  # the case does press on something
    s = 1e-6
    for i in range(ref.dof):
        e = np.zeros_like(q)
        e[i] = s
        grad = (V(q + e) - V(q - e)) / (2 * s)
        assert np.abs(tau[i] + grad).max() < 1e-6 * max(1.0, np.abs(tau).max()), i


def test_force_law_is_continuous_at_its_three_seams():
    """delta = 0 (touch-down / lift-off), vn = 1 / d (the damping term would pull) and v_t = 0 (Coulomb friction's
    discontinuity, regularised): the one-sided limits agree to rounding"""
    rng = np.random.default_rng(5)
    B = 500
    n = rng.normal(size=(3, B))
    n /= np.linalg.norm(n, axis=0)
    t = rng.normal(size=(3, B))
    t -= np.sum(t * n, axis=0) * n
    t /= np.linalg.norm(t, axis=0)
    rows = np.zeros((9, B))
    rows[3:6], rows[6], rows[7], rows[8] = n, rng.uniform(*cc.K_RANGE, B), rng.uniform(0.05, 0.5, B), rng.uniform(0.1, 0.8, B)
    v = rng.normal(0, 0.5, (3, B))
    # delta = 0: the plane through the origin, the point a hair inside and outside (exact: no cancellation against p0)
    _, _, Fin = force_law(-1e-30 * n, v, rows, cc.V_EPS)
    _, fo, Fout = force_law(+1e-30 * n, v, rows, cc.V_EPS)
    assert np.all(fo == 0) and np.all(Fout == 0) and np.abs(Fin).max() < 1e-20
    # vn = 1 / d, 5 mm inside
    x = -5e-3 * n
    scale = rows[6] * 5e-3 * (1 + rows[8])
    vt = 0.2 * t
    lo, hi = (1 - 1e-14) / rows[7], (1 + 1e-14) / rows[7]
    _, _, Fa = force_law(x, lo * n + vt, rows, cc.V_EPS)
    _, fb, Fb = force_law(x, hi * n + vt, rows, cc.V_EPS)
    assert np.all(fb == 0) and np.abs(Fa - Fb).max() < 1e-12 * scale.max()
    # v_t = 0
    _, fa, Fa = force_law(x, -0.1 * n + 1e-18 * t, rows, cc.V_EPS)
    _, _, Fb = force_law(x, -0.1 * n - 1e-18 * t, rows, cc.V_EPS)
    _, _, F0 = force_law(x, -0.1 * n, rows, cc.V_EPS)
    assert np.abs(Fa - Fb).max() < 1e-12 * fa.max() and np.abs(Fa - F0).max() < 1e-12 * fa.max()
    assert np.abs(F0 - fa * n).max() < 1e-12 * fa.max()  # no friction at rest


def test_contact_dissipates():
    """d, mu > 0: the contact power F . v minus the elastic part k delta vn (= -dV/dt) is <= 0 on 10 000 random states.
    (1 - d vn >= 0: -k delta d vn^2 - friction; otherwise f_n = 0 and vn > 0.) Slack: rounding of the two products."""
    rng = np.random.default_rng(6)
    B = 10000
    rows = np.zeros((9, B))
    n = rng.normal(size=(3, B))
    rows[3:6] = n / np.linalg.norm(n, axis=0)
    rows[0:3] = rng.normal(0, 0.5, (3, B))
    rows[6], rows[7], rows[8] = rng.uniform(*cc.K_RANGE, B), rng.uniform(1e-3, 0.5, B), rng.uniform(1e-3, 0.8, B)
    x = rows[0:3] - rng.uniform(-0.01, 0.03, B) * rows[3:6] + 0.1 * rng.normal(size=(3, B))
    v = rng.normal(0, 2.0, (3, B))  # fast enough that vn > 1 / d occurs
    delta, fn, F = force_law(x, v, rows, cc.V_EPS)
    vn = np.sum(rows[3:6] * v, axis=0)
    assert np.count_nonzero(fn > 0) > B // 4 and np.count_nonzero((delta > 0) & (fn == 0)) > 10
    elastic = rows[6] * np.maximum(0.0, delta) * vn
    power = np.sum(F * v, axis=0)
    slack = 16 * np.finfo(float).eps * (np.abs(elastic) + np.sum(np.abs(F * v), axis=0))
    assert np.all(power - elastic <= slack)
    assert np.all(F[:, delta <= 0] == 0)


def _controller_oracle(B, link, n):
    """the hierarchy whose first task carries the sensor: a sensor frame rotated and offset from the control frame"""
    mft = ol.motion_force_task("m", link=link, frame_pos=(0.01, 0.02, 0.06), robot_dof=n)
    a = 0.4
    mft.sensor_rot[:] = [np.cos(a), -np.sin(a), 0, np.sin(a), np.cos(a), 0, 0, 0, 1]
    mft.sensor_pos[:] = [0.0, 0.01, -0.03]
    return ol.Oracle(cc.model("panda"), [mft, ol.joint_task("j", robot_dof=n)], B)


def test_sensor_rows_invert_the_tasks_own_transform():
    """the sensed rows, pushed through the oracle's get_mft_status (MotionForceTask.cpp:805-828), give back -sum F_k and
    the moment about the control point: 1e-12"""
    B = 60
    case, ref = _states("panda", B, 3)
    ref.set_state(case["q"], case["dq"])
    o = _controller_oracle(B, case["link"], ref.dof)
    rep = ref.report(sensor=(o, 0))
    assert rep["robots_in_contact"] > B // 3
    o.set_mft_sensed_wrench(0, rep["sensed"][:3], rep["sensed"][3:])
    st = o.get_mft_status(0)
    assert np.abs(st["sensed_force"] + rep["wrench_world"][:3]).max() < 1e-12 * max(1.0, np.abs(rep["wrench_world"]).max())
    assert np.abs(st["sensed_moment"] + rep["wrench_world"][3:]).max() < 1e-12 * max(1.0, np.abs(rep["wrench_world"]).max())
    # and the moment is the one about the control point
    f = ref.forces(*ref.get_state())
    _, _, xc, _ = o.get_model(0)
    M = sum(np.cross(f["x"][k] - xc, f["F"][k], axis=0) for k in range(4))
    assert np.abs(M - rep["wrench_world"][3:]).max() < 1e-12


@pytest.mark.parametrize("B", [200, 4099])
@pytest.mark.parametrize("n_points", [1, 4])
@pytest.mark.parametrize("robot", cc.ROBOTS)
def test_inputs_of_the_gpu_tests_are_well_conditioned(robot, n_points, B):
    """The bounds of tests/test_gpu_contact.py (|dq| 1e-12, |ddq| 1e-10 after 5 periods of 3 substeps) assume that the map
    from the initial state to the final one does not amplify a rounding: the reference started one ulp away in every
    component of q and dq ends within a tenth of those bounds of the unperturbed run, with and without gravity, over the
    ranges of contact_cases (whose k was narrowed until this holds: see there)."""
    case = cc.draw(robot, B, n_points)
    for grav in (False, True):
        a = cc.reference_run(case, grav).get_state()
        b = cc.reference_run(case, grav, q=np.nextafter(case["q"], np.inf), dq=np.nextafter(case["dq"], np.inf)).get_state()
        dq_, ddq_ = np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()
        print(f"{robot} points={n_points} gravity={grav}: one-ulp start -> |dq| {dq_:.2e} |ddq| {ddq_:.2e}")
        assert dq_ < 1e-13 and ddq_ < 1e-11
    third = case["third"]
    assert all(np.count_nonzero(third == k) > B // 6 for k in ((0, 2) if n_points == 1 else (0, 1, 2)))


def test_closed_force_loop_is_well_conditioned_and_presses():
    """tests/contact_loop.py on the CPU (oracle tick + contact_reference), B = 64, 300 periods: every robot touches, the
    controller switches to force control, and a start one ulp away ends within a tenth of the closed-loop bounds the GPU
    test holds the loops to (1e-9, 1e-8): that decides the number of periods there."""
    import contact_loop as cl

    B, periods = 64, 300
    inp = cl.inputs(B)
    a, b = cl.CpuLoop(inp, B), cl.CpuLoop(inp, B)
    qa, va, sa = a.run(inp, periods)
    qb, vb, _ = b.run(inp, periods, q0=np.nextafter(inp["q"], np.inf), switch_at=sa)
    assert sa is not None and 30 < sa < periods - 100 and a.in_contact() == B
    print(f"switch at {sa}; one-ulp start -> |dq| {np.abs(qa - qb).max():.2e} |ddq| {np.abs(va - vb).max():.2e}")
    assert np.abs(qa - qb).max() < 1e-10 and np.abs(va - vb).max() < 1e-9
    fz = -a.rep["wrench_world"][2]
    assert np.all(fz < -1.0)  # pressing on the surface: the sensed normal force on the environment points down
