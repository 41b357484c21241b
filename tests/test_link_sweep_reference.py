"""The yardsticks of tests/test_gpu_link_sweep.py at inner links, without a GPU (cells: tests/link_sweep_cases.py): the payload
oracle against the 40-digit sum over bodies with the body mid-chain, the contact reference's kinematics against the
independent numpy chain at an inner link, the conditioning of every contact cell the GPU tests draw, that the reference's
contact torque outboard of the contact link is exactly zero, and the sensor rows with the sensor task off the contact link.
The bounds are those of tests/test_payload_reference.py and tests/test_contact_reference.py at the last link."""
import numpy as np
import pytest

import contact_cases as cc
import hp_dynamics_fixture as hd
import hp_fixture
import hp_reference as hp
import joint_dynamics_cases as jc
import link_sweep_cases as ls
import oracle_lib as ol
import payload_cases as pc
import sai2_primitives_perso_amd as pkg
import urdf_np
from contact_reference import ContactReference

EPS = hd.EPS
POSES = 8
# "far more than the bound": a payload attached one link off must miss the oracle-vs-40-digit bound by three decades
FAR = 1e3
ORACLE_PAYLOADS = (1, 2, 3, 9)  # the point mass off the axis, every product of inertia, the light body, a drawn one


def _oracle_terms(text, q, dq):
    pm, _ = pkg.model_from_urdf(text, is_file=False)
    o = ol.Oracle(pm, [ol.joint_task("j", robot_dof=int(pm.dof))], q.shape[1])
    o.set_state(q, dq)
    o.enable_gravity_compensation(True)
    o.tick()
    return o.get_model(), o.get_gravity(), o.get_bias(False), o.get_bias(True)


@pytest.mark.parametrize("k", ORACLE_PAYLOADS)
@pytest.mark.parametrize("robot, link", ls.ORACLE_CELLS)
def test_the_oracle_on_the_merged_model_meets_the_40_digit_sum_over_bodies_at_inner_links(robot, link, k):
    """tests/test_payload_reference.py's test of that name with the body on an inner link, its bounds: the bias and gravity
    vectors to C_BIAS eps beta, M to C_BIAS eps max|M|. And the link is visible: the oracle with the same body one link
    further out misses M and the bias vector by more than FAR times those bounds at every pose (g too, except between the
    horizontal slide of sliding_base and the link turning about the vertical behind it: neither placement loads a joint)."""
    text = pc.texts(robot, link=link)[k]
    model = hp.Model(text)
    n = model.dof
    rng = np.random.default_rng(1000 * link + 100 + k)
    if robot == "panda":
        q = np.ascontiguousarray(rng.uniform(-1.2, 1.2, size=(n, POSES)))
        q[3] = -1.5 + 0.5 * q[3]
    else:  # the middle 60 % of every joint range
        mid, half = 0.5 * (model.lower + model.upper), 0.5 * (model.upper - model.lower)
        q = np.ascontiguousarray(mid[:, None] + 0.6 * half[:, None] * rng.uniform(-1, 1, (n, POSES)))
    dq = np.ascontiguousarray(rng.uniform(-1, 1, size=(n, POSES)))
    M, g, b0, bg = _oracle_terms(text, q, dq)
    Mn, gn, _, bgn = _oracle_terms(pc.texts(robot, link=link + 1)[k], q, dq)
    worst = dict(M=0.0, g=0.0, bias=0.0, bias0=0.0)
    apart = dict(M=np.inf, g=np.inf, bias=np.inf)
    for p in range(POSES):
        _, _, Mx, gx = model.dynamics(q[:, p])
        Mx = np.array([[float(Mx[i, j]) for j in range(n)] for i in range(n)])
        bound_M = hd.C_BIAS * EPS * np.abs(Mx).max()
        bx, beta = hp.bias_terms(model, q[:, p], dq[:, p], None)
        bx, beta = np.array([float(x) for x in bx]), float(hp.norm_inf(beta))
        bound_b = hd.C_BIAS * EPS * beta
        b0x, beta0 = hp.bias_terms(model, q[:, p], dq[:, p], False)
        bound_0 = hd.C_BIAS * EPS * max(float(hp.norm_inf(beta0)), 1e-300)
        err = dict(M=np.abs(M[:, p].reshape(n, n) - Mx).max() / bound_M, bias=np.abs(bg[:, p] - bx).max() / bound_b,
                   g=np.abs(g[:, p] - np.array([float(x) for x in gx])).max() / bound_b,
                   bias0=np.abs(b0[:, p] - np.array([float(x) for x in b0x])).max() / bound_0)
        for key, e in err.items():
            worst[key] = max(worst[key], e)
            assert e <= 1.0, (robot, link, k, p, key, e)
        apart["M"] = min(apart["M"], np.abs(M[:, p] - Mn[:, p]).max() / bound_M)
        apart["g"] = min(apart["g"], np.abs(g[:, p] - gn[:, p]).max() / bound_b)
        apart["bias"] = min(apart["bias"], np.abs(bg[:, p] - bgn[:, p]).max() / bound_b)
    print(f"{robot} link {link} payload {k}: oracle vs 40 digits, in units of the bound: " + " ".join(f"{a} {b:.3f}" for a, b in worst.items())
          + "; one link further out, in units of the bound: " + " ".join(f"{a} {b:.2e}" for a, b in apart.items()))
    assert apart["M"] > FAR and apart["bias"] > FAR, apart
    if (robot, link) != ("sliding_base", 0):
        assert apart["g"] > FAR, apart


@pytest.mark.parametrize("robot, link", ls.KINEMATICS_LINKS)
def test_point_kinematics_agree_with_independent_numpy_chain_at_an_inner_link(robot, link):
    """tests/test_contact_reference.py's test of that name at one inner link per robot (rprp_4: link 2, a slide inboard and
    one outboard of it): x_k, J_k and v_k to 1e-12, and the columns of J_k outboard of the link are exactly zero"""
    B = 12
    case = cc.draw(robot, B, 4, 1, link=link)
    assert case["link"] == link < int(case["model"].dof) - 1
    ref = ContactReference(case["model"], B, link, case["points"], case["rows"], cc.V_EPS)
    chain = urdf_np.Chain(hp_fixture.urdf_text(robot), is_file=False)
    if robot == "rprp_4":
        types = [j["type"] for j in hp.Model(hp_fixture.urdf_text(robot)).moving]
        assert "prismatic" in types[: link + 1] and "prismatic" in types[link + 1:]
    name = chain.moving[link]["child"]
    _, links = pkg.model_from_urdf(hp_fixture.urdf_text(robot), is_file=False)
    idx, pos, R = pkg.resolve_link_frame(links, name)
    assert idx == link
    in_urdf_link = [R.T @ (c - pos) for c in case["points"]]
    x, J, v = ref.point_kinematics(case["q"], case["dq"])
    assert np.all(J[:, :, link + 1:] == 0) and np.abs(J[:, :, link]).max() > 0
    for b in range(B):
        for k, c in enumerate(in_urdf_link):
            Jn, xn, _ = chain.jacobian(case["q"][:, b], name, c)
            assert np.abs(xn - x[k, :, b]).max() < 1e-12
            assert np.abs(Jn[:3] - J[k, :, :, b]).max() < 1e-12
            assert np.abs(Jn[:3] @ case["dq"][:, b] - v[k, :, b]).max() < 1e-12


def test_the_link_keyword_leaves_the_default_draw_as_it_was():
    """draw without a link is draw at the last link, and the link is not part of the seed: states, torques, normals and
    gains of every link of a robot are the same numbers"""
    a, b, c = cc.draw("six_r", 50, 4), cc.draw("six_r", 50, 4, link=5), cc.draw("six_r", 50, 4, link=2)
    assert a["link"] == b["link"] == 5 and c["link"] == 2
    for key in ("q", "dq", "tau", "rows", "third", "points"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("q", "dq", "tau", "third", "points"):
        assert np.array_equal(a[key], c[key]), key
    assert np.array_equal(a["rows"][3:], c["rows"][3:]) and not np.array_equal(a["rows"][:3], c["rows"][:3])


@pytest.mark.parametrize("robot, link, n_points, B", ls.DRAWN_CELLS)
def test_inputs_of_the_gpu_link_sweep_are_well_conditioned(robot, link, n_points, B):
    """tests/test_contact_reference.py::test_inputs_of_the_gpu_tests_are_well_conditioned on every cell the GPU sweep draws,
    its bounds: a start one ulp away ends within |dq| 1e-13 and |ddq| 1e-11, each third of the robots is there. And the mask
    the kernel must reproduce: the reference's contact torque on every joint outboard of the link is exactly zero, while at
    least B // 4 robots load the link's own joint."""
    case = cc.draw(robot, B, n_points, link=link)
    for grav in (False, True):
        a = cc.reference_run(case, grav).get_state()
        b = cc.reference_run(case, grav, q=np.nextafter(case["q"], np.inf), dq=np.nextafter(case["dq"], np.inf)).get_state()
        dq_, ddq_ = np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()
        print(f"{robot} link {link} points={n_points} B={B} gravity={grav}: one-ulp start -> |dq| {dq_:.2e} |ddq| {ddq_:.2e}")
        assert dq_ < 1e-13 and ddq_ < 1e-11
    third = case["third"]
    counts = [int(np.count_nonzero(third == k)) for k in range(3)]
    print(f"{robot} link {link} points={n_points} B={B}: thirds {counts}")
    assert all(counts[k] > B // 6 for k in ((0, 2) if n_points == 1 else (0, 1, 2)))
    tau = ContactReference(case["model"], B, link, case["points"], case["rows"], cc.V_EPS).forces(case["q"], case["dq"])["tau"]
    loaded = int(np.count_nonzero(tau[link]))
    print(f"{robot} link {link} points={n_points} B={B}: robots with a torque on joint {link}: {loaded}")
    assert np.all(tau[link + 1:] == 0) and loaded >= B // 4


@pytest.mark.parametrize("payload_link, contact_link", ls.MIXED_CELLS)
def test_mixed_link_cells_are_well_conditioned(payload_link, contact_link):
    """payload on one link, contact on another, every joint effect on (the cell of test_gpu_link_sweep's mixed test): the
    reference of tests/joint_dynamics_reference.py over the payload oracles and the contact reference, started one ulp away,
    ends within a tenth of the bounds that test holds (1e-12, 1e-10)"""
    B = ls.MIXED_B
    con, case, rows, k = ls.mixed_case(contact_link)
    cfgs = [ol.joint_task("j", robot_dof=7)]
    ends = []
    for ulp in (False, True):
        plant = pc.PayloadOracles(pc.texts("panda", payload_link), cfgs, B)
        cref = ContactReference(case["model"], B, contact_link, con["points"], con["rows"], cc.V_EPS)
        q, dq = (np.nextafter(case["q"], np.inf), np.nextafter(case["dq"], np.inf)) if ulp else (case["q"], case["dq"])
        ends.append(jc.reference_run(case, rows, k, True, plant=plant, contact=cref, q=q, dq=dq).get_state())
    dq_, ddq_ = np.abs(ends[0][0] - ends[1][0]).max(), np.abs(ends[0][1] - ends[1][1]).max()
    print(f"payload link {payload_link} contact link {contact_link}: one-ulp start -> |dq| {dq_:.2e} |ddq| {ddq_:.2e}")
    assert dq_ < 1e-13 and ddq_ < 1e-11


@pytest.mark.parametrize("contact_link, sensor_link", [c for c in ls.SENSOR_CELLS if c[1] is not None])
def test_sensor_rows_invert_the_tasks_own_transform_off_the_contact_link(contact_link, sensor_link):
    """tests/test_contact_reference.py::test_sensor_rows_invert_the_tasks_own_transform with the sensor task's control frame on
    another link than the contact: the sensed rows, pushed through the oracle's get_mft_status, give back -sum F_k and the
    moment about the task's control point (which is not on the contact link): 1e-12 scaled as there"""
    B = 60
    case = cc.draw("panda", B, 4, 3, link=contact_link)
    ref = ContactReference(case["model"], B, contact_link, case["points"], case["rows"], cc.V_EPS)
    ref.set_state(case["q"], case["dq"])
    o = ol.Oracle(cc.model("panda"), ls.sensor_tasks(ol.motion_force_task, ol.joint_task, sensor_link), B)
    rep = ref.report(sensor=(o, 0))
    assert rep["robots_in_contact"] > B // 3
    o.set_mft_sensed_wrench(0, rep["sensed"][:3], rep["sensed"][3:])
    st = o.get_mft_status(0)
    scale = max(1.0, np.abs(rep["wrench_world"]).max())
    assert np.abs(st["sensed_force"] + rep["wrench_world"][:3]).max() < 1e-12 * scale
    assert np.abs(st["sensed_moment"] + rep["wrench_world"][3:]).max() < 1e-12 * scale
    f = ref.forces(*ref.get_state())
    _, _, xc, _ = o.get_model(0)
    M = sum(np.cross(f["x"][k] - xc, f["F"][k], axis=0) for k in range(4))
    assert np.abs(M - rep["wrench_world"][3:]).max() < 1e-12
    # and the link of the control frame matters: the moment about the contact link's origin is another one
    assert np.abs(ref.report()["wrench_world"][3:] - rep["wrench_world"][3:]).max() > 1e-3


@pytest.mark.parametrize("config", (2, 3, 4))
def test_the_payloads_link_is_visible_in_the_torques(config):
    """the workloads of the GPU sweep at its batch: between the oracles with the payload on link L and on link L + 1, every
    robot that carries a payload moves by more than 1e-5 of max|tau|, for every L in 0..5: the GPU torques, within 1e-10 of the
    oracles of link L, are then more than the 1e-6 the GPU test asks for away from those of link L + 1"""
    B = ls.PAYLOAD_B
    inp = pkg.workloads.make_inputs(config, B=B, seed=5)
    taus = []
    for link in range(7):
        o = pc.PayloadOracles(pc.texts("panda", link=link), ol.task_configs(inp["tasks"]), B)
        o.load_inputs(inp)
        o.enable_gravity_compensation(True)
        taus.append(o.tick())
    carries = np.arange(B) % pc.P != 0
    assert carries.sum() >= 120
    for link in ls.PANDA_PAYLOAD_LINKS:
        d = np.abs(taus[link] - taus[link + 1]).max(axis=0) / np.abs(taus[link]).max()
        print(f"C{config} payload on link {link} against link {link + 1}: least move of a loaded robot {d[carries].min():.2e} of max|tau|")
        assert d[carries].min() > 1e-5
        assert np.array_equal(taus[link][:, ~carries], taus[link + 1][:, ~carries])
