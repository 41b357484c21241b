"""CPU-only: pins tests/external_wrench_reference.py (the reference the GPU tests of the plant's external wrench compare
with) and the host-only entry points sai2b_default_external_wrench / sai2b_validate_external_wrench of the built library.

The host-ARRAY checks of sai2b_set_external_wrench need a context, and a context needs a device: they are exercised in
tests/test_gpu_external_wrench.py (test_argument_checks).

What of this file fails without the feature: the tests of the library's entry points and of the sharding helper
(test_defaults_and_layout, test_rejections, test_sharding_slices_the_rows). The tests that pin the numpy reference (power
identity, frames, known answer, countdown, sensor rows, one-ulp condition) run on the oracle alone and pass with or
without it: they are there so that the GPU tests, which all need the feature, compare with something that is held itself."""
import ctypes as C

import numpy as np
import pytest

import external_wrench_cases as wc
import external_wrench_reference as wr
import hp_fixture
import oracle_lib as ol
import payload_cases as pc
import sai2_primitives_perso_amd as pkg
import urdf_np
from sai2_primitives_perso_amd import _abi


def _urdf_point(robot, link, point):
    """(URDF link name, the point of the model's link frame in the URDF link's frame)"""
    text = hp_fixture.urdf_text(robot)
    _, links = pkg.model_from_urdf(text, is_file=False)
    name = pc.link_name(text, link)
    idx, pos, R = pkg.resolve_link_frame(links, name)
    assert idx == link
    return text, name, R.T @ (np.asarray(point) - pos)  # model = pos + R urdf


@pytest.mark.parametrize("robot, link, frame", wc.cells())
def test_power_identity(robot, link, frame):
    """tx . dq = F_w . v_x + M_w . omega with v_x, omega of the application point from tests/urdf_np.py (its own forward
    kinematics and Jacobian from the URDF text, independent of the oracle), 1e-12 relative to the sum of the magnitudes of
    the terms; rows of joints outboard of the link are exactly zero"""
    B = 16
    case = wc.draw(robot, B, link, frame)
    ref = wc.reference(case)
    w = ref.wrench(case["q"], case["dq"])
    text, name, c = _urdf_point(robot, link, case["point"])
    chain = urdf_np.Chain(text, is_file=False)
    assert np.all(w["tau"][link + 1:] == 0) and np.all(w["tau"][: link + 1] != 0)
    for b in range(B):
        J, x, _ = chain.jacobian(case["q"][:, b], name, c)
        v = J @ case["dq"][:, b]
        assert np.abs(x - w["x"][:, b]).max() < 1e-14
        lhs = w["tau"][:, b] @ case["dq"][:, b]
        rhs = w["Fw"][:, b] @ v[:3] + w["Mw"][:, b] @ v[3:]
        scale = np.abs(w["tau"][:, b] * case["dq"][:, b]).sum() + np.abs(w["Fw"][:, b] * v[:3]).sum() + np.abs(w["Mw"][:, b] * v[3:]).sum()
        assert abs(lhs - rhs) < 1e-12 * scale, (b, lhs, rhs)


@pytest.mark.parametrize("robot", wc.ROBOTS)
def test_link_frame_rows_are_world_rows_of_the_turned_wrench(robot):
    B = 32
    for link in wc.links(robot):
        in_link = wc.draw(robot, B, link, "link")
        a = wc.reference(in_link).wrench(in_link["q"], in_link["dq"])
        turned = in_link["rows"].copy()
        turned[0:3] = np.einsum("ijb,jb->ib", a["R"], in_link["rows"][0:3])
        turned[3:6] = np.einsum("ijb,jb->ib", a["R"], in_link["rows"][3:6])
        in_world = wc.draw(robot, B, link, "world")
        b = wc.reference(in_world, rows=turned).wrench(in_world["q"], in_world["dq"])
        assert np.array_equal(a["tau"], b["tau"]) and np.array_equal(a["Fw"], b["Fw"]) and np.array_equal(a["Mw"], b["Mw"])
        assert np.abs(a["Fw"] - in_link["rows"][0:3]).max() > 1.0  # the frames do differ


def test_planar_4r_known_answer():
    """planar 4R (all axes z, links of 0.5 m along x) at q = (pi/2, -pi/2, pi/2, 0): joint origins (0, 0), (0, 0.5), (0.5, 0.5),
    (0.5, 1), last link turned by pi/2. c = (0.2, 0.1, 0.07), F = (3, -4, 7), M = (0.5, -0.25, 2):
      last link, world: x = (0.4, 1.2, 0.07), tx_i = r_x F_y - r_y F_x + M_z with r = x - p_i: -3.2, -1.7, 0.3, 1.8
      last link, link frame: F_w = (4, 3, 7): 1.2 - 4.8 + 2 = -1.6, 1.2 - 2.8 + 2 = 0.4, -0.3 - 2.8 + 2 = -1.1, -0.3 - 0.8 + 2 = 0.9
      link 1 (turned by 0), world: x = (0.2, 0.6, 0.07): -0.8 - 1.8 + 2 = -0.6, -0.8 - 0.3 + 2 = 0.9, 0, 0"""
    m = wc.model("planar_4r")
    q = np.array([[np.pi / 2], [-np.pi / 2], [np.pi / 2], [0.0]])
    rows = np.array([[3.0], [-4.0], [7.0], [0.5], [-0.25], [2.0], [-1.0]])
    for link, frame, want in ((3, wr.WORLD, (-3.2, -1.7, 0.3, 1.8)), (3, wr.LINK, (-1.6, 0.4, -1.1, 0.9)), (1, wr.WORLD, (-0.6, 0.9, 0.0, 0.0))):
        ref = wr.ExternalWrenchReference(m, 1, link, rows, (0.2, 0.1, 0.07), frame)
        w = ref.wrench(q, np.zeros((4, 1)))
        assert np.abs(w["tau"][:, 0] - want).max() < 1e-14, (link, frame, w["tau"][:, 0])
        if link == 1:
            assert np.all(w["tau"][2:] == 0)
            assert np.abs(w["x"][:, 0] - (0.2, 0.6, 0.07)).max() < 1e-15


def test_countdown_and_activity():
    steps = np.array([0.0, 1.0, 3.0, -1.0, np.nan, 0.5, -0.0, np.inf])
    assert list(wr.active(steps)) == [False, True, True, True, False, True, False, True]
    after = wr.countdown(steps)
    assert np.array_equal(after[[0, 1, 2, 3, 5, 7]], [0.0, 0.0, 2.0, -1.0, 0.0, np.inf]) and np.isnan(after[4]) and after[6] == 0
    # a reference over five periods: robots pushed for exactly 0, 1, 3, 5, 0 periods; an inactive robot's rows are exact zeros
    B = 5
    case = wc.draw("panda", B)
    case["rows"][6] = [0.0, 1.0, 3.0, -1.0, np.nan]
    ref = wc.reference(case)
    ref.set_state(case["q"], case["dq"])
    pushed = np.zeros(B, dtype=int)
    for _ in range(wc.PERIODS):
        ref.step(case["tau"], wc.DT, wc.SUBSTEPS, True)
        rep = ref.report()
        pushed += ref.active
        assert rep["robots_pushed"] == np.count_nonzero(ref.active)
        assert not rep["wrench_world"][:, ~ref.active].any() and not rep["torque"][:, ~ref.active].any()
    assert list(pushed) == [0, 1, 3, 5, 0]
    assert np.array_equal(ref.rows[6][:4], [0.0, 0.0, 0.0, -1.0]) and np.isnan(ref.rows[6][4])


@pytest.mark.parametrize("same_link", [True, False])
def test_sensor_rows_through_the_oracles_transform(same_link):
    """the sensed rows, given to the oracle as its sensor reading, come back from its own sensor-to-control-point transform
    (get_mft_status) as -F_w and -(M_w + (x - x_c) x F_w): sensor task on the wrench link and on another link"""
    B = 24
    case = wc.draw("panda", B, 6, "link")
    mft = ol.motion_force_task("m", link=6 if same_link else 4, frame_pos=(0.01, 0.02, 0.06))
    mft.sensor_rot[:] = [np.cos(0.4), -np.sin(0.4), 0, np.sin(0.4), np.cos(0.4), 0, 0, 0, 1]
    mft.sensor_pos[:] = (0.0, 0.01, -0.03)
    o = ol.Oracle(case["model"], [mft, ol.joint_task("j")], B, threads=8)
    ref = wc.reference(case)
    ref.set_state(case["q"], case["dq"])
    rep = ref.report(sensor=(o, 0))
    o.set_mft_sensed_wrench(0, np.ascontiguousarray(rep["sensed"][:3]), np.ascontiguousarray(rep["sensed"][3:]))
    o.update_task_models()
    st = o.get_mft_status(0)
    Fw, Mw = rep["wrench_world"][:3], rep["wrench_world"][3:]
    want_m = -(Mw + np.cross(rep["x"] - st["pos"], Fw, axis=0))
    assert np.abs(st["sensed_force"] + Fw).max() < 1e-12 * wc.F_MAX
    assert np.abs(st["sensed_moment"] - want_m).max() < 1e-12 * wc.F_MAX


@pytest.mark.parametrize("robot, link, frame", wc.cells())
def test_one_ulp_sensitivity(robot, link, frame):
    """The bounds the GPU tests hold the state to (1e-12 rad, 1e-10 rad/s) must stand well above what the reference itself
    makes of a one-ulp change of the start state: below a tenth of each bound on every drawn cell, 257 robots per cell."""
    B = 257
    case = wc.draw(robot, B, link, frame)
    for grav in (False, True):
        a = wc.reference_run(case, grav)
        b = wc.reference_run(case, grav, q=np.nextafter(case["q"], np.inf), dq=np.nextafter(case["dq"], np.inf))
        (qa, va), (qb, vb) = a.get_state(), b.get_state()
        eq, ev = np.abs(qa - qb).max(), np.abs(va - vb).max()
        print(f"{robot} link={link} frame={frame} gravity={grav}: one ulp -> |dq| {eq:.2e} |ddq| {ev:.2e}")
        assert eq < 1e-13 and ev < 1e-11


# ---- the host-only entry points of the library
def _lib():
    return _abi.load_library()


def _validate(cfg, tasks, dof=7):
    msg = C.create_string_buffer(256)
    arr = (_abi.TaskConfig * len(tasks))(*tasks) if tasks else None
    rc = _lib().sai2b_validate_external_wrench(C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def test_defaults_and_layout():
    assert _lib().sai2b_sizeof_external_wrench_config() == C.sizeof(_abi.ExternalWrenchConfig) == 40
    assert (_abi.BUF_EXTERNAL_WRENCH, _abi.BUF_EXTERNAL_WRENCH_STATE) == (13, 14) and (_abi.WRENCH_WORLD, _abi.WRENCH_LINK) == (0, 1)
    cfg = _abi.ExternalWrenchConfig()
    assert _lib().sai2b_default_external_wrench(C.byref(cfg), 5) == _abi.OK
    assert (cfg.link, cfg.frame, cfg.sensor_task, list(cfg.point)) == (5, _abi.WRENCH_WORLD, -1, [0.0, 0.0, 0.0])
    for dof in (4, 6, 7, 8):
        _lib().sai2b_default_external_wrench(C.byref(cfg), dof - 1)
        assert _validate(cfg, [], dof) == (_abi.OK, "")
    assert _validate(cfg, [], 5)[0] == _abi.UNSUPPORTED


def test_rejections():
    tasks = [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")]

    def cfg(**kw):
        c = _abi.ExternalWrenchConfig()
        _lib().sai2b_default_external_wrench(C.byref(c), 6)
        for k, v in kw.items():
            if k == "point":
                c.point[:] = v
            else:
                setattr(c, k, v)
        return c

    assert _validate(cfg(sensor_task=0, frame=_abi.WRENCH_LINK, point=(0.1, 0.2, 0.3)), tasks) == (_abi.OK, "")
    for bad, message in ((dict(link=-1), "external wrench: link must be in [0, dof)"), (dict(link=7), "external wrench: link must be in [0, dof)"),
                         (dict(frame=2), "external wrench: frame must be SAI2B_WRENCH_WORLD or SAI2B_WRENCH_LINK"),
                         (dict(frame=-1), "external wrench: frame must be SAI2B_WRENCH_WORLD or SAI2B_WRENCH_LINK"),
                         (dict(point=(0.0, float("nan"), 0.0)), "external wrench: point must be finite"),
                         (dict(point=(float("inf"), 0.0, 0.0)), "external wrench: point must be finite"),
                         (dict(sensor_task=1), "external wrench: sensor_task must be -1 or the index of a MotionForceTask"),
                         (dict(sensor_task=2), "external wrench: sensor_task must be -1 or the index of a MotionForceTask"),
                         (dict(sensor_task=-2), "external wrench: sensor_task must be -1 or the index of a MotionForceTask")):
        assert _validate(cfg(**bad), tasks) == (_abi.INVALID_ARGUMENT, message), bad
        assert _lib().sai2b_last_error(None).decode() == message
    assert _validate(cfg(sensor_task=0), [])[0] == _abi.INVALID_ARGUMENT  # no tasks given: no sensor task to name


def test_sharding_slices_the_rows():
    """sharding.set_external_wrench gives every rank its columns of rows given for the whole batch, as set_link_payload does;
    a [3] force and a scalar steps are batch-uniform and pass as they are"""
    from sai2_primitives_perso_amd import sharding

    class Recorder:
        def set_external_wrench(self, link, force, moment=None, steps=None, **kw):
            self.got = (link, force, moment, steps, kw)

    B, world = 10, 3
    rng = np.random.default_rng(0)
    F, M, S = rng.normal(size=(3, B)), rng.normal(size=(3, B)), np.arange(B, dtype=np.float64)
    seen = []
    for rank in range(world):
        lo, hi = sharding.shard_bounds(B, world, rank)
        c = Recorder()
        sharding.set_external_wrench(c, world, rank, 5, F, M, S, point=(0.0, 0.0, 0.1), frame="link", sensor_task=0)
        link, f, m, s, kw = c.got
        assert link == 5 and kw == dict(point=(0.0, 0.0, 0.1), frame="link", sensor_task=0)
        assert np.array_equal(f, F[:, lo:hi]) and np.array_equal(m, M[:, lo:hi]) and np.array_equal(s, S[lo:hi])
        assert f.flags.c_contiguous and m.flags.c_contiguous
        seen.append(hi - lo)
        sharding.set_external_wrench(c, world, rank, 5, np.array([1.0, 2.0, 3.0]), None, 4.0)
        assert np.array_equal(c.got[1], [1.0, 2.0, 3.0]) and c.got[2] is None and c.got[3] == 4.0
    assert sum(seen) == B
