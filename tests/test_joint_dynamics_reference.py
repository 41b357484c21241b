"""CPU-only: pins tests/joint_dynamics_reference.py (the reference the GPU tests of the plant's joint dynamics compare with)
and the host-only entry points sai2b_default_joint_dynamics / sai2b_validate_joint_dynamics of the built library.

The host-ARRAY checks of sai2b_set_joint_dynamics need a context, and a context needs a device: they are exercised in
tests/test_gpu_joint_dynamics.py (test_host_array_validation)."""
import ctypes as C

import numpy as np
import pytest

import joint_dynamics_cases as jc
import joint_dynamics_reference as jr
import oracle_lib as ol
from sai2_primitives_perso_amd import _abi


def _oracle(case, B):
    return ol.Oracle(case["model"], [ol.joint_task("j", robot_dof=case["n"])], B, threads=8)


@pytest.mark.parametrize("robot", ["panda", "planar_4r", "sliding_base"])
def test_neutral_rows_are_the_plain_step(robot):
    """a = d = f = 0, t = +inf, lo / hi = -/+inf: five periods of three substeps equal Oracle.sim_step within 1e-13.
    The law solves for the new velocity itself, M dq+ = M dq + h (tau - b), where the oracle adds h M^-1 (tau - b) to dq: the
    two differ by cond(M) eps |dq| per substep, and cond(M) reaches 4e3 on the planar 4R. The bound is absolute, so the
    states are gentle ones (speeds of N(0, 0.04^2), torques of N(0, 0.2^2): |dq| stays below 1 rad/s)."""
    B = 64
    case = jc.draw(robot, B)
    n = case["n"]
    rows = jr.rows_array(n, B)
    tau = 0.01 * case["tau"]
    case["dq"] = 0.05 * case["dq"]
    for grav in (False, True):
        o = _oracle(case, B)
        o.set_state(case["q"], case["dq"])
        ref = jr.JointDynamicsReference(case["model"], B, rows)
        ref.set_state(case["q"], case["dq"])
        for _ in range(jc.PERIODS):
            o.sim_step(tau, jc.DT, jc.SUBSTEPS, grav)
            ref.step(tau, jc.DT, jc.SUBSTEPS, grav)
        (qo, vo), (qr, vr) = o.get_state(), ref.get_state()
        eq, ev = np.abs(qo - qr).max(), np.abs(vo - vr).max()
        print(f"{robot} gravity={grav}: |dq| {eq:.2e} |ddq| {ev:.2e}")
        assert eq < 1e-13 and ev < 1e-13
        rep = ref.report()
        assert rep["robots_saturated"] == 0 and rep["robots_at_stop"] == 0 and not rep["stop_torque"].any()
        assert not rep["dissipative_torque"].any() and np.array_equal(rep["applied_torque"], tau)


def test_step_identity_on_random_states():
    """(M + diag(a)) (dq+ - dq) / h = ts + sl - su - g o dq+ - b on 10 000 random states: "implicit" pinned with a formula the
    solver does not use. Relative residual: the largest |lhs - rhs| of a robot over the sum of the magnitudes of the terms
    that enter it, (|M + diag(a)| (|dq+| + |dq|)) / h + |ts| + |sl| + |su| + |g dq+| + |b| (a backward-error measure: what one
    rounding of each term is worth), below 1e-12."""
    B = 10000
    case = jc.draw("panda", B, seed=3)
    n = case["n"]
    rows, k = jc.select(case, "all")
    ref = jc.reference(case, rows, k)
    h = jc.DT / jc.SUBSTEPS
    q, dq = case["q"], case["dq"]
    q1, dq1 = ref.substep(q, dq, case["tau"], h, True)
    T = ref.terms(q, dq, case["tau"], True)
    Ma = T["M"] + np.eye(n)[:, :, None] * rows[0][None]
    lhs = np.einsum("ijb,jb->ib", Ma, dq1 - dq) / h
    rhs = T["ts"] + T["sl"] - T["su"] - T["g"] * dq1 - T["b"]
    scale = (np.einsum("ijb,jb->ib", np.abs(Ma), np.abs(dq1) + np.abs(dq)) / h + np.abs(T["ts"]) + T["sl"] + T["su"] + np.abs(T["g"] * dq1)
             + np.abs(T["b"]))
    res = (np.abs(lhs - rhs) / scale).max()
    print(f"relative residual {res:.2e}; at a stop {np.count_nonzero((T['sl'] - T['su']).any(axis=0))}, "
          f"saturated {np.count_nonzero((T['ts'] != case['tau']).any(axis=0))}")
    assert res < 1e-12
    assert np.array_equal(q1, q + h * dq1)
    assert np.count_nonzero((T["sl"] - T["su"]).any(axis=0)) > B // 5 and np.count_nonzero((T["ts"] != case["tau"]).any(axis=0)) > B // 2


def test_signs_and_seams():
    rng = np.random.default_rng(5)
    # friction: |torque| <= f, tending to f for |dq| >> e, opposing the motion
    f, e = rng.uniform(0.1, 2, 1000), 1e-3
    dq = rng.normal(0, 1, 1000) * 10.0 ** rng.uniform(-6, 1, 1000)
    tf = -jr.dissipation(dq, 0.0, f, e) * dq
    assert np.all(np.abs(tf) <= f) and np.all(tf * dq <= 0)
    fast = np.abs(dq) > 1e3 * e
    assert fast.sum() > 100 and np.all(np.abs(tf[fast]) > f[fast] * (1 - 1e-6))
    assert np.all(np.abs(-jr.dissipation(1e-9, 0.0, f, e) * 1e-9) < 1e-5 * f)  # it fades to zero at rest
    # stops: zero strictly inside, never pull into a stop, continuous at q = lo, q = hi and where the Hunt-Crossley factor crosses zero
    lo, hi, k, c = -1.0, 2.0, 1e4, 0.5
    q = rng.uniform(lo, hi, 1000)
    sl, su = jr.stop_torques(q, rng.normal(0, 3, 1000), lo, hi, k, c)
    assert not sl.any() and not su.any()
    q, dq = rng.uniform(lo - 0.1, hi + 0.1, 4000), rng.normal(0, 3, 4000)
    sl, su = jr.stop_torques(q, dq, lo, hi, k, c)
    assert np.all(sl >= 0) and np.all(su >= 0) and not (sl[q >= lo].any() or su[q <= hi].any())
    assert (sl > 0).sum() > 50 and (su > 0).sum() > 50 and ((q < lo) & (sl == 0)).sum() > 5  # leaving fast: no pull back in
    for eps in (1e-9, 1e-12):
        for v in (-1.0, 0.0, 1.0):
            a, b = jr.stop_torques(np.array([lo - eps, hi + eps]), v, lo, hi, k, c)
            assert a[0] <= k * eps * (1 + c) * 1.001 and b[1] <= k * eps * (1 + c) * 1.001 and a[1] == 0 and b[0] == 0  # (1.001: q itself is rounded)
        # 1 - c dq = 0 at dq = 1 / c (lower stop, leaving), 1 + c dq = 0 at dq = -1 / c (upper stop, leaving)
        a, _ = jr.stop_torques(lo - 0.01, np.array([1 / c - eps, 1 / c + eps]), lo, hi, k, c)
        _, b = jr.stop_torques(hi + 0.01, np.array([-1 / c + eps, -1 / c - eps]), lo, hi, k, c)
        assert 0 <= a[0] <= k * 0.01 * c * eps * 1.01 and a[1] == 0 and 0 <= b[0] <= k * 0.01 * c * eps * 1.01 and b[1] == 0
    # saturation: tau inside the limit, -t / +t outside
    t = rng.uniform(5, 30, 1000)
    tau = rng.normal(0, 20, 1000)
    ts = jr.saturate(tau, t)
    inside = np.abs(tau) <= t
    assert np.array_equal(ts[inside], tau[inside]) and np.array_equal(ts[~inside], np.sign(tau[~inside]) * t[~inside])
    assert inside.sum() > 100 and (~inside).sum() > 100


def test_infinite_limits_give_no_nan():
    B = 32
    case = jc.draw("panda", B)
    rows, k = jc.select(case, "all")
    rows[3, :, ::2] = np.inf
    rows[4, :, ::3] = -np.inf
    rows[5, :, 1::3] = np.inf
    ref = jc.reference_run(case, rows, k, True)
    q, dq = ref.get_state()
    rep = ref.report()
    assert np.isfinite(q).all() and np.isfinite(dq).all()
    assert all(np.isfinite(rep[key]).all() for key in ("applied_torque", "stop_torque", "dissipative_torque"))
    assert np.array_equal(rep["applied_torque"][:, ::2], case["tau"][:, ::2])


@pytest.mark.parametrize("robot", jc.ROBOTS)
def test_one_ulp_sensitivity(robot):
    """The bounds the GPU tests hold the state to (1e-12 rad, 1e-10 rad/s) must stand well above what the reference itself
    makes of a one-ulp change of the start state: below a tenth of each bound, for every robot and with every effect on."""
    B = 130
    case = jc.draw(robot, B)
    rows, k = jc.select(case, "all")
    for grav in (False, True):
        a = jc.reference_run(case, rows, k, grav)
        b = jc.reference_run(case, rows, k, grav, q=np.nextafter(case["q"], np.inf), dq=np.nextafter(case["dq"], np.inf))
        (qa, va), (qb, vb) = a.get_state(), b.get_state()
        eq, ev = np.abs(qa - qb).max(), np.abs(va - vb).max()
        print(f"{robot} gravity={grav}: one ulp -> |dq| {eq:.2e} |ddq| {ev:.2e}")
        assert eq < 1e-13 and ev < 1e-11


# ---- the host-only entry points of the library
def _lib():
    return _abi.load_library()


def _validate(cfg, dof=7):
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_joint_dynamics(C.byref(cfg), dof, msg, 256)
    return rc, msg.value.decode()


def test_defaults_and_layout():
    assert _lib().sai2b_sizeof_joint_dynamics_config() == C.sizeof(_abi.JointDynamicsConfig) == 3 * 8 * _abi.MAX_DOF
    assert (_abi.BUF_JOINT_DYNAMICS, _abi.BUF_JOINT_DYNAMICS_STATE) == (11, 12)
    for dof in (4, 6, 7, 8):
        cfg = _abi.JointDynamicsConfig()
        assert _lib().sai2b_default_joint_dynamics(C.byref(cfg), dof) == _abi.OK
        assert not any(cfg.stop_stiffness) and not any(cfg.stop_damping) and all(e == 1e-2 for e in cfg.friction_velocity_eps)
        assert _validate(cfg, dof) == (_abi.OK, "")
    assert _lib().sai2b_default_joint_dynamics(C.byref(cfg), 5) == _abi.UNSUPPORTED and _validate(cfg, 5)[0] == _abi.UNSUPPORTED


@pytest.mark.parametrize("field, value, message", [
    ("stop_stiffness", -1.0, "joint dynamics: stop_stiffness must be finite and >= 0"),
    ("stop_stiffness", float("inf"), "joint dynamics: stop_stiffness must be finite and >= 0"),
    ("stop_stiffness", float("nan"), "joint dynamics: stop_stiffness must be finite and >= 0"),
    ("stop_damping", -0.5, "joint dynamics: stop_damping must be finite and >= 0"),
    ("stop_damping", float("nan"), "joint dynamics: stop_damping must be finite and >= 0"),
    ("friction_velocity_eps", 0.0, "joint dynamics: friction_velocity_eps must be finite and > 0"),
    ("friction_velocity_eps", -1e-3, "joint dynamics: friction_velocity_eps must be finite and > 0"),
    ("friction_velocity_eps", float("inf"), "joint dynamics: friction_velocity_eps must be finite and > 0"),
    ("friction_velocity_eps", float("nan"), "joint dynamics: friction_velocity_eps must be finite and > 0"),
])
def test_rejections(field, value, message):
    cfg = _abi.JointDynamicsConfig()
    assert _lib().sai2b_default_joint_dynamics(C.byref(cfg), 7) == _abi.OK
    getattr(cfg, field)[7] = value  # an entry >= dof is ignored
    assert _validate(cfg) == (_abi.OK, "")
    getattr(cfg, field)[3] = value
    assert _validate(cfg) == (_abi.INVALID_ARGUMENT, message)
    assert _lib().sai2b_last_error(None).decode() == message
