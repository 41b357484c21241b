"""CPU-only: tests/reward_reference.py (the numpy restatement the GPU tests compare with) against hand-computed answers."""
import types

import numpy as np

import reward_reference as rr


def _cfg(dim, axis, in_frame, P=None):
    P6 = np.eye(6)
    if P is not None:
        P6[:3, :3] = P
    return types.SimpleNamespace(force_space_dimension=dim, force_axis=axis, parametrization_in_compliant_frame=in_frame,
                                 partial_projection=list(P6.reshape(-1)))


def _rot_z90(B=1):
    """the compliant frame turned by +90 degrees about the world z: its x axis is the world's y"""
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return np.repeat(R.reshape(9, 1), B, axis=1)


def test_hinges_exactly_at_their_knee():
    dq, tau = np.zeros((2, 3)), np.zeros((2, 3))
    margin = np.array([0.25, 0.1, 0.4])
    g = rr.global_terms(dq, tau, tau, np.ones(3, bool), margin, 0.25, np.zeros(3, np.uint8), np.zeros(6))
    assert np.array_equal(g["limit"], [0.0, 0.15, 0.0]) and g["limit"][0] == 0.0  # at the knee: exactly 0, not negative
    f = np.array([[3.0, 3.0, 0.0], [4.0, 0.0, 0.0], [0.0, 0.0, 0.0]])  # |f| = 5, 3, 0
    t = rr.task_terms(_cfg(0, (0, 0, 1), False), _rot_z90(3), np.zeros((6, 3)), np.zeros(3), np.zeros(3), f, np.zeros((3, 3)), 1.0, 1.0, 5.0)
    assert np.array_equal(t["force_excess"], [0.0, 0.0, 0.0])
    t = rr.task_terms(_cfg(0, (0, 0, 1), False), _rot_z90(3), np.zeros((6, 3)), np.zeros(3), np.zeros(3), f, np.zeros((3, 3)), 1.0, 1.0, 3.0)
    assert np.array_equal(t["force_excess"], [2.0, 0.0, 0.0])


def test_tanh_at_zero_and_far_out():
    d = np.array([0.0, 1e3, 0.5])
    t = rr.task_terms(_cfg(0, (0, 0, 1), False), _rot_z90(3), np.zeros((6, 3)), d, d, np.zeros((3, 3)), np.zeros((3, 3)), 0.5, 2.0, 0.0)
    assert t["pos_tanh"][0] == 1.0 and t["pos_tanh"][1] == 0.0 and t["ori_tanh"][0] == 1.0 and t["ori_tanh"][1] == 0.0
    assert abs(t["pos_tanh"][2] - (1 - np.tanh(1.0))) < 1e-16 and abs(t["ori_tanh"][2] - (1 - np.tanh(0.25))) < 1e-16
    assert np.array_equal(t["pos"], d) and np.array_equal(t["pos_sq"], d * d) and np.array_equal(t["ori_sq"], d * d)


def test_a_force_axis_in_the_control_frame():
    # one force direction along the control frame's x, which is the world's y: only the y difference counts
    fs, fg = np.array([[1.0], [5.0], [7.0]]), np.array([[0.5], [2.0], [-1.0]])
    t = rr.task_terms(_cfg(1, (1, 0, 0), True), _rot_z90(), np.zeros((6, 1)), np.zeros(1), np.zeros(1), fs, fg, 1.0, 1.0, 0.0)
    assert abs(t["force_err_sq"][0] - 9.0) < 1e-15
    # the same axis read in the world frame: the x difference
    t = rr.task_terms(_cfg(1, (1, 0, 0), False), _rot_z90(), np.zeros((6, 1)), np.zeros(1), np.zeros(1), fs, fg, 1.0, 1.0, 0.0)
    assert abs(t["force_err_sq"][0] - 0.25) < 1e-15
    # two force directions (the plane normal to the axis), all three, none
    for dim, want in ((2, 0.25 + 64.0), (3, 0.25 + 9.0 + 64.0), (0, 0.0)):
        t = rr.task_terms(_cfg(dim, (1, 0, 0), True), _rot_z90(), np.zeros((6, 1)), np.zeros(1), np.zeros(1), fs, fg, 1.0, 1.0, 0.0)
        assert abs(t["force_err_sq"][0] - want) < 1e-13, dim
    # a partial task without translation rows has no force space
    t = rr.task_terms(_cfg(3, (1, 0, 0), True, P=np.zeros((3, 3))), _rot_z90(), np.zeros((6, 1)), np.zeros(1), np.zeros(1), fs, fg, 1.0, 1.0, 0.0)
    assert t["force_err_sq"][0] == 0.0
    # twist and speed terms
    v = np.array([[1.0], [2.0], [2.0], [0.0], [3.0], [4.0]])
    t = rr.task_terms(_cfg(0, (0, 0, 1), False), _rot_z90(), v, np.zeros(1), np.zeros(1), fs, fg, 1.0, 1.0, 0.0)
    assert t["lin_vel_sq"][0] == 9.0 and t["ang_vel_sq"][0] == 25.0


def test_global_terms_and_a_done_byte_with_two_bits():
    dq, tau, prev = np.array([[1.0, 0.0], [2.0, 0.0]]), np.array([[3.0, 1.0], [4.0, 1.0]]), np.array([[1.0, 0.0], [1.0, 0.0]])
    done = np.array([2 | 32, 0], dtype=np.uint8)
    value = np.array([10.0, -1.0, -2.0, -4.0, -8.0, 0.5])
    g = rr.global_terms(dq, tau, prev, np.array([True, False]), np.array([1.0, 1.0]), 0.0, done, value)
    assert np.array_equal(g["alive"], [1.0, 1.0]) and np.array_equal(g["joint_speed"], [5.0, 0.0]) and np.array_equal(g["torque"], [25.0, 2.0])
    assert np.array_equal(g["torque_rate"], [13.0, 0.0])  # robot 1 has no valid tau_prev
    assert np.array_equal(g["done"], [-0.5, 0.0])


def test_fold_is_a_multiply_and_an_add_per_step():
    w, a, b = 0.1, 3.0, 0.7
    r = rr.fold([np.array([a]), np.array([b])], [w, w])
    assert r[0] == (0.0 + w * a) + w * b
    r, bad = rr.replace_nonfinite(np.array([1.0, np.nan, np.inf, -np.inf]), -7.0)
    assert np.array_equal(r, [1.0, -7.0, -7.0, -7.0]) and list(bad) == [False, True, True, True]


def test_the_fold_of_return_and_discount_over_five_steps_with_a_done_in_the_middle():
    s = rr.start_state(1)
    r = [1.0, 2.0, 4.0, 8.0, 16.0]
    done = [0, 0, 32, 0, 0]
    step = [1, 2, 3, 1, 2]
    seen = []
    for k in range(5):
        rr.accumulate(s, np.array([r[k]]), np.array([done[k]], np.uint8), np.array([step[k]]), 0.5)
        seen.append((s["ret"][0], s["disc"][0], s["last_return"][0], int(s["last_length"][0])))
    assert seen == [(1.0, 0.5, 0.0, 0), (2.0, 0.25, 0.0, 0), (0.0, 1.0, 3.0, 3), (8.0, 0.5, 3.0, 3), (16.0, 0.25, 3.0, 3)]
    assert s["last_length"].dtype == np.int32
