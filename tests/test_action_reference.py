"""Known answers for tests/action_reference.py, the numpy evaluation sai2b_apply_action is held to on the GPU."""
import numpy as np

import action_reference as ar
from sai2_primitives_perso_amd import _abi

# the reference names and orders the blocks and modes as the ABI mirror does
assert ar.BLOCKS == tuple(_abi.ACT_BLOCKS) and {"delta_goal", "delta_current", "absolute", "none"} == set(_abi.ACT_MODES)

KINDS = [("mft",), ("jt", 7)]


def _goals(B, rng):
    g = rng.normal(size=(30, B))
    R = ar.expm_so3(rng.normal(size=(B, 3)))
    g[ar.MFT_ROT] = R.reshape(B, 9).T
    return [g, rng.normal(size=(21, B))]


def test_zero_action_in_delta_goal_is_the_identity():
    B = 17
    goals = _goals(B, np.random.default_rng(0))
    tasks = {0: dict(mode="delta_goal", blocks=("position", "orientation"), pos_scale=0.3, ori_scale=0.7), 1: dict(mode="delta_goal", jt_scale=0.2)}
    lay, rows = ar.layout(KINDS, tasks)
    assert rows == 13 and lay == {"position0": slice(0, 3), "orientation0": slice(3, 6), "joints1": slice(6, 13)}
    new, flags = ar.apply_action(KINDS, tasks, True, goals, {}, {}, np.zeros((rows, B)))
    assert all(np.array_equal(a, b) for a, b in zip(new, goals))
    assert not any(f.any() for f in flags.values())


def test_exponential_of_a_quarter_turn_about_each_axis():
    want = {0: [[1, 0, 0], [0, 0, -1], [0, 1, 0]], 1: [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], 2: [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}
    for axis, R in want.items():
        w = np.zeros((1, 3))
        w[0, axis] = np.pi / 2
        assert np.abs(ar.expm_so3(w)[0] - np.array(R, float)).max() < 4e-16
    assert np.array_equal(ar.expm_so3(np.zeros((2, 3))), np.broadcast_to(np.eye(3), (2, 3, 3)))
    # through apply_action, absolute mode: the rows are the exponential, row-major
    tasks = {0: dict(mode="absolute", blocks=("orientation",), ori_scale=np.pi)}
    a = np.array([[0.0], [0.0], [0.5]])
    new, _ = ar.apply_action([("mft",)], tasks, False, [np.zeros((30, 1))], {}, {}, a)
    assert np.abs(new[0][ar.MFT_ROT][:, 0] - np.array(want[2], float).ravel()).max() < 4e-16


def test_box_then_lead_on_a_hand_computed_case():
    # goal (0, 0, 0), action (1, 0.5, 0) scaled by 2: (2, 1, 0); box upper (1, 3, 3): (1, 1, 0);
    # robot at (1, 1, -1), lead 0.25: e = (0, 0, 1), |e| = 1 > 0.25: p = x + 0.25 e = (1, 1, -0.75)
    tasks = {0: dict(mode="delta_goal", blocks=("position",), pos_scale=2.0, pos_lower=-3.0, pos_upper=(1.0, 3.0, 3.0), max_pos_lead=0.25)}
    goals = [np.zeros((30, 2))]
    pose = {0: (np.array([[1.0, 1.0], [1.0, 1.0], [-1.0, 0.0]]), np.tile(np.eye(3).reshape(9, 1), (1, 2)))}
    a = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 0.0]])
    new, flags = ar.apply_action([("mft",)], tasks, False, goals, pose, {}, a)
    assert np.array_equal(new[0][ar.MFT_POS][:, 0], [1.0, 1.0, -0.75])
    # the second robot: (0, 1, 0) is inside the box; e = (-1, 0, 0): p = (1 - 0.25, 1, 0)
    assert np.array_equal(new[0][ar.MFT_POS][:, 1], [0.75, 1.0, 0.0])
    assert flags["limited"].tolist() == [True, True] and not flags["clipped"].any() and not flags["rejected"].any()
    # without the lead the second robot is not limited at all
    tasks[0]["max_pos_lead"] = np.inf
    new, flags = ar.apply_action([("mft",)], tasks, False, goals, pose, {}, a)
    assert np.array_equal(new[0][ar.MFT_POS], [[1.0, 0.0], [1.0, 1.0], [0.0, 0.0]]) and flags["limited"].tolist() == [True, False]


def test_two_deltas_about_one_axis_add_their_angles():
    B = 5
    rng = np.random.default_rng(1)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    goals = _goals(B, rng)[:1]
    tasks = {0: dict(mode="delta_goal", blocks=("orientation",), ori_scale=1.0)}
    a1, a2 = np.outer(axis, rng.uniform(0.1, 0.6, B)), np.outer(axis, rng.uniform(0.1, 0.6, B))
    once, _ = ar.apply_action([("mft",)], tasks, False, goals, {}, {}, a1 + a2)
    first, _ = ar.apply_action([("mft",)], tasks, False, goals, {}, {}, a1)
    twice, _ = ar.apply_action([("mft",)], tasks, False, first, {}, {}, a2)
    assert np.abs(once[0] - twice[0]).max() < 1e-15
    R = once[0][ar.MFT_ROT].T.reshape(B, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14


def test_clip_reject_and_mask():
    tasks = {1: dict(mode="absolute", jt_scale=2.0, jt_lower=-1.5, jt_upper=1.5)}
    goals = [np.full((30, 4), 7.0), np.full((21, 4), 7.0)]
    a = np.zeros((7, 4))
    a[0] = [3.0, 0.5, np.nan, 0.9]
    new, flags = ar.apply_action(KINDS, tasks, True, goals, {}, {}, a, mask=np.array([1, 1, 1, 0]))
    assert new[1][0].tolist() == [1.5, 1.0, 7.0, 7.0] and np.array_equal(new[1][7:], goals[1][7:]) and np.array_equal(new[0], goals[0])
    assert flags["clipped"].tolist() == [True, False, False, False] and flags["limited"].tolist() == [True, False, False, False]
    assert flags["rejected"].tolist() == [False, False, True, False]
