"""numpy restatement of include/sai2b.h "rewards and episode returns", for the tests. Its inputs are rows of the CPU oracle
(oracle_lib: pose, J dq, the error norms, the sensed world force, the goal force, the limit margin) and sigma_force built here
from the task's own force-space configuration and the oracle's rotation; the library's get_mft_sigma is not used.

All per-robot quantities are arrays with the batch last ([B] or [k][B])."""
import numpy as np

TERMS = ("alive", "joint_speed", "torque", "torque_rate", "limit", "done")  # flag order = storage order
TASK_TERMS = ("pos", "pos_sq", "pos_tanh", "ori", "ori_sq", "ori_tanh", "lin_vel_sq", "ang_vel_sq", "force_err_sq", "force_excess")
DONE_REASONS = 6


def sigma_force(cfg, rot):
    """sigmaForce of a MotionForceTask (MotionForceTask.cpp:892-971) -> [B][3][3]. cfg: the task's configuration
    (force_space_dimension, force_axis, parametrization_in_compliant_frame, partial_projection); rot [9][B]: the compliant
    frame's orientation in the world, row-major."""
    B = rot.shape[1]
    R = rot.T.reshape(B, 3, 3)
    P = np.array(list(cfg.partial_projection)).reshape(6, 6)[:3, :3]
    axis = np.array(list(cfg.force_axis), dtype=np.float64)
    a = R @ axis if cfg.parametrization_in_compliant_frame else np.broadcast_to(axis, (B, 3))
    aa = a[:, :, None] * a[:, None, :]
    dim = cfg.force_space_dimension
    if dim == 3:
        return np.broadcast_to(P, (B, 3, 3)).copy()
    A = {0: np.zeros((B, 3, 3)), 1: aa, 2: np.eye(3) - aa}[dim]
    return P @ A @ P.T


def done_term(done, done_value):
    """sum_r done_value[r] * bit r, added in the order of the bits"""
    v = np.zeros(done.shape)
    for r in range(DONE_REASONS):
        v = v + done_value[r] * ((done >> r) & 1).astype(np.float64)
    return v


def global_terms(dq, tau, tau_prev, tau_prev_valid, margin, limit_soft_margin, done, done_value):
    """name -> [B]. tau_prev [dof][B] with tau_prev_valid [B] (bool): TORQUE_RATE is 0 where it is not valid"""
    rate = ((tau - tau_prev) ** 2).sum(axis=0)
    return dict(alive=np.ones(dq.shape[1]), joint_speed=(dq * dq).sum(axis=0), torque=(tau * tau).sum(axis=0),
                torque_rate=np.where(tau_prev_valid, rate, 0.0), limit=np.maximum(0.0, limit_soft_margin - margin),
                done=done_term(done, done_value))


def task_terms(cfg, rot, twist, pos_norm, ori_norm, sensed_force_world, goal_force, pos_scale, ori_scale, force_soft_limit):
    """name -> [B] for one MotionForceTask. twist [6][B] = J dq; the norms are rows 6 and 7 of the ERROR observation block"""
    sf = sigma_force(cfg, rot)
    df = np.einsum("bij,jb->ib", sf, sensed_force_world - goal_force)
    fn = np.sqrt((sensed_force_world ** 2).sum(axis=0))
    return dict(pos=pos_norm, pos_sq=pos_norm * pos_norm, pos_tanh=1.0 - np.tanh(pos_norm / pos_scale),
                ori=ori_norm, ori_sq=ori_norm * ori_norm, ori_tanh=1.0 - np.tanh(ori_norm / ori_scale),
                lin_vel_sq=(twist[:3] ** 2).sum(axis=0), ang_vel_sq=(twist[3:] ** 2).sum(axis=0),
                force_err_sq=(df ** 2).sum(axis=0), force_excess=np.maximum(0.0, fn - force_soft_limit))


def fold(rows, weights):
    """r = sum weight * row in the order given, from 0.0: a multiply and an add of their own per step (numpy never fuses them)"""
    r = np.zeros(np.asarray(rows[0]).shape) if len(rows) else 0.0
    for w, v in zip(weights, rows):
        p = w * np.asarray(v)
        r = r + p
    return r


def replace_nonfinite(r, nonfinite_reward):
    """-> (reward, replaced [B] bool)"""
    bad = ~np.isfinite(r)
    return np.where(bad, nonfinite_reward, r), bad


def accumulate(state, r, done, step, gamma):
    """one call's update of the accumulators, in place. state: dict of [B] arrays ret, disc, last_return, last_length;
    done [B] the call's byte, step [B] the episode step the call reported"""
    p = state["disc"] * r
    ret = state["ret"] + p
    disc = state["disc"] * gamma
    closed = done != 0
    state["last_return"] = np.where(closed, ret, state["last_return"])
    state["last_length"] = np.where(closed, step, state["last_length"]).astype(np.int32)
    state["ret"] = np.where(closed, 0.0, ret)
    state["disc"] = np.where(closed, 1.0, disc)
    return state


def start_state(B):
    return dict(ret=np.zeros(B), disc=np.ones(B), last_return=np.zeros(B), last_length=np.zeros(B, dtype=np.int32))
