"""A numpy evaluation of sai2b_apply_action (include/sai2b.h "actions"): the reference the GPU tests hold the kernel to.

It restates the mapping from the header, not from the kernel: the rotation exponential is the matrix power series of [w]x,
summed until a term no longer changes the sum (after halving the argument until |w| <= 1/2, and squaring back), where the
kernel evaluates Rodrigues' closed form with a series branch; the product with the base is a plain matrix product, where the
kernel adds a delta to the base.

Shapes are the library's: batch-minor [rows][B]. `kinds` describes the hierarchy, one entry per task: ("mft",) or
("jt", task_dof). `tasks` is the dict Controller.action_config takes: task index -> settings (mode, blocks, scales,
limits); `clip` its clip_actions."""
import numpy as np

MFT_POS, MFT_ROT, MFT_FORCE, MFT_MOMENT = slice(0, 3), slice(3, 12), slice(24, 27), slice(27, 30)
BLOCKS = ("position", "orientation", "force", "moment")  # row order inside a MotionForceTask


def skew(w):
    """[B][3] -> [B][3][3]"""
    W = np.zeros(w.shape[:-1] + (3, 3))
    W[..., 0, 1], W[..., 0, 2] = -w[..., 2], w[..., 1]
    W[..., 1, 0], W[..., 1, 2] = w[..., 2], -w[..., 0]
    W[..., 2, 0], W[..., 2, 1] = -w[..., 1], w[..., 0]
    return W


def expm_so3(w):
    """exp([w]x) for rotation vectors w [B][3] -> [B][3][3]: power series to convergence, with scaling and squaring"""
    w = np.asarray(w, dtype=np.float64)
    norm = float(np.abs(w).max()) if w.size else 0.0
    squarings = 0
    while norm > 0.5:
        norm *= 0.5
        squarings += 1
    W = skew(w / 2.0**squarings)
    E = np.broadcast_to(np.eye(3), W.shape).copy()
    term = E.copy()
    for n in range(1, 200):
        term = term @ W / n
        new = E + term
        if np.array_equal(new, E):
            break
        E = new
    else:
        raise AssertionError("the exponential series did not converge")
    for _ in range(squarings):
        E = E @ E
    return E


def layout(kinds, tasks):
    """dict name -> slice of action rows, as Controller.action_layout names them, and the number of rows"""
    out, row = {}, 0
    for t, kind in enumerate(kinds):
        s = tasks.get(t)
        if not s or s.get("mode", "none") == "none":
            continue
        if kind[0] == "jt":
            out[f"joints{t}"] = slice(row, row + kind[1])
            row += kind[1]
        else:
            for name in BLOCKS:
                if name in s["blocks"]:
                    out[f"{name}{t}"] = slice(row, row + 3)
                    row += 3
    return out, row


def _vec(v, n):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))[:, None]


def apply_action(kinds, tasks, clip, goals, pose, Sq, action, mask=None, state_finite=None):
    """goals: list per task of [rows][B] arrays (MotionForceTask 30 rows, JointTask 3 task_dof); pose: dict task -> (pos [3][B],
    rot [9][B] row-major) of the robot as it is now; Sq: dict task -> [task_dof][B]; action [rows][B]; mask [B] or None;
    state_finite [B] bool or None (all finite). -> (new goals, dict of [B] bool 'rejected', 'clipped', 'limited')"""
    action = np.asarray(action, dtype=np.float64)
    B = action.shape[1]
    lay, rows = layout(kinds, tasks)
    assert action.shape == (rows, B)
    selected = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
    finite = np.isfinite(action).all(axis=0)
    reads_state = any(s.get("mode") == "delta_current" or ("position" in s.get("blocks", ()) and s.get("max_pos_lead", np.inf) < np.inf)
                      for t, s in tasks.items() if s.get("mode", "none") != "none")
    if reads_state and state_finite is not None:
        finite = finite & state_finite
    accept = selected & finite
    clipped = (np.abs(action) > 1.0).any(axis=0) & bool(clip)
    limited = np.zeros(B, bool)
    with np.errstate(invalid="ignore"):
        a_all = np.clip(action, -1.0, 1.0) if clip else action
    new = [g.copy() for g in goals]

    def clamp(v, lo, hi):
        nonlocal limited
        lo, hi = _vec(lo, v.shape[0]), _vec(hi, v.shape[0])
        with np.errstate(invalid="ignore"):
            hit = (v < lo) | (v > hi)
            limited = limited | hit.any(axis=0)
            return np.where(v < lo, lo, np.where(v > hi, hi, v))

    for t, kind in enumerate(kinds):
        s = tasks.get(t)
        if not s or s.get("mode", "none") == "none":
            continue
        mode, G = s["mode"], goals[t]
        if kind[0] == "jt":
            k0 = kind[1]
            a = a_all[lay[f"joints{t}"]]
            base = {"delta_goal": G[:k0], "delta_current": Sq.get(t), "absolute": np.zeros((k0, B))}[mode]
            g = clamp(base + _vec(s.get("jt_scale", 1.0), k0) * a, s.get("jt_lower", -np.inf), s.get("jt_upper", np.inf))
            new[t][:k0] = g
            continue
        if "position" in s["blocks"]:
            a = a_all[lay[f"position{t}"]]
            base = {"delta_goal": G[MFT_POS], "delta_current": pose[t][0] if t in pose else None, "absolute": np.zeros((3, B))}[mode]
            p = clamp(base + _vec(s.get("pos_scale", 1.0), 3) * a, s.get("pos_lower", -np.inf), s.get("pos_upper", np.inf))
            lead = float(s.get("max_pos_lead", np.inf))
            if lead < np.inf:
                x = pose[t][0]
                with np.errstate(invalid="ignore", divide="ignore"):
                    e = p - x
                    n = np.sqrt((e * e).sum(axis=0))
                    over = n > lead
                    p = np.where(over, x + e * (lead / n), p)
                limited = limited | over
            new[t][MFT_POS] = p
        if "orientation" in s["blocks"]:
            a = a_all[lay[f"orientation{t}"]]
            with np.errstate(invalid="ignore"):
                w = np.where(np.isfinite(a), float(s.get("ori_scale", 1.0)) * a, 0.0)  # rejected robots are not written anyway
            E = expm_so3(w.T)
            Rb = {"delta_goal": G[MFT_ROT], "delta_current": pose[t][1] if t in pose else None, "absolute": np.tile(np.eye(3).reshape(9, 1), (1, B))}[mode]
            Rn = E @ Rb.T.reshape(B, 3, 3)
            new[t][MFT_ROT] = Rn.reshape(B, 9).T
        if "force" in s["blocks"]:
            new[t][MFT_FORCE] = float(s.get("force_scale", 1.0)) * a_all[lay[f"force{t}"]]
        if "moment" in s["blocks"]:
            new[t][MFT_MOMENT] = float(s.get("moment_scale", 1.0)) * a_all[lay[f"moment{t}"]]
    for t in range(len(kinds)):  # robots that are masked out or rejected keep every row as it was
        new[t][:, ~accept] = goals[t][:, ~accept]
    flags = {"rejected": selected & ~finite, "clipped": clipped & accept, "limited": limited & accept}
    return new, flags
