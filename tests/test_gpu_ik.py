"""GPU tests (-m gpu) of the inverse kinematics (csrc/sai2b_ik.hip: ik_kernel; include/sai2b.h "inverse kinematics") against
tests/ik_reference.py (numpy on the independent URDF chain), against the CPU oracle's pose and against twin contexts. The record
sets are those of tests/ik_cases.py, whose conditions tests/test_ik_reference.py asserts on the CPU; value-by-value comparisons
leave out the records without separation (at most 2 % of a set).

1: one iteration, the four robots at B = 1, 63, 64, 65, 200. 2: near-seed solves, Panda at 4 099 and the others at 200: every robot
converged, the oracle's pose at q_out within tol + 1e-12 of the goal, the status error rows within 1e-12 of the oracle's error at
q_out, q_out within the bound measured on the CPU (ik_cases.Q_BOUND) where the path is well conditioned. 3: masks. 4: limits.
5: unreachable goals. 6: non-finite inputs. 7: far seeds with restarts. 8: shards. 9: options. 10: composition with reset_robots
and observe, torch tensors on a caller stream. 11: no side effects on C3 and C4. 12: argument checks."""
import numpy as np
import pytest

import collision_cases as cc
import ik_cases as ic
import joint_sensor_reference as jr
import sai2_primitives_perso_amd as pkg
import test_gpu_subset_reset as sr
from ik_reference import AT_LIMIT, CONVERGED, EXHAUSTED, NONFINITE
from sai2_primitives_perso_amd import _abi, sharding

pytestmark = pytest.mark.gpu

TOL = 1e-12
SENTINEL = -7.25


def _controller(robot, B):
    return pkg.Controller(cc.model(robot)[0], ic.task_configs(robot), B)


def _cfg(robot, **kw):
    """the product's arguments for an ik_cases configuration (the reference's keys are the product's)"""
    kw.setdefault("axes", ic.axes_of(robot))
    return kw


def _counts_of(flags, selected):
    return dict(selected=int(selected), converged=int(((flags & CONVERGED) != 0).sum()), exhausted=int(((flags & EXHAUSTED) != 0).sum()),
                nonfinite=int(((flags & NONFINITE) != 0).sum()))


def _agree(robot, case, out, got, cond_q=True, what=None):
    """flags on the separated records, status rows 0, 1 and 4 and q_out where the path is well conditioned"""
    q, status, flags = got
    sep = ic.separated(out)
    assert np.array_equal(flags[sep], out["flags"][sep]), what
    cond = sep & (out["sigma_min"] >= ic.SIGMA_MIN)
    assert cond.sum() >= max(1, len(flags) // 4) or len(flags) < 8, what
    if cond_q and cond.any():
        err = np.abs(q[:, cond] - out["q"][:, cond]).max()
        assert err <= ic.Q_BOUND, (what, err)
        assert np.array_equal(status[2:4, cond], out["status"][2:4, cond]), what
        return err
    return 0.0


def _as_the_near_seed_cell(robot, case, out, got, tol=1e-6, axes=None, what=None):
    """what the near-seed cell asks: every robot converged (the reference too: the condition on the inputs), the oracle's pose at
    q_out within tol + 1e-12 of the goal, the status error rows within 1e-12 of the oracle's error at q_out, q_out within the bound
    measured on the CPU where the path is well conditioned"""
    q, status, flags = got
    assert (out["flags"] & CONVERGED).all(), what
    assert (flags & CONVERGED).all(), what
    ep, er = ic.oracle_error(robot, case["goal"][:12], q, axes=axes)
    assert (ep <= tol + TOL).all() and (er <= tol + TOL).all(), what
    assert np.abs(status[0] - ep).max() < TOL and np.abs(status[1] - er).max() < TOL, what
    return _agree(robot, case, out, got, what=what)


_ran = {}


def _solve(robot, kind, B, **cfg):
    """(case, reference result, device result, counts) of a record set, run once and shared"""
    key = (robot, kind, B, tuple(sorted(cfg.items())))
    if key not in _ran:
        case, out = ic.solved(robot, kind, B, **cfg)
        g = _controller(robot, B)
        g.set_ik(**_cfg(robot, **cfg))
        got = g.solve_ik(case["goal"], case["seed"])
        _ran[key] = (case, out, got, g.get_ik_counts())
    return _ran[key]


# ---------------------------------------------------------------------------------------------- 1: one iteration
@pytest.mark.parametrize("B", ic.BATCHES)
@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_one_iteration(robot, B):
    cfg = dict(max_iterations=1, step_max=0.2, limit_margin=0.01)
    case, out, (q, status, flags), counts = _solve(robot, "far", B, **cfg)
    sep = out["sep"] >= 1e-9
    assert sep.all() or (~sep).mean() <= ic.MAX_DROPPED
    assert np.array_equal(flags[sep], out["flags"][sep])
    err = max(np.abs(q[:, sep] - out["q"][:, sep]).max(), np.abs(status[:, sep] - out["status"][:, sep]).max())
    print(f"{robot} {B}: worst {err:.2e}, counts {counts}")
    assert err < TOL
    assert counts == _counts_of(flags, B)
    if sep.all():
        assert list(counts.values()) == out["counts"]


# ---------------------------------------------------------------------------------------------- 2: near seeds
NEAR = [("panda", 4099), ("planar_4r", 200), ("six_r", 200), ("sliding_base", 200)]


@pytest.mark.parametrize("robot, B", NEAR, ids=lambda v: str(v))
def test_near_seed_solves(robot, B):
    case, out, (q, status, flags), counts = _solve(robot, "near", B, **ic.NEAR)
    assert (flags & CONVERGED).all() and counts == dict(selected=B, converged=B, exhausted=0, nonfinite=0)
    ep, er = ic.oracle_error(robot, case["goal"], q)
    assert (ep <= 1e-6 + TOL).all() and (er <= 1e-6 + TOL).all()
    assert np.abs(status[0] - ep).max() < TOL and np.abs(status[1] - er).max() < TOL
    err = _agree(robot, case, out, (q, status, flags), what=(robot, B))
    print(f"{robot} {B}: worst |q - q_reference| {err:.2e} (bound {ic.Q_BOUND:.2e}); iterations median {np.median(status[2]):.0f} worst {status[2].max():.0f}")


@pytest.mark.parametrize("robot, B", [("panda", 4099), ("six_r", 2000)], ids=lambda v: str(v))
def test_near_seeds_as_they_are_drawn(robot, B):
    """the draws without the condition: the records near a singular configuration, on which 40 iterations do not suffice, included"""
    case, out, (q, status, flags), counts = _solve(robot, "raw", B, **ic.NEAR)
    assert 0 < ((out["flags"] & EXHAUSTED) != 0).sum() < B // 50  # some such records are in the set
    sep = ic.separated(out)
    assert np.array_equal(flags[sep], out["flags"][sep]) and counts == _counts_of(flags, B)
    ep, er = ic.oracle_error(robot, case["goal"], q)
    cv = (flags & CONVERGED) != 0
    assert (ep[cv] <= 1e-6 + TOL).all() and (er[cv] <= 1e-6 + TOL).all()
    assert np.abs(status[0] - ep).max() < TOL and np.abs(status[1] - er).max() < TOL
    print(f"{robot} {B}: exhausted {(~cv).sum()} (reference {((out['flags'] & EXHAUSTED) != 0).sum()}), without separation {(~sep).sum()}")


# ---------------------------------------------------------------------------------------------- 3: masks
def test_masks():
    robot, B = "panda", 4099
    case, out, (q, status, flags), _ = _solve(robot, "near", B, **ic.NEAR)
    g = _controller(robot, B)
    g.set_ik(**_cfg(robot, **ic.NEAR))
    fresh = lambda: (np.full((7, B), SENTINEL), np.full((5, B), SENTINEL), np.full(B, 0xA5, dtype=np.uint8))
    # empty: nothing written, every count zero
    q0, s0, f0 = g.solve_ik(case["goal"], case["seed"], np.zeros(B, dtype=bool), *fresh())
    assert (q0 == SENTINEL).all() and (s0 == SENTINEL).all() and (f0 == 0xA5).all()
    assert g.get_ik_counts() == dict(selected=0, converged=0, exhausted=0, nonfinite=0)
    # 1 % scattered (some wavefronts without a robot, some with one): the same robots' outputs under a full mask, bit for bit
    mask = np.zeros(B, dtype=bool)
    mask[np.random.default_rng(4).choice(B, B // 100, replace=False)] = True
    mask[[0, B - 1]] = True
    q1, s1, f1 = g.solve_ik(case["goal"], case["seed"], mask, *fresh())
    assert (q1[:, ~mask] == SENTINEL).all() and (s1[:, ~mask] == SENTINEL).all() and (f1[~mask] == 0xA5).all()
    assert np.array_equal(q1[:, mask], q[:, mask]) and np.array_equal(s1[:, mask], status[:, mask]) and np.array_equal(f1[mask], flags[mask])
    assert g.get_ik_counts() == _counts_of(f1[mask], mask.sum())
    # uint8 mask with other non-zero bytes; a full mask is the call without one
    q2, s2, f2 = g.solve_ik(case["goal"], case["seed"], np.where(mask, 7, 0).astype(np.uint8), *fresh())
    assert np.array_equal(q2, q1) and np.array_equal(s2, s1) and np.array_equal(f2, f1)
    q3, s3, f3 = g.solve_ik(case["goal"], case["seed"], np.ones(B, dtype=bool), *fresh())
    assert np.array_equal(q3, q) and np.array_equal(s3, status) and np.array_equal(f3, flags)


# ---------------------------------------------------------------------------------------------- 4: limits
@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_limits(robot):
    B = 200
    case, out, (q, status, flags), counts = _solve(robot, "limit", B, **ic.NEAR)
    lo, hi = ic.limits(robot)
    assert (q >= lo[:, None]).all() and (q <= hi[:, None]).all()
    at = ((q <= lo[:, None]) | (q >= hi[:, None])).any(axis=0)
    assert np.array_equal((flags & AT_LIMIT) != 0, at)
    sep = ic.separated(out)
    assert np.array_equal(flags[sep] & AT_LIMIT, out["flags"][sep] & AT_LIMIT) and np.array_equal(flags[sep], out["flags"][sep])
    assert at.any() or robot == "six_r"
    # with a margin the box shrinks with it
    g = _controller(robot, B)
    g.set_ik(**_cfg(robot, limit_margin=0.05, **ic.NEAR))
    q2, _, f2 = g.solve_ik(case["goal"], case["seed"])
    assert (q2 >= lo[:, None] + 0.05).all() and (q2 <= hi[:, None] - 0.05).all() and (f2 & AT_LIMIT).any()


# ---------------------------------------------------------------------------------------------- 5: unreachable goals
@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_unreachable_goals(robot):
    B = 200
    cfg = dict(max_iterations=20, restarts=1, seed=3)
    case, out, (q, status, flags), counts = _solve(robot, "unreachable", B, **cfg)
    assert (flags & EXHAUSTED).all() and not (flags & CONVERGED).any()
    assert counts == dict(selected=B, converged=0, exhausted=B, nonfinite=0)
    ep, er = ic.oracle_error(robot, case["goal"], q)
    assert np.abs(status[0] - ep).max() < TOL and np.abs(status[1] - er).max() < TOL
    assert (status[2] == 40).all() and set(status[3].tolist()) <= {0.0, 1.0}
    # the best iterate: its weighted error is no larger than the seed's
    sp, sr_ = ic.oracle_error(robot, case["goal"], case["seed"])
    L2 = 0.25**2
    assert (ep**2 + L2 * er**2 <= (sp**2 + L2 * sr_**2) * (1 + 1e-12)).all()
    assert (ep > 1.0).all()


# ---------------------------------------------------------------------------------------------- 6: non-finite inputs
def test_non_finite_inputs():
    robot, B = "panda", 200
    case, out, (q, status, flags), _ = _solve(robot, "near", 4099, **ic.NEAR)
    goal, seed = np.ascontiguousarray(case["goal"][:, :B]), np.ascontiguousarray(case["seed"][:, :B])
    bad = np.zeros(B, dtype=bool)
    bad[3::7] = True
    idx = np.nonzero(bad)[0]
    for k, b in enumerate(idx):
        (goal if k % 2 else seed)[k % 7, b] = (np.nan, np.inf, -np.inf)[k % 3]
    g = _controller(robot, B)
    g.set_ik(**_cfg(robot, **ic.NEAR))
    fresh = lambda: (np.full((7, B), SENTINEL), np.full((5, B), SENTINEL), np.full(B, 0xA5, dtype=np.uint8))
    q1, s1, f1 = g.solve_ik(goal, seed, None, *fresh())
    assert (f1[bad] == NONFINITE).all() and (q1[:, bad] == SENTINEL).all() and (s1[:, bad] == SENTINEL).all()
    assert g.get_ik_counts() == dict(selected=B, converged=B - bad.sum(), exhausted=0, nonfinite=bad.sum())
    # every other robot as in a run in which the NaN robots were simply unselected
    q2, s2, f2 = g.solve_ik(goal, seed, ~bad, *fresh())
    assert np.array_equal(q1[:, ~bad], q2[:, ~bad]) and np.array_equal(s1[:, ~bad], s2[:, ~bad]) and np.array_equal(f1[~bad], f2[~bad])
    assert np.array_equal(q1[:, ~bad], q[:, :B][:, ~bad]) and (f2[bad] == 0xA5).all()


# ---------------------------------------------------------------------------------------------- 7: far seeds, restarts
def test_far_seeds_with_restarts():
    robot, B = "panda", 4099
    case, out, (q, status, flags), counts = _solve(robot, "far", B, **ic.FAR)
    share = ((flags & EXHAUSTED) != 0).mean()
    assert ((out["flags"] & EXHAUSTED) != 0).mean() <= 0.05  # the condition on the inputs
    assert share <= 0.05 and counts == _counts_of(flags, B)
    cv = (flags & CONVERGED) != 0
    ep, er = ic.oracle_error(robot, case["goal"], q)
    assert (ep[cv] <= 1e-6 + TOL).all() and (er[cv] <= 1e-6 + TOL).all()
    assert np.abs(status[0] - ep).max() < TOL and np.abs(status[1] - er).max() < TOL
    sep = ic.separated(out)
    assert np.array_equal(status[3, sep], out["status"][3, sep]) and np.array_equal(flags[sep], out["flags"][sep])
    assert (status[3] > 0).any() and status[3].max() <= 8 and status[2].max() <= 900
    print(f"exhausted {share:.4f} (reference {((out['flags'] & EXHAUSTED) != 0).mean():.4f}); starts used {np.bincount(status[3].astype(int)).tolist()}")


# ---------------------------------------------------------------------------------------------- 8: shards
def test_two_shards_are_bit_equal_to_one_context():
    robot, B = "panda", 4099
    case, out, (q, status, flags), counts = _solve(robot, "far", B, **ic.FAR)
    total = np.zeros(4, dtype=int)
    bounds = []
    for rank in range(2):
        lo, hi = sharding.shard_bounds(B, 2, rank)
        bounds.append(hi - lo)
        c = _controller(robot, hi - lo)
        sharding.set_ik(c, 2, rank, B, **_cfg(robot, **ic.FAR))
        assert c.get_ik().first_robot == lo
        qs, ss, fs = c.solve_ik(sharding.shard_rows(case["goal"], 2, rank), sharding.shard_rows(case["seed"], 2, rank))
        assert np.array_equal(qs, q[:, lo:hi]) and np.array_equal(ss, status[:, lo:hi]) and np.array_equal(fs, flags[lo:hi]), rank
        total += np.array(list(c.get_ik_counts().values()))
    assert sum(bounds) == B
    assert total.tolist() == list(counts.values())


def test_shards_of_2048_and_2051():
    """the split the issue names: first_robot by hand"""
    robot, B = "panda", 4099
    case, out, (q, status, flags), _ = _solve(robot, "far", B, **ic.FAR)
    for lo, hi in ((0, 2048), (2048, 4099)):
        c = _controller(robot, hi - lo)
        c.set_ik(first_robot=lo, **_cfg(robot, **ic.FAR))
        qs, ss, fs = c.solve_ik(np.ascontiguousarray(case["goal"][:, lo:hi]), np.ascontiguousarray(case["seed"][:, lo:hi]))
        assert np.array_equal(qs, q[:, lo:hi]) and np.array_equal(ss, status[:, lo:hi]) and np.array_equal(fs, flags[lo:hi]), lo


# ---------------------------------------------------------------------------------------------- 9: options
def test_position_only_and_the_planar_triple():
    for robot, axes in (("panda", 0b000111), ("planar_4r", ic.PLANAR_AXES)):
        B = 200
        case = ic.near_seed(robot, B, seed=11)
        ref = ic.reference(robot, axes=axes, **ic.NEAR)
        out = ref.solve(case["goal"], case["seed"], track_sigma=True)
        g = _controller(robot, B)
        g.set_ik(axes=axes, **ic.NEAR)
        q, status, flags = g.solve_ik(case["goal"], case["seed"])
        _as_the_near_seed_cell(robot, case, out, (q, status, flags), axes=axes, what=(robot, axes))
        if axes == 0b000111:
            assert (status[1] == 0).all()  # no rotational component is selected
            full = ic.oracle_error(robot, case["goal"], q)[1]
            assert (full > 1e-3).any()  # and the orientation is indeed left free


def test_a_rest_posture_pulls_the_redundant_arm():
    robot, B = "panda", 200
    case = ic.near_seed(robot, B, seed=12)
    lo, hi = ic.limits(robot)
    rest = np.ascontiguousarray(np.tile((0.5 * (lo + hi))[:, None], (1, B)))
    rows = np.concatenate([case["goal"], rest])
    # the pull biases the fixed point: J^T W^2 e = -nu (q_rest - q) there, an error of about nu |q_rest - q| / (sigma L^2), up to
    # 3e-3 here; the tolerances are set above it, mu0 at nu so that the pull acts from the first step, and 100 iterations, with
    # which the reference converges on every record
    cfg = dict(rest_weight=1e-5, max_iterations=100, tol_pos=5e-3, tol_rot=5e-3, mu0=1e-5)
    ref = ic.reference(robot, **cfg)
    out = ref.solve(rows, case["seed"], track_sigma=True)
    g = _controller(robot, B)
    g.set_ik(**_cfg(robot, **cfg))
    assert g.ik_input_rows() == (19, 7)
    q, status, flags = g.solve_ik(rows, case["seed"])
    _as_the_near_seed_cell(robot, case, out, (q, status, flags), tol=5e-3, what="rest")
    # against the solve without it: closer to the rest posture
    g.set_ik(**_cfg(robot, **{k: v for k, v in cfg.items() if k != "rest_weight"}))
    q0, _, _ = g.solve_ik(case["goal"], case["seed"])
    assert np.linalg.norm(q - rest, axis=0).mean() < np.linalg.norm(q0 - rest, axis=0).mean()
    with pytest.raises(ValueError):
        g.solve_ik(rows, case["seed"])  # 19 rows where 12 are read


def test_goal_from_the_task_and_seed_from_the_state_in_both_views():
    robot, B = "six_r", 200
    case, out = ic.solved(robot, "near", B, **ic.NEAR)
    n = 6
    g = _controller(robot, B)
    g.set_state(case["seed"], np.zeros((n, B)))
    g.set_mft_goals(0, np.ascontiguousarray(case["goal"][:3]), np.ascontiguousarray(case["goal"][3:12]))
    g.set_ik(goal_source="task", seed_source="state", **_cfg(robot, **ic.NEAR))
    assert g.ik_input_rows() == (0, 0)
    q, status, flags = g.solve_ik()
    ref_run = _solve(robot, "near", B, **ic.NEAR)[2]
    assert np.array_equal(q, ref_run[0]) and np.array_equal(status, ref_run[1]) and np.array_equal(flags, ref_run[2])
    # a joint sensor with a calibration offset: view 'measured' seeds from the measured q, 'truth' from the plant's
    rows = jr.ideal_rows(n, B)
    rows[1 : 1 + n] = np.random.default_rng(3).uniform(-0.05, 0.05, (n, B))
    g.set_joint_sensor(rows)
    qm, _ = g.get_measured_state()
    assert np.abs(qm - case["seed"]).max() > 0.01
    g.set_ik(goal_source="task", seed_source="state", view="measured", **_cfg(robot, **ic.NEAR))
    q1, s1, f1 = g.solve_ik()
    lo, hi = ic.limits(robot)
    want = ic.reference(robot, **ic.NEAR).solve(case["goal"], qm, track_sigma=True)
    _as_the_near_seed_cell(robot, case, want, (q1, s1, f1), what="measured")
    assert not np.array_equal(q1, q)
    g.set_ik(goal_source="task", seed_source="state", view="truth", **_cfg(robot, **ic.NEAR))
    q2, s2, f2 = g.solve_ik()
    assert np.array_equal(q2, q) and np.array_equal(s2, status) and np.array_equal(f2, flags)


# ---------------------------------------------------------------------------------------------- 10: composition
def test_solve_reset_observe_and_the_torch_path_on_a_caller_stream():
    import torch

    robot, B = "panda", 200
    case = ic.far_seed(robot, B, seed=5)
    cfg = dict(max_iterations=30)
    g = _controller(robot, B)
    g.set_ik(**_cfg(robot, **cfg))
    start = np.ascontiguousarray(case["seed"])
    g.set_state(start, np.zeros((7, B)))
    g.reinitialize()
    g.set_observation(blocks=("q",), tasks=[0], task_blocks=("pose",))
    hq, hs, hf = g.solve_ik(case["goal"], case["seed"])
    assert 0 < ((hf & CONVERGED) != 0).sum() < B  # some converge in 30 iterations from far seeds, some do not
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        goal, seed = torch.from_numpy(case["goal"]).cuda(non_blocking=True), torch.from_numpy(case["seed"]).cuda(non_blocking=True)
        dq_, ds, df = torch.full((7, B), SENTINEL, dtype=torch.float64, device="cuda"), torch.zeros((5, B), dtype=torch.float64, device="cuda"), \
            torch.zeros(B, dtype=torch.uint8, device="cuda")
        g.solve_ik(goal, seed, None, dq_, ds, df)
        mask = df & 1
        g.reset_robots(mask, dq_, torch.zeros_like(dq_))
    stream.synchronize()
    g.synchronize()
    assert np.array_equal(dq_.cpu().numpy(), hq) and np.array_equal(ds.cpu().numpy(), hs) and np.array_equal(df.cpu().numpy(), hf)
    obs, _ = g.observe()
    lay = g.observation_layout()
    cv = (hf & CONVERGED) != 0
    pose = obs[lay["pose0"]]
    assert np.linalg.norm(pose[:3, cv] - case["goal"][:3, cv], axis=0).max() <= 1e-6 + TOL
    assert np.array_equal(obs[lay["q"]][:, cv], hq[:, cv]) and np.array_equal(obs[lay["q"]][:, ~cv], start[:, ~cv])
    # a JointTask goal from a pose
    g.set_jt_goals(1, dq_)
    g.synchronize()


# ---------------------------------------------------------------------------------------------- 11: no side effects
@pytest.mark.parametrize("name", ["c3", "c4"])
def test_six_ticks_are_bit_equal_to_a_twin_that_never_made_the_calls(name, monkeypatch):
    s = sr.scenario(name)
    a, twin = sr.contexts(s, 2, monkeypatch)
    words = a.snapshot_words()
    launches = a.counters()[0]
    a.set_ik(task=s.kinds.index("mft"), max_iterations=10, restarts=2, seed=5)
    assert a.counters()[0] == launches  # configuring launches nothing
    rng = np.random.default_rng(9)
    goal = np.concatenate([rng.uniform(-0.5, 0.5, (3, sr.B)), np.tile(np.eye(3).reshape(9, 1), (1, sr.B))])
    every = np.ones(sr.B, dtype=bool)
    for k in range(6):
        if k % 2 == 0:
            a.solve_ik(goal, s.q1)
            assert a.counters()[0] == launches + 1
        ta, tt = sr.period(a), sr.period(twin)
        launches = a.counters()[0]
        sr.assert_columns([ta] + sr.snapshot(a, s.kinds), [tt] + sr.snapshot(twin, s.kinds), every, (name, k))
    assert a.snapshot_words() == words == twin.snapshot_words()
    a.clear_ik()
    with pytest.raises(ValueError, match="no inverse kinematics"):
        a.solve_ik(goal, s.q1)


# ---------------------------------------------------------------------------------------------- 12: argument checks
def test_argument_checks():
    import ctypes as C

    robot, B = "panda", 63
    g = _controller(robot, B)
    launches = g.counters()[0]
    goal, seed = np.zeros((12, B)), np.zeros((7, B))
    for call in (lambda: g.solve_ik(goal, seed), g.get_ik_counts, g.get_ik):
        with pytest.raises(ValueError, match="no inverse kinematics"):
            call()
    with pytest.raises(ValueError, match="MotionForceTask"):
        g.set_ik(task=1)  # the JointTask
    with pytest.raises(ValueError, match="task"):
        g.set_ik(task=2)  # beyond the hierarchy
    with pytest.raises(ValueError, match="no inverse kinematics"):
        g.get_ik()  # a failing call leaves the context as it was
    g.set_ik()
    lib, h = g.lib, g.h
    q, st, fl = np.zeros((7, B)), np.zeros((5, B)), np.zeros(B, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for args, word in (((None, p(seed), None, p(q), p(st), p(fl)), "goal_rows"), ((p(goal), None, None, p(q), p(st), p(fl)), "seed_rows"),
                       ((p(goal), p(seed), None, None, p(st), p(fl)), "q_out"), ((p(goal), p(seed), None, p(q), None, p(fl)), "status"),
                       ((p(goal), p(seed), None, p(q), p(st), None), "flags")):
        assert lib.sai2b_solve_ik(h, *args, 0) == _abi.INVALID_ARGUMENT and word in lib.sai2b_last_error(h).decode()
    assert lib.sai2b_get_ik_counts(h, None) == _abi.INVALID_ARGUMENT
    assert g.counters()[0] == launches  # none of this launched anything
    with pytest.raises(ValueError):
        g.solve_ik(goal[:11], seed)
    with pytest.raises(ValueError):
        g.solve_ik(goal, seed, np.zeros(B + 1, dtype=bool))
    g.solve_ik(goal, seed)
    assert g.counters()[0] == launches + 1 and g.get_ik_counts()["selected"] == B
