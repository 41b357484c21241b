"""Pins tests/ik_reference.py, the numpy restatement of the inverse-kinematics law (include/sai2b.h "inverse kinematics"), on the
CPU, no GPU: its pose and Jacobian against the CPU oracle, its rotation logarithm, one step against Newton's, the monotone error,
the limits, the restart seeds against the reset sampler's draw, and the CONDITIONS on the record sets of tests/ik_cases.py that the
other IK tests take for granted (the reference converges on the near-seed sets, leaves at most 5 % of the far-seed set exhausted,
and at most 2 % of any set hangs on a rounding)."""
import numpy as np
import pytest

import ik_cases as ic
import reset_sampler_reference as rr
from ik_reference import AT_LIMIT, CONVERGED, EXHAUSTED, SEPARATION, rotation_exp, rotation_log


@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_pose_and_jacobian_equal_the_oracle(robot):
    ref = ic.reference(robot)
    lo, hi = ic.limits(robot)
    rng = np.random.default_rng(5)
    B = 50
    q = lo[:, None] + (hi - lo)[:, None] * rng.random((len(lo), B))
    x, R, J = ref.fk(q.T, jac=True)
    xo, Ro, Jo = ic.oracle_pose(robot, q)
    worst = max(np.abs(x - xo.T).max(), np.abs(R - Ro).max(), np.abs(J - Jo).max())
    print(robot, f"worst {worst:.2e}")
    assert worst < 1e-12


def test_the_logarithm_inverts_the_exponential_up_to_pi():
    rng = np.random.default_rng(6)
    axis = rng.normal(size=(400, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    near = np.array([0.0, 1e-13, 1e-9, 1e-7, 1e-6, np.pi - 1e-6, np.pi - 1e-7, np.pi - 3e-8, np.pi / 2 - 1e-9, np.pi / 2, np.pi / 2 + 1e-9])
    theta = np.concatenate([rng.uniform(0, np.pi - 1e-6, 400 - 10 * len(near)), np.repeat(near, 10)])
    r = axis[: len(theta)] * theta[:, None]
    back = rotation_log(rotation_exp(r))
    err = np.abs(back - r).max(axis=1)
    print(f"worst {err.max():.2e} at theta = {theta[err.argmax()]!r}")
    # the entries of a rotation matrix carry errors of a few ulps of 1 (1e-16 each, a dozen operations): its vector comes back to
    # 1e-13 absolutely, near 0 and near pi as anywhere
    assert err.max() < 1e-13
    # and the error of a pose against itself is exactly zero
    assert not rotation_log(np.broadcast_to(np.eye(3), (3, 3, 3)).copy()).any()


def test_one_step_without_damping_is_the_newton_step():
    ref = ic.reference("six_r", mu0=1e-14, mu_min=1e-14, rot_length=0.7)
    lo, hi = ic.limits("six_r")
    rng = np.random.default_rng(8)
    q = (lo[:, None] + (hi - lo)[:, None] * rng.uniform(0.2, 0.8, (6, 400))).T
    x, R, J = ref.fk(q, jac=True)
    sv = np.linalg.svd(J, compute_uv=False)
    ok = sv[:, -1] > 0.1  # square and well conditioned
    assert ok.sum() > 50
    q, J = q[ok], J[ok]
    e = rng.normal(size=(len(q), 6)) * 0.05
    d = ref.step(q, J, e, np.full(len(q), 1e-14))
    newton = np.linalg.solve(J, e[:, :, None])[:, :, 0]
    err = np.abs(d - newton).max()
    print(f"worst {err:.2e}")
    assert err < 1e-10


@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_an_accepted_step_never_increases_the_error_and_iterates_stay_inside_the_limits(robot):
    case = ic.far_seed(robot, 300, seed=3)
    lo, hi = ic.limits(robot)
    W = lambda ref, q: ref.norms(ref.error(case["goal"][:3].T, case["goal"][3:12].T.reshape(-1, 3, 3), *ref.fk(q.T)))[0]
    q_prev = np.clip(case["seed"], lo[:, None], hi[:, None])
    E_prev = W(ic.reference(robot), q_prev)
    moved = 0
    for k in (1, 2, 3, 5, 9):
        ref = ic.reference(robot, max_iterations=k, limit_margin=0.01)
        out = ref.solve(case["goal"], case["seed"])
        q = out["q"]
        assert (q >= ref.lo[:, None]).all() and (q <= ref.hi[:, None]).all(), k
        E = W(ref, q)
        if k > 1:
            assert (E <= E_prev).all(), k
            moved += int((E < E_prev).sum())
        E_prev = E
        at = ((q <= ref.lo[:, None]) | (q >= ref.hi[:, None])).any(axis=0)
        assert np.array_equal((out["flags"] & AT_LIMIT) != 0, at), k
    assert moved > 300


def test_restart_seeds_are_the_reset_samplers_draw_on_the_same_counters(monkeypatch):
    monkeypatch.setattr(rr, "CANDIDATE", 11)
    for robot in ic.ROBOTS:
        ref = ic.reference(robot, seed=0x1234567890ABCDEF, first_robot=4000, draw_id=9, limit_margin=0.05, restarts=3)
        robots = np.arange(70)
        for n in (1, 2, 16):
            got = ref.restart_seed(n, robots)
            want = rr.candidate(np.full(70, n), 9, (robots + 4000).astype(np.uint64), 0x1234567890ABCDEF, np.tile(ref.lo[:, None], (1, 70)),
                                np.tile(ref.hi[:, None], (1, 70)))
            assert np.array_equal(got.T, want), (robot, n)
            assert (got >= ref.lo).all() and (got <= ref.hi).all()
        assert not np.array_equal(ref.restart_seed(1, robots), ref.restart_seed(2, robots))


# ---- the conditions on the record sets the other files use
NEAR_SETS = [("panda", 4099), ("planar_4r", 200), ("six_r", 200), ("sliding_base", 200)] + [(r, 2000) for r in ic.ROBOTS]


@pytest.mark.parametrize("robot, B", NEAR_SETS, ids=lambda v: str(v))
def test_the_reference_converges_on_every_near_seed_record(robot, B):
    case, out = ic.solved(robot, "near", B, **ic.NEAR)
    assert (out["flags"] & CONVERGED).all() and out["counts"] == [B, B, 0, 0]
    ep, er = ic.reference(robot).pose_error(case["goal"], out["q"])
    assert (ep <= 1e-6).all() and (er <= 1e-6).all()
    it = out["status"][2]
    ok = ic.separated(out)
    cond = out["sigma_min"] >= ic.SIGMA_MIN
    print(f"{robot} {B}: iterations median {np.median(it):.0f} worst {it.max():.0f}; without separation {(~ok).sum()}; "
          f"sigma_min >= {ic.SIGMA_MIN}: {cond.sum()}")
    assert cond.sum() >= B // 4  # the agreement bound of tests/test_ik_law.py is measured on a set that is not thin


@pytest.mark.parametrize("robot, B", [("panda", 4099), ("six_r", 2000)], ids=lambda v: str(v))
def test_the_raw_near_seed_sets_hold_near_singular_records_and_keep_their_separation(robot, B):
    _, out = ic.solved(robot, "raw", B, **ic.NEAR)
    n = int(((out["flags"] & EXHAUSTED) != 0).sum())
    ok = ic.separated(out)
    print(f"{robot} {B}: exhausted {n}, without separation {(~ok).sum()}")
    assert 0 < n < B // 50


def test_the_far_seed_set_leaves_at_most_five_percent_exhausted():
    case, out = ic.solved("panda", "far", 4099, **ic.FAR)
    share = ((out["flags"] & EXHAUSTED) != 0).mean()
    ok = ic.separated(out)
    print(f"exhausted {share:.4f}; restarts used: {np.bincount(out['status'][3].astype(int), minlength=9).tolist()}; without separation {(~ok).sum()}")
    assert share <= 0.05
    assert (out["status"][3] > 0).any()  # some robot needed a restart


@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_the_other_sets_keep_their_separation(robot):
    for kind, B, cfg in (("limit", 200, ic.NEAR), ("unreachable", 200, dict(max_iterations=20, restarts=1, seed=3))):
        _, out = ic.solved(robot, kind, B, **cfg)
        if kind == "unreachable":  # held to the oracle alone on the GPU: a robot at rest in a local minimum has no separation
            assert (out["flags"] & EXHAUSTED).all()
        else:
            ic.separated(out)
            assert (out["flags"] & AT_LIMIT).any() or robot == "six_r"  # (not redundant: it converges off its limits)
    assert SEPARATION == 1e-9
