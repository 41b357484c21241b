"""sai2b_reset_robots_sampled (include/sai2b.h "episode starts") on the GPU against tests/reset_sampler_reference.py.

Tolerances: tries, q, the counts and the episode counters are exact (the candidates are one product and one sum of exact
uniforms; every seed used here has no candidate of any try of any robot within 1e-9 of a threshold on the reference, which each
test asserts); dq within 4e-15 relative (log / sin / cos of the two maths libraries, the hardware test's bound for the normals);
goals within 1e-12 (the start pose of two forward kinematics plus an offset of order 1)."""
import numpy as np
import pytest

import contact_cases as cc
import oracle_lib as ol
import plumbing
import reset_sampler_reference as rr
import sai2_primitives_perso_amd as pkg
import test_gpu_subset_reset as sr
from sai2_primitives_perso_amd import _abi, sharding

pytestmark = pytest.mark.gpu

DQ_TOL, GOAL_TOL = 4e-15, 1e-12
FRAME_POS = (0.01, 0.02, 0.06)
ROBOTS = {"planar_4r": 4, "six_r": 6, "panda": 7, "sliding_base": 8}


def _mask(B, seed, p=0.6):
    m = np.random.default_rng([B, seed]).uniform(size=B) < p
    m[0] = True
    return m


def _everything(g, kinds):
    return sr.snapshot(g, kinds) + [plumbing.device_rows(g, _abi.BUF_TAU, -1, g.dof)]


def _equal_columns(a, b, cols, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x[..., cols], y[..., cols], equal_nan=True), (what, i)


def _check_draws(g, ref, out, mask, kinds):
    st = g.reset_sampler_state()
    q, dq = g.get_state()
    assert np.array_equal(st["tries"][mask], out["tries"][mask])
    assert np.array_equal(q[:, mask], out["q"][:, mask])
    scale = np.maximum(np.abs(out["dq"][:, mask]), 1e-300)
    assert (np.abs(dq[:, mask] - out["dq"][:, mask]) <= DQ_TOL * scale).all()
    assert not dq[:, out["exhausted"]].any() and not np.signbit(dq[:, out["exhausted"]]).any()
    for t, want in out["goals"].items():
        if kinds[t] == "mft":
            got = g.get_mft_goals(t)
            assert np.abs(got[0][:, mask] - want[0][:, mask]).max() <= GOAL_TOL
            assert np.abs(got[1][:, mask] - want[1][:, mask]).max() <= GOAL_TOL
            assert not any(np.any(x[:, mask]) for x in got[2:])
        else:
            got = g.get_jt_goals(t)
            assert np.abs(got[0][:, mask] - want[:, mask]).max() <= GOAL_TOL and not got[1][:, mask].any() and not got[2][:, mask].any()
    assert tuple(g.reset_sampler_counts().values()) == out["counts"]
    assert np.array_equal(st["episode"], ref.e)
    assert ref.borderline() == 0


# ------------------------------------------------------------------------------- the Panda case of the issue: ratio 0.06, 8 tries
def _panda(B, cfg_kw, rows_kw=None, first_robot=0):
    g = pkg.Controller(pkg.panda_model(), [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    cfg = g.reset_sampler_config(first_robot=first_robot, **cfg_kw)
    rows = g.reset_sampler_rows(cfg, **(rows_kw or {}))
    g.set_reset_sampler(cfg, rows)
    return g, cfg, rows


PANDA_CFG = dict(seed=20261020, max_tries=8, goal_tasks=(0, 1), ratio_task=0, min_ratio=0.06)
PANDA_ROWS = dict(dq_sigma=np.array([0.3, 0.2, 0.0, 0.1, 0.5, 0.05, 0.4]),
                  goals={0: dict(pos_lower=(-0.1, -0.05, 0.0), pos_upper=(0.1, 0.05, 0.2), theta_max=0.7), 1: dict(half_width=0.25)})


def _panda_reference(B, first_robot=0, rows=None, cfg=PANDA_CFG):
    c = dict(first_robot=first_robot, absolute_position=0, box_task=-1, box_lower=(0, 0, 0), box_upper=(0, 0, 0), clearance=None, **cfg)
    c["goal_tasks"] = sum(1 << t for t in cfg["goal_tasks"])
    return rr.ResetSamplerReference(7, B, [("mft",), ("jt", 7, None)], c, rows, rr.panda_kinematics(0))


def test_panda_ratio_criterion_4099():
    B = 4099
    g, cfg, rows = _panda(B, PANDA_CFG, PANDA_ROWS)
    twin, _, _ = _panda(B, PANDA_CFG, PANDA_ROWS)
    q0 = np.random.default_rng(5).uniform(-0.5, 0.5, (7, B)) + np.array([0, 0, 0, -1.5, 0, 1.5, 0])[:, None]
    for c in (g, twin):
        c.set_state(q0, 0.1 * q0)
        c.reinitialize()
    ref = _panda_reference(B, rows=rows)
    mask = _mask(B, 1)
    out = ref.reset(mask)
    t = out["tries"][mask]
    assert (t == 1).any() and ((t > 1) & (t <= 8)).any() and (t == 9).any()  # first try, a later one, exhausted
    g.reset_robots_sampled(mask)
    _check_draws(g, ref, out, mask, ["mft", "jt"])
    qn = g.get_reset_sampler()[1][21:28]
    assert np.array_equal(g.get_state()[0][:, out["exhausted"]], qn[:, out["exhausted"]])
    _equal_columns(_everything(g, ["mft", "jt"]), _everything(twin, ["mft", "jt"]), ~mask, "unselected")
    # a second call draws another episode, for the robots of its own mask
    mask2 = _mask(B, 2, 0.3)
    out2 = ref.reset(mask2)
    g.reset_robots_sampled(mask2)
    _check_draws(g, ref, out2, mask2, ["mft", "jt"])
    both = mask & mask2
    assert not np.array_equal(out["q"][:, both], out2["q"][:, both])


# ------------------------------------------------------------------------------- every robot size, box criterion, both goal kinds
def _generic(robot, B, seed, cfg_kw, contact=None, otg=True, partial=None):
    m = cc.model(robot)
    n = int(m.dof)
    link = n - 1
    mk = lambda M, J: [M("m", link=link, frame_pos=FRAME_POS, partial=partial, robot_dof=n, internal_otg=otg), J("j", robot_dof=n, internal_otg=otg)]
    g = pkg.Controller(m, mk(pkg.motion_force_task_config, pkg.joint_task_config), B)
    t0 = g.tasks[0]  # the projection the library built from the directions, and its rank: what criterion (a) multiplies J with
    P = {0: (np.array(t0.partial_projection[:]).reshape(6, 6), int(t0.pos_range + t0.ori_range))} if partial is not None else None
    if contact is not None:
        g.set_contact(contact["link"], contact["points"], contact["rows"][0:3], contact["rows"][3:6], contact["rows"][6], contact["rows"][7],
                      contact["rows"][8])
    cfg = g.reset_sampler_config(seed=seed, **cfg_kw)
    rng = np.random.default_rng([n, B, seed])
    rows = g.reset_sampler_rows(cfg, dq_sigma=rng.uniform(0, 1, (n, B)) * (rng.uniform(size=(n, B)) < 0.7),
                                goals={0: dict(pos_lower=rng.uniform(-0.2, 0, (3, B)), pos_upper=rng.uniform(0, 0.2, (3, B)),
                                               theta_max=rng.uniform(0, 3.0, B) * (np.arange(B) % 3 != 0)),
                                       1: dict(half_width=rng.uniform(0, 0.5, (n, B)))})
    g.set_reset_sampler(cfg, rows)
    kin = rr.oracle_kinematics(m, {0: mk(ol.motion_force_task, ol.joint_task)[0]}, B,
                               None if contact is None else (contact["link"], contact["points"]))
    c = dict(seed=seed, first_robot=0, max_tries=cfg.max_tries, goal_tasks=cfg.goal_tasks, absolute_position=cfg.absolute_position,
             ratio_task=cfg.ratio_task, min_ratio=cfg.min_ratio, box_task=cfg.box_task, box_lower=tuple(cfg.box_lower),
             box_upper=tuple(cfg.box_upper), clearance=cfg.clearance if cfg.use_clearance else None)
    ref = rr.ResetSamplerReference(n, B, [("mft",), ("jt", n, None)], c, rows, kin, None if contact is None else contact["rows"], P=P)
    return g, ref, m


def _box(robot, B):
    """a box that holds roughly half of the default-range control points"""
    m = cc.model(robot)
    n = int(m.dof)
    kin = rr.oracle_kinematics(m, {0: ol.motion_force_task("m", link=n - 1, frame_pos=FRAME_POS, robot_dof=n)}, 256)
    lo, hi = np.array(m.q_lower[:n]), np.array(m.q_upper[:n])
    q = (0.5 * (lo + hi))[:, None] + 0.8 * (0.5 * (hi - lo))[:, None] * np.random.default_rng(n).uniform(-1, 1, (n, 256))
    x = kin(q)["x"][0]
    med = np.median(x, axis=1)
    return tuple(med - np.array([10.0, 10.0, 0.0])), tuple(med + 10.0)  # the half space z >= median, bounded


@pytest.mark.parametrize("robot, B", [("planar_4r", 65), ("six_r", 63), ("panda", 64), ("sliding_base", 200), ("planar_4r", 1), ("sliding_base", 1)])
def test_box_criterion_and_goals_every_robot_size(robot, B):
    lo, hi = _box(robot, B)
    if robot == "planar_4r":  # planar: z is constant, split along x
        lo, hi = (lo[0] + 10.0, lo[1], lo[2] - 10.0), hi
    g, ref, m = _generic(robot, B, 7 + B, dict(max_tries=4, goal_tasks=(0, 1), absolute_position=(0,) if B == 63 else (), box_task=0,
                                               box_lower=lo, box_upper=hi))
    mask = _mask(B, 3)
    out = ref.reset(mask)
    g.reset_robots_sampled(mask)
    _check_draws(g, ref, out, mask, ["mft", "jt"])
    if B > 1:
        assert (out["tries"][mask] > 1).any() and (out["tries"][mask] == 1).any()


@pytest.mark.parametrize("robot", ["six_r", "sliding_base"])
def test_all_three_criteria(robot):
    B = 200
    n = ROBOTS[robot]
    contact = cc.draw(robot, B, 4, seed=1, link=n - 1)
    lo, hi = _box(robot, B)
    g, ref, m = _generic(robot, B, 11, dict(max_tries=16, goal_tasks=(0, 1), ratio_task=0, min_ratio=0.02, box_task=0, box_lower=lo, box_upper=hi,
                                            clearance=0.0), contact=contact)
    mask = _mask(B, 4)
    out = ref.reset(mask)
    g.reset_robots_sampled(mask)
    _check_draws(g, ref, out, mask, ["mft", "jt"])
    assert {m_[1] for m_ in ref.margins} == {"ratio", "box", "clearance"} and (out["tries"][mask] > 1).any()


PLANAR = (np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[0, 0, 1.0]]))  # x, y and the turn about z: rank 3
POSITION = (np.eye(3), np.zeros((0, 3)))  # the three translations alone
OBLIQUE = (np.array([[0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]), np.array([[1.0, 0, 0], [0, 0.6, 0.8]]))  # a projection that is not diagonal: rank 4


@pytest.mark.parametrize("robot, partial, rank, min_ratio", [("planar_4r", PLANAR, 3, 0.15), ("panda", POSITION, 3, 0.18), ("sliding_base", OBLIQUE, 4, 0.2),
                                                              ("planar_4r", None, 6, 0.0)])
def test_ratio_of_a_partial_task_and_of_a_robot_with_fewer_joints_than_rows(robot, partial, rank, min_ratio):
    """criterion (a) as the law states it: the singular values of P J with P the task's partial projection, s_(rank-1) / s_0; a
    six-row task on four joints has s_5 = 0, ratio 0: accepted at min_ratio 0, never above it"""
    B = 65
    g, ref, m = _generic(robot, B, 17, dict(max_tries=6, goal_tasks=(0, 1), ratio_task=0, min_ratio=min_ratio), partial=partial)
    if partial is not None:
        assert ref.P[0][1] == rank and not np.array_equal(ref.P[0][0], np.eye(6))
        if partial is OBLIQUE:
            assert np.count_nonzero(ref.P[0][0] - np.diag(np.diag(ref.P[0][0]))) > 0
    mask = _mask(B, 9)
    out = ref.reset(mask)
    g.reset_robots_sampled(mask)
    t = out["tries"][mask]
    if min_ratio > 0:
        assert (t == 1).any() and (t > 1).any()
        _check_draws(g, ref, out, mask, ["mft", "jt"])
    else:
        assert (t == 1).all() and tuple(g.reset_sampler_counts().values()) == out["counts"]
        assert np.array_equal(g.get_state()[0][:, mask], out["q"][:, mask])
        # any positive threshold rejects every candidate of the four-joint robot: s_5 is 0 up to rounding
        g2, ref2, _ = _generic(robot, B, 17, dict(max_tries=3, goal_tasks=(0, 1), ratio_task=0, min_ratio=1e-6))
        g2.reset_robots_sampled(mask)
        assert (g2.reset_sampler_state()["tries"][mask] == 4).all() and g2.reset_sampler_counts()["exhausted"] == int(mask.sum())


@pytest.mark.parametrize("robot, n_points, inner", [("panda", 1, False), ("panda", 4, True), ("planar_4r", 4, False), ("sliding_base", 1, True)])
def test_clearance_alone(robot, n_points, inner):
    import external_wrench_cases as wc

    B = 65
    n = ROBOTS[robot]
    contact = cc.draw(robot, B, n_points, seed=2, link=wc.INNER[robot] if inner else n - 1)
    g, ref, m = _generic(robot, B, 13, dict(max_tries=6, goal_tasks=(0, 1), clearance=0.01), contact=contact)
    mask = _mask(B, 5)
    out = ref.reset(mask)
    g.reset_robots_sampled(mask)
    _check_draws(g, ref, out, mask, ["mft", "jt"])
    t = out["tries"][mask]
    assert (t == 1).any() and (t > 1).any()
    # after the contact is cleared the call is refused and nothing moves
    before = g.get_state()
    g.clear_contact()
    with pytest.raises(ValueError, match="use_clearance needs a contact"):
        g.reset_robots_sampled(mask)
    assert all(np.array_equal(a, b) for a, b in zip(before, g.get_state()))


def test_zero_widths_keep_the_start_pose_bit_for_bit():
    B = 64
    g, cfg, rows = _panda(B, dict(seed=3, goal_tasks=(0, 1)))
    twin, _, _ = _panda(B, dict(seed=3, goal_tasks=()))
    mask = _mask(B, 6)
    for c in (g, twin):
        c.reset_robots_sampled(mask)
    _equal_columns(_everything(g, ["mft", "jt"]), _everything(twin, ["mft", "jt"]), np.ones(B, dtype=bool), "goals at the start pose")
    pos, rot = g.get_mft_goals(0)[:2]
    des = g.get_mft_desired(0)
    assert np.array_equal(pos[:, mask], des[0][:, mask]) and np.array_equal(rot[:, mask], des[1][:, mask])


# ------------------------------------------------------------------------------- twin: reset_robots + the goal setters
@pytest.mark.parametrize("name", ["c3", "c4", "generic", "jerk", "n4", "n8"])
def test_twin_reset_robots_and_goal_setters(name, monkeypatch):
    s = sr.scenario(name)
    B = sr.B
    a, r0, r1 = sr.contexts(s, 3, monkeypatch)
    goals = {}
    for t, k in enumerate(s.kinds):
        goals[t] = dict(pos_lower=-0.03, pos_upper=0.04, theta_max=0.0 if s.n == 4 else 0.2) if k == "mft" else dict(half_width=0.1)
        if k == "mft" and s.n == 4:
            goals[t]["pos_lower"], goals[t]["pos_upper"] = (-0.03, -0.03, 0.0), (0.04, 0.04, 0.0)
    cfg = a.reset_sampler_config(seed=99, goal_tasks=tuple(range(len(s.kinds))))
    lo, hi = np.array(a.model.q_lower[: s.n]), np.array(a.model.q_upper[: s.n])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    a.set_reset_sampler(cfg, a.reset_sampler_rows(cfg, q_lower=mid - 0.5 * half, q_upper=mid + 0.5 * half, dq_sigma=0.1, goals=goals))
    mask = sr.MASK_A
    a.reset_robots_sampled(mask)
    q, dq = a.get_state()
    r1.reset_robots(mask, sr.with_garbage(q, mask), sr.with_garbage(dq, mask))
    for t, k in enumerate(s.kinds):
        if k == "mft":
            pos, rot = a.get_mft_goals(t)[:2]
            cur = r1.get_mft_goals(t)[:2]
            r1.set_mft_goals(t, np.where(mask, pos, cur[0]), np.where(mask, rot, cur[1]), None, None, None, None)
        else:
            r1.set_jt_goals(t, np.where(mask, a.get_jt_goals(t)[0], r1.get_jt_goals(t)[0]), None, None)
    snaps = [_everything(c, s.kinds) for c in (a, r0, r1)]
    _equal_columns(snaps[0], snaps[2], np.ones(B, dtype=bool), "twin, snapshot")
    _equal_columns(snaps[0], snaps[1], ~mask, "unselected, snapshot")
    after = [sr.flat(sr.run(c, 5)) for c in (a, r0, r1)]
    _equal_columns(after[0], after[2], np.ones(B, dtype=bool), "twin, periods after")
    _equal_columns(after[0], after[1], ~mask, "unselected, periods after")
    assert not np.array_equal(snaps[0][0][:, mask], snaps[1][0][:, mask])


def _bank_blocks(g):
    """every block of every robot's state as a snapshot bank holds it (q .. the passivity observer's popc_f / popc_i / popc_q):
    dict (block name, task) -> [rows][B] uint64 or uint32 (a block's rows stand one after the other, each B elements long)"""
    B = g.B
    bank = g.snapshot_bank(B)
    bank.save()
    blob = np.asarray(bank.export())
    bank.close()
    body = blob[_abi.SNAPSHOT_HEADER_BYTES : _abi.SNAPSHOT_HEADER_BYTES + 4 * g.snapshot_words() * B].tobytes()
    out = {}
    for r in g.snapshot_layout():
        part = body[4 * B * r["first_word"] : 4 * B * r["first_word"] + r["rows"] * r["elem_bytes"] * B]
        out[(r["block"], r["task"])] = np.frombuffer(part, dtype=np.uint64 if r["elem_bytes"] == 8 else np.uint32).reshape(r["rows"], B)
    return out


def test_twin_with_a_passivity_observer():
    """[MotionForceTask with a closed-loop force space and the passivity observer, JointTask] (the hierarchy of
    tests/test_gpu_subset_reset.py::test_passivity_observer): the sampled reset against reset_robots + the goal setters on a twin,
    bit-equal in every block a snapshot bank holds, the observer's popc_f / popc_i / popc_q among them, and over 5 further periods"""
    B = sr.B
    rng = np.random.default_rng(5)
    inp = pkg.workloads.make_inputs(3, B=B, seed=78)
    sensed = rng.normal(0, 3.0, (125, 3, B))
    wrench = np.tile(np.array(plumbing.FORCE_AXIS)[:, None] * 5.0, (1, B))

    def make():
        cfgs = [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")]
        c = cfgs[0]
        c.force_space_dimension, c.closed_loop_force, c.passivity_enabled = 1, 1, 1
        for i in range(3):
            c.force_axis[i], c.ki_force[i] = plumbing.FORCE_AXIS[i], 1.3
        g = pkg.Controller(pkg.panda_model(), cfgs, B)
        g.set_state(inp["q"], inp["dq"])
        g.reinitialize()
        g.set_mft_goal_wrench(0, wrench, None)
        cfg = g.reset_sampler_config(seed=31, goal_tasks=(0, 1))
        g.set_reset_sampler(cfg, g.reset_sampler_rows(cfg, dq_sigma=0.05, goals={0: dict(pos_lower=-0.02, pos_upper=0.03, theta_max=0.1),
                                                                                  1: dict(half_width=0.05)}))
        return g

    def go(g, k0, k1):
        out = []
        for k in range(k0, k1):
            g.set_mft_sensed_wrench(0, sensed[k], None)
            out.append(sr.period(g))
        return np.array(out)

    a, r0, r1 = (make() for _ in range(3))
    for g in (a, r0, r1):
        go(g, 0, 120)
    mask = sr.MASK_A
    a.reset_robots_sampled(mask)
    q, dq = a.get_state()
    r1.reset_robots(mask, sr.with_garbage(q, mask), sr.with_garbage(dq, mask))
    pos, rot = a.get_mft_goals(0)[:2]
    cur = r1.get_mft_goals(0)[:2]
    r1.set_mft_goals(0, np.where(mask, pos, cur[0]), np.where(mask, rot, cur[1]), None, None, None, None)
    r1.set_jt_goals(1, np.where(mask, a.get_jt_goals(1)[0], r1.get_jt_goals(1)[0]), None, None)
    ba, b0, b1 = (_bank_blocks(g) for g in (a, r0, r1))
    popc = [("popc_f", 0), ("popc_i", 0), ("popc_q", 0)]
    assert set(popc) <= set(ba) and ("reset_sampler_episode", -1) in ba and set(ba) == set(b0) == set(b1)

    def differing(x, y, cols):
        return sorted(k for k in x if k[0] != "reset_sampler_episode" and not np.array_equal(x[k][:, cols], y[k][:, cols]))

    # (the twin never made the sampled call: its episode counter stays 0, the one block left out)
    assert differing(ba, b1, np.ones(B, dtype=bool)) == [] and differing(ba, b0, ~mask) == []
    # the observers had state and the reset replaced it: value and counters; the ring's old samples stay where they are, unread
    # (ring head and size are zero again), as reset_robots leaves them
    assert set(popc[:2]) <= set(differing(ba, b0, mask)) and b0[("popc_i", 0)][2].any() and not ba[("popc_i", 0)][1:, mask].any()
    assert np.array_equal(ba[("reset_sampler_episode", -1)][0], mask.astype(np.uint32))
    ta, t0, t1 = (go(g, 120, 125) for g in (a, r0, r1))
    assert np.array_equal(ta, t1) and np.array_equal(ta[..., ~mask], t0[..., ~mask]) and not np.array_equal(ta[..., mask], t0[..., mask])
    _equal_columns(_everything(a, ["mft", "jt"]), _everything(r1, ["mft", "jt"]), np.ones(B, dtype=bool), "after 5 periods")
    ba, b1 = (_bank_blocks(g) for g in (a, r1))
    assert differing(ba, b1, np.ones(B, dtype=bool)) == []  # the observers too, 5 periods on


# ------------------------------------------------------------------------------- reproducibility
def test_shards_seed_snapshot_clone_and_export():
    B = 4099
    cfg_kw = dict(PANDA_CFG, max_tries=4)
    g, cfg, rows = _panda(B, cfg_kw, PANDA_ROWS)
    mask = _mask(B, 7)
    g.reset_robots_sampled(mask)
    one = _everything(g, ["mft", "jt"])
    tries = g.reset_sampler_state()["tries"]
    # two shards with first_robot set
    for rank in range(2):
        lo, hi = sharding.shard_bounds(B, 2, rank)
        s = pkg.Controller(pkg.panda_model(), [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], hi - lo)
        sharding.set_reset_sampler(s, 2, rank, B, rows=rows, **cfg_kw)
        assert s.get_reset_sampler()[0].first_robot == lo
        sharding.reset_robots_sampled(s, 2, rank, mask)
        part = _everything(s, ["mft", "jt"])
        m = mask[lo:hi]
        for x, y in zip(part, one):
            assert np.array_equal(x[..., m], y[..., lo:hi][..., m])
        assert np.array_equal(s.reset_sampler_state()["tries"][m], tries[lo:hi][m])
        s.close()
    # the same seed twice; save, reset, load, reset again
    h, _, _ = _panda(B, cfg_kw, PANDA_ROWS)
    bank = h.snapshot_bank(B)
    bank.save()
    h.reset_robots_sampled(mask)
    first = _everything(h, ["mft", "jt"])
    _equal_columns(first, one, mask, "same seed")
    h.reset_robots_sampled(mask)
    second = _everything(h, ["mft", "jt"])
    assert not np.array_equal(first[0][:, mask], second[0][:, mask]) and (h.reset_sampler_state()["episode"][mask] == 2).all()
    bank.load()
    assert not h.reset_sampler_state()["episode"].any()
    h.reset_robots_sampled(mask)
    _equal_columns(_everything(h, ["mft", "jt"]), first, mask, "after load")
    # export into a fresh context and import there: the sequence continues (episode 1 -> the second draw)
    bank.save()
    f, _, _ = _panda(B, cfg_kw, PANDA_ROWS)
    fb = f.snapshot_bank(B)
    fb.import_(bank.export())
    fb.load()
    assert np.array_equal(f.reset_sampler_state()["episode"], h.reset_sampler_state()["episode"])
    f.reset_robots_sampled(mask)
    _equal_columns(_everything(f, ["mft", "jt"]), second, mask, "imported")
    # one slot cloned into every robot: different draws per robot
    fb.load(slots=np.zeros(B, dtype=np.int32))
    f.reset_robots_sampled(np.ones(B, dtype=bool))
    q, accepted = f.get_state()[0], f.reset_sampler_state()["tries"] <= cfg_kw["max_tries"]
    assert accepted.sum() > 0.85 * B and len(np.unique(q[0, accepted])) == accepted.sum()  # (an exhausted robot gets q_nominal)
    for b_ in (bank, fb):
        b_.close()


# ------------------------------------------------------------------------------- hardware clocks, reward accumulators
def test_hardware_and_reward_follow():
    B = 200
    g, cfg, rows = _panda(B, dict(seed=5, goal_tasks=(0,)), dict(goals={0: dict(pos_lower=-0.05, pos_upper=0.05)}))
    g.set_hardware(max_delay=2, seed=1)
    g.set_observation(blocks=("q",), max_episode_steps=1000)
    g.set_reward(terms={"alive": 1.0})
    for _ in range(3):
        g.tick(want_output=False)
        g.sim_step(None)
        g.observe_reward()
    mask = _mask(B, 8)
    hw0, st0 = g.get_hardware_state(), g.episode_stats()
    g.reset_robots_sampled(mask)
    hw1, st1 = g.get_hardware_state(), g.episode_stats()
    assert (hw1["period"][mask] == 0).all() and np.array_equal(hw1["period"][~mask], hw0["period"][~mask]) and (hw0["period"] == 3).all()
    assert np.array_equal(hw1["episode"], hw0["episode"] + mask)
    assert np.array_equal(st1["ret"][~mask], st0["ret"][~mask]) and not st1["ret"][mask].any() and (st0["ret"] == 3.0).all()
    # exactly what sai2b_reset_robots does to the accumulators (the same follow-up launch): a new return, "last" as it was
    assert (st1["discount"] == 1.0).all() and np.array_equal(st1["last_return"], st0["last_return"])
    assert np.array_equal(st1["last_length"], st0["last_length"])


# ------------------------------------------------------------------------------- the resident loop
def test_resident_loop_device_mask_equals_numpy_mask():
    import torch

    B = 200
    runs = []
    for device in (True, False):
        g, cfg, rows = _panda(B, dict(PANDA_CFG, max_tries=16), PANDA_ROWS)
        g.set_observation(blocks=("q",), max_episode_steps=5, max_joint_speed=0.9)  # (the speed limit spreads the ends over the periods)
        g.reset_robots_sampled(np.ones(B, dtype=bool))
        done = torch.zeros(B, dtype=torch.uint8, device="cuda") if device else None
        out = torch.zeros((g.observation_rows(), B), dtype=torch.float64, device="cuda") if device else None
        starts = []
        for _ in range(20):
            g.tick(want_output=False)
            g.sim_step(None)
            if device:
                g.observe(out, done)
                g.reset_robots_sampled(done)
                d = done.cpu().numpy() != 0
            else:
                _, d8 = g.observe()
                g.reset_robots_sampled(d8)
                d = d8 != 0
            starts.append((d, g.get_state()[0], g.reset_sampler_state()["tries"]))
        runs.append((starts, _everything(g, ["mft", "jt"])))
    for (da, qa, ta), (db, qb, tb) in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(da, db) and np.array_equal(qa, qb) and np.array_equal(ta, tb)
    _equal_columns(runs[0][1], runs[1][1], np.ones(B, dtype=bool), "device against numpy")
    kin = rr.panda_kinematics(0)
    seen = 0
    for d, q, t in runs[0][0]:
        ok = d & (t <= 16)
        if ok.any():
            r = rr.ratio(kin(q)["J"][0])[ok]
            assert (np.abs(r - 0.06) > 1e-9 * 0.06).all()  # no start state is borderline, so the threshold itself is what holds
            assert (r >= 0.06).all()
            seen += int(ok.sum())
    assert seen > B and len({int(d.sum()) for d, _, _ in runs[0][0]}) > 3  # masks of several sizes, none of them the whole batch only


# ------------------------------------------------------------------------------- argument checks
def test_argument_checks():
    B = 5
    g = pkg.Controller(pkg.panda_model(), [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    ones = np.ones(B, dtype=bool)
    with pytest.raises(ValueError, match="no reset sampler is configured"):
        g.reset_robots_sampled(ones)
    with pytest.raises(ValueError, match="no reset sampler is configured"):
        g.reset_sampler_counts()
    with pytest.raises(ValueError, match="use_clearance needs a contact"):
        g.set_reset_sampler(clearance=0.01)
    g.set_reset_sampler(seed=1)
    before = g.get_state()
    assert g.lib.sai2b_reset_robots_sampled(g.h, None, 0) == _abi.INVALID_ARGUMENT and b"mask is NULL" in g.lib.sai2b_last_error(g.h)
    cfg = g.reset_sampler_config(seed=1)
    rows = g.reset_sampler_rows(cfg)
    for edit, msg in ((lambda r: r.__setitem__((0, 1), np.nan), "finite"), (lambda r: r.__setitem__((0, 2), 9.0), "q_lower must not exceed"),
                      (lambda r: r.__setitem__((14, 0), -1.0), "dq_sigma"), (lambda r: r.__setitem__((21, 3), 50.0), "q_nominal")):
        bad = rows.copy()
        edit(bad)
        with pytest.raises(ValueError, match=msg):
            g.set_reset_sampler(cfg, bad)
    # the goal rows: a MotionForceTask's theta_max (row 6 of its seven) and a JointTask's half widths
    gcfg = g.reset_sampler_config(seed=2, goal_tasks=(0, 1))
    grows = g.reset_sampler_rows(gcfg, goals={0: dict(theta_max=np.pi), 1: dict(half_width=0.0)})
    lay = g.reset_sampler_layout(gcfg)
    assert lay["goal0"] == (28, 7) and lay["goal1"] == (35, 7) and lay["total"] == 42
    for row, col, value, msg in ((34, 4, np.nextafter(np.pi, 4.0), "theta_max must be in"), (34, 0, -1e-300, "theta_max must be in"),
                                 (35, 2, -1e-300, "half_width must not be negative"), (41, 4, -0.5, "half_width must not be negative"),
                                 (33, 1, np.inf, "finite")):
        bad = grows.copy()
        bad[row, col] = value
        with pytest.raises(ValueError, match=msg):
            g.set_reset_sampler(gcfg, bad)
    for row in (28, 33):  # a position box may have any sign and order: neither row is checked beyond being finite
        ok = grows.copy()
        ok[row] = -3.0
        g.set_reset_sampler(gcfg, ok)
    g.set_reset_sampler(cfg, rows)
    with pytest.raises(ValueError, match="a mask of one entry per robot"):
        g.reset_robots_sampled(None)
    assert g.get_reset_sampler()[0].seed == 1 and np.array_equal(g.get_reset_sampler()[1], rows)  # the context is as it was
    assert all(np.array_equal(a, b) for a, b in zip(before, g.get_state())) and tuple(g.reset_sampler_counts().values()) == (0, 0, 0)
    g.reset_robots_sampled(ones)
    assert g.reset_sampler_counts()["reset"] == B
    g.clear_reset_sampler()
    with pytest.raises(ValueError, match="no reset sampler is configured"):
        g.reset_robots_sampled(ones)
