"""GPU tests (-m gpu) of the masked re-initialisation and the episode reset (sai2b_reinitialize_robots, sai2b_reset_robots:
csrc/sai2b_otg.hip reset_subset_kernel), through pkg.Controller.

What a selected robot must end as is defined by the whole-batch calls (set_state + reinitialize, task_reinitialize), and
what an unselected one must end as by a context that never made the call, so every comparison between contexts is
np.array_equal: nothing here has a tolerance except the comparison with the CPU oracle (the project's 1e-10, relative to
max(1, the robot's largest torque)).

Batch 130 = two full wavefronts and a 2-lane tail. MASK_A selects lanes 0 and 63 of wavefront 0, nothing of wavefront 1
(the wavefront that leaves after its mask load) and robot 129, the last lane of the tail; MASK_B selects all of wavefront
1 and nothing else. Eight robots (0, 5, 63, 64, 70, 100, 128, 129: some selected by either mask, some not, 6 % of the
batch so that no batch-wide kernel switch can engage) sit inside a blending region of the 6-row task, so their
singularity histories are not empty. The Panda ones are placed here (elbow stretched, s_5 / s_0 about 0.03:
tests/singular_poses.py covers the robots of tests/robots.py, not the Panda); the 8-joint robot's come from
singular_poses.

History: reinitialize at the start poses, new goals for every task (every generator mid-trajectory), integral gains on
(every integrator non-zero), then 30 periods of tick -> sim_step(None)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import plumbing
import robots
import sai2_primitives_perso_amd as pkg
import singular_poses as sp
from sai2_primitives_perso_amd import _abi
from sai2_primitives_perso_amd import workloads as wl

pytestmark = pytest.mark.gpu

B = 130
HISTORY, AFTER = 30, 10
SINGULAR = np.array([0, 5, 63, 64, 70, 100, 128, 129])
MASK_A = np.zeros(B, dtype=bool)
MASK_A[[0, 63, 129]] = True
MASK_B = np.zeros(B, dtype=bool)
MASK_B[64:128] = True
MASKS = {"A": MASK_A, "B": MASK_B}


def _panda_blending(q_regular):
    """the pose with the elbow stretched (q4 next to its upper limit, plumbing.ELBOW_STRETCHED): s_5 / s_0 of the 6-row task is
    about 0.03 there, inside the blending band (s_min = 0.006, s_max = 0.06) by a factor of 1.5 at least on either side"""
    q = q_regular.copy()
    q[3] = plumbing.ELBOW_STRETCHED
    s = np.linalg.svd(wl.frame_jacobian(*wl.fk(q[None]))[0][0], compute_uv=False)
    assert 0.012 < s[5] / s[0] < 0.04, s[5] / s[0]
    return q


class Scenario:
    """model, task configs (fresh ones per context, oracle's or product's), start state, the goals of period 0, the state a
    reset puts robots into"""

    def __init__(self, name):
        self.name, self.env = name, {}
        rng = np.random.default_rng([20250117, len(name), ord(name[0])])
        otg = True
        if name in ("c3", "regular", "jerk", "generic", "c4", "idle_otg"):
            self.model, self.omodel, n = pkg.panda_model, ol.panda_model, 7
            inp = wl.make_inputs(4 if name == "c4" else 3, B=B, seed=77)
            q = inp["q"]
            if name == "c4":
                part, sel = inp["tasks"][0][1]["partial"], inp["tasks"][1][1]["selection"]
                q = wl.make_inputs(3, B=B, seed=77)["q"]  # (regular poses: config 4's own singular tenth is not what this is about)
                self.mk = lambda M, J: [M("m", partial=part, internal_otg=True), J("j2", sel, internal_otg=True), J("j7", internal_otg=True)]
                self.kinds = ["mft", "jt", "jt"]
            else:
                otg = name != "idle_otg"
                self.mk = lambda M, J: [M("m", internal_otg=otg), J("j", internal_otg=otg)]
                self.kinds = ["mft", "jt"]
                if name not in ("regular", "idle_otg"):
                    for b in SINGULAR:
                        q[:, b] = _panda_blending(q[:, b])
            if name == "generic":
                self.env = {"SAI2B_NO_FAST_PATH": "1"}
        else:
            robot = {"n4": "planar_4r", "n8": "sliding_base"}[name]
            text = robots.TEXT[robot]()
            self.model = self.omodel = lambda: pkg.model_from_urdf(text, is_file=False)[0]
            m, links = pkg.model_from_urdf(text, is_file=False)
            n = m.dof
            lo, hi = np.array(list(m.q_lower)[:n]), np.array(list(m.q_upper)[:n])
            q = (0.5 * (lo + hi))[:, None] + 0.6 * (0.5 * (hi - lo))[:, None] * rng.uniform(-1, 1, (n, B))
            if robot == "planar_4r":
                link, fpos, frot = pkg.resolve_link_frame(links, "link4", (0.5, 0.0, 0.0))
                part = (np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[0, 0, 1.0]]))
                self.mk = lambda M, J: [M("m", link, fpos, frot, part, internal_otg=True, robot_dof=n), J("j", None, internal_otg=True, robot_dof=n)]
                self.kinds = ["mft", "jt"]
            else:
                link, fpos, frot = pkg.resolve_link_frame(links, "end-effector", (0.0, 0.0, 0.07))
                sel = np.zeros((2, n))
                sel[0, 0] = sel[1, 7] = 1
                self.mk = lambda M, J: [J("p", sel, internal_otg=True, robot_dof=n), M("m", link, fpos, frot, internal_otg=True, robot_dof=n),
                                        J("j", None, internal_otg=True, robot_dof=n)]
                self.kinds = ["jt", "mft", "jt"]
                q[:, SINGULAR[:4]] = sp.poses("sliding_base", "blending", 4)
        self.n = n
        self.q0, self.dq0 = np.ascontiguousarray(q), rng.normal(0, 0.2, (n, B))
        # what a reset puts a robot into: the start poses of other robots, other velocities
        self.q1, self.dq1 = np.ascontiguousarray(np.roll(self.q0, 7, axis=1)), rng.normal(0, 0.1, (n, B))
        self.rng_goals = [rng.uniform(-1, 1, (12, B)) for _ in self.kinds]

    def configs(self, oracle=False):
        cfgs = self.mk(ol.motion_force_task, ol.joint_task) if oracle else self.mk(pkg.motion_force_task_config, pkg.joint_task_config)
        for c in cfgs:
            plumbing._gains(c, False)  # integral gains on
        if self.name == "jerk":
            c = cfgs[1]
            c.internal_otg_jerk_limited = 1
            for i in range(c.task_dof):
                c.otg_max_jerk[i] = 20.0 + i
        return cfgs

    def controller(self, monkeypatch=None):
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)  # (read when the context is created)
        try:
            return pkg.Controller(self.model(), self.configs(), B)
        finally:
            for k in self.env:
                monkeypatch.delenv(k)

    def oracle(self):
        return ol.Oracle(self.omodel(), self.configs(oracle=True), B, threads=8)

    def start(self, c):
        """state, tasks re-initialised there, then new goals around the pose"""
        c.set_state(self.q0, self.dq0)
        c.reinitialize()
        for t, k in enumerate(self.kinds):
            r = self.rng_goals[t]
            if k == "mft":
                pos, rot = c.get_mft_desired(t)[:2]
                d = 0.04 * r[:3]
                if self.n == 4:
                    d[2] = 0  # planar
                    ax = np.tile(np.array([0, 0, 1.0]), (B, 1))
                else:
                    ax = r[3:6].T / np.linalg.norm(r[3:6].T, axis=1, keepdims=True)
                R = rot.T.reshape(B, 3, 3) @ wl._expmap(ax * 0.1 * (1 + r[6])[:, None])
                c.set_mft_goals(t, pos + d, np.ascontiguousarray(R.reshape(B, 9).T), None, None, None, None)
            else:
                k0 = c.tasks[t].task_dof
                c.set_jt_goals(t, c.get_jt_desired(t)[0] + 0.1 * r[:k0], None, None)


@functools.lru_cache(maxsize=None)
def scenario(name):
    return Scenario(name)


def period(c):
    tau = c.tick()
    c.sim_step(None if isinstance(c, pkg.Controller) else tau)
    return tau


def run(c, periods):
    """-> tau and the state after it, of every period"""
    out = []
    for _ in range(periods):
        tau = period(c)
        out.append((tau,) + tuple(c.get_state()))
    return out


def snapshot(c, kinds):
    """every getter the comparisons use: goals, desired state, generator status, the tasks' persistent state rows (integrators;
    a MotionForceTask's q_prior, dq_prior and type-2 direction too), singularity history, robot state"""
    out = list(c.get_state())
    for t, k in enumerate(kinds):
        if k == "mft":
            out += list(c.get_mft_goals(t)) + list(c.get_mft_desired(t)) + list(c.get_mft_singularity_state(t))
            out.append(plumbing.device_rows(c, _abi.BUF_STATE, t, 12 + 3 * c.dof))
        else:
            out += list(c.get_jt_goals(t)) + list(c.get_jt_desired(t))
            out.append(plumbing.device_rows(c, _abi.BUF_STATE, t, c.tasks[t].task_dof))
        out += list(c.get_otg_status(t))
    return [np.asarray(a) for a in out]


def assert_columns(got, want, cols, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a[..., cols], b[..., cols]), (what, i, np.flatnonzero((a != b).reshape(-1, B).any(axis=0) & cols)[:8])


def flat(runs):
    return [a for r in runs for a in r]


def mixed(c, s, mask):
    """the context's current state with the selected columns replaced by the reset state"""
    q, dq = c.get_state()
    q[:, mask], dq[:, mask] = s.q1[:, mask], s.dq1[:, mask]
    return q, dq


def with_garbage(a, mask):
    out = np.full_like(a, np.nan)
    out[:, mask] = a[:, mask]
    return out


def contexts(s, count, monkeypatch):
    cs = [s.controller(monkeypatch) for _ in range(count)]
    for c in cs:
        s.start(c)
        run(c, HISTORY)
    return cs


def test_control_two_contexts_driven_alike_are_bit_equal(monkeypatch):
    """what every later comparison rests on"""
    s = scenario("c3")
    a, b = (s.controller(monkeypatch) for _ in range(2))
    ra, rb = [], []
    for c, r in ((a, ra), (b, rb)):
        s.start(c)
        r += run(c, HISTORY)
    every = np.ones(B, dtype=bool)
    assert_columns(flat(ra), flat(rb), every, "history")
    assert_columns(snapshot(a, s.kinds), snapshot(b, s.kinds), every, "snapshot")
    n_sing = a.get_mft_singularity_state(0)[0]
    assert (n_sing[SINGULAR] > 0).all() and (np.delete(n_sing, SINGULAR) == 0).all()  # the blending robots are where they were put
    integ = plumbing.device_rows(a, _abi.BUF_STATE, 0, 12)[:6]
    assert (np.abs(integ).max(axis=0) > 0).all() and not a.get_otg_status(0)[0].all()  # integrators moved, generators under way


@pytest.mark.parametrize("call", ["reset", "task0", "task1", "all_tasks"])
def test_full_mask_equals_the_whole_batch_call(call, monkeypatch):
    s = scenario("c3")
    a, r = contexts(s, 2, monkeypatch)
    ones = np.ones(B, dtype=np.uint8)
    if call == "reset":
        a.reset_robots(ones, s.q1, s.dq1)
        r.set_state(s.q1, s.dq1)
        r.reinitialize()
    elif call == "all_tasks":
        a.reinitialize_robots(ones)
        r.reinitialize()
    else:
        a.reinitialize_robots(ones, task=int(call[-1]))
        r.task_reinitialize(int(call[-1]))
    every = ones.astype(bool)
    assert_columns(snapshot(a, s.kinds), snapshot(r, s.kinds), every, "snapshot")
    assert_columns(flat(run(a, AFTER)), flat(run(r, AFTER)), every, "periods after")


def subset_case(name, mask, monkeypatch, on_device=False):
    s = scenario(name)
    r0, r1, a = contexts(s, 3, monkeypatch)
    r1.set_state(*mixed(r1, s, mask))
    r1.reinitialize()
    q_new, dq_new, m = with_garbage(s.q1, mask), with_garbage(s.dq1, mask), mask
    if on_device:
        import torch

        q_new, dq_new, m = (torch.from_numpy(x).cuda() for x in (q_new, dq_new, mask))
    a.reset_robots(m, q_new, dq_new)
    tau = plumbing.device_rows(a, _abi.BUF_TAU, -1, s.n)
    assert not tau[:, mask].any() and np.array_equal(tau[:, ~mask], plumbing.device_rows(r0, _abi.BUF_TAU, -1, s.n)[:, ~mask])
    snaps = [snapshot(c, s.kinds) for c in (a, r0, r1)]
    assert_columns(snaps[0], snaps[2], mask, "selected, snapshot")
    assert_columns(snaps[0], snaps[1], ~mask, "unselected, snapshot")
    after = [flat(run(c, AFTER)) for c in (a, r0, r1)]
    assert_columns(after[0], after[2], mask, "selected, periods after")
    assert_columns(after[0], after[1], ~mask, "unselected, periods after")
    # the reset did something, and the three runs are not all alike
    assert not np.array_equal(snaps[0][0][:, mask], snaps[1][0][:, mask]) and not np.array_equal(after[1][0][:, ~mask], after[2][0][:, ~mask])


@pytest.mark.parametrize("mask, on_device", [("A", False), ("B", False), ("A", True)], ids=["A-numpy", "B-numpy", "A-torch"])
def test_subset(mask, on_device, monkeypatch):
    subset_case("c3", MASKS[mask], monkeypatch, on_device)


@pytest.mark.parametrize("name", ["c4", "n4", "n8", "jerk", "generic"])
def test_subset_other_routes(name, monkeypatch):
    """config 4's three levels (tick_cert_kernel), the 4- and 8-joint builds, a jerk-limited JointTask generator, the generic
    kernel alone"""
    subset_case(name, MASK_A, monkeypatch)


@pytest.mark.parametrize("task", [-1, 0, 1])
def test_subset_reinitialize_robots(task, monkeypatch):
    """the masked reInitializeTask of every task / one task against the whole-batch call and against no call"""
    s = scenario("c3")
    r0, r1, a = contexts(s, 3, monkeypatch)
    r1.reinitialize() if task < 0 else r1.task_reinitialize(task)
    a.reinitialize_robots(MASK_A.astype(np.uint8), task=task)
    snaps = [snapshot(c, s.kinds) for c in (a, r0, r1)]
    assert_columns(snaps[0], snaps[2], MASK_A, "selected, snapshot")
    assert_columns(snaps[0], snaps[1], ~MASK_A, "unselected, snapshot")
    after = [flat(run(c, AFTER)) for c in (a, r0, r1)]
    assert_columns(after[0], after[2], MASK_A, "selected, periods after")
    assert_columns(after[0], after[1], ~MASK_A, "unselected, periods after")


def test_subset_against_the_cpu_oracle(monkeypatch):
    """regular poses only; the oracle twins run the scripts of R0 (no call) and R1 (set_state + reinitialize) on their own
    states"""
    s = scenario("regular")
    a = s.controller(monkeypatch)
    o0, o1 = s.oracle(), s.oracle()
    for c in (a, o0, o1):
        s.start(c)
        run(c, HISTORY)
    o1.set_state(*mixed(o1, s, MASK_A))
    o1.reinitialize()
    a.reset_robots(MASK_A, with_garbage(s.q1, MASK_A), with_garbage(s.dq1, MASK_A))
    worst = 0.0
    for k in range(AFTER):
        tg, t0, t1 = period(a), period(o0), period(o1)
        ref = np.where(MASK_A[None, :], t1, t0)
        err = (np.abs(tg - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)).max()
        print(f"period {k} after the reset: torque error vs the oracle twins {err:.3e}")
        worst = max(worst, err)
    assert worst < 1e-10, worst


def test_passivity_observer(monkeypatch):
    """[MotionForceTask with a closed-loop force space and the passivity observer, JointTask]: reset_robots re-initialises the
    selected robots' observers (what switching passivity off and on does for everybody), reinitialize_robots leaves them"""
    rng = np.random.default_rng(5)
    inp = wl.make_inputs(3, B=B, seed=78)
    sensed = rng.normal(0, 3.0, (180, 3, B))

    def make():
        cfgs = [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")]
        c = cfgs[0]
        c.force_space_dimension, c.closed_loop_force, c.passivity_enabled = 1, 1, 1
        for i in range(3):
            c.force_axis[i], c.ki_force[i] = plumbing.FORCE_AXIS[i], 1.3
        g = pkg.Controller(pkg.panda_model(), cfgs, B)
        g.set_state(inp["q"], inp["dq"])
        g.reinitialize()
        g.set_mft_goal_wrench(0, np.tile(np.array(plumbing.FORCE_AXIS)[:, None] * 5.0, (1, B)), None)
        return g

    def go(g, k0, k1):
        out = []
        for k in range(k0, k1):
            g.set_mft_sensed_wrench(0, sensed[k], None)
            out.append(period(g))
        return out

    q1, dq1 = np.ascontiguousarray(np.roll(inp["q"], 3, axis=1)), rng.normal(0, 0.1, (7, B))
    untouched, fresh, plain, a, b = (make() for _ in range(5))
    for g in (untouched, fresh, plain, a, b):
        go(g, 0, 120)
    assert not np.array_equal(plumbing.device_rows(a, _abi.BUF_STATE, 0, 12)[6:9], np.zeros((3, B)))
    # twins: observer re-initialised for everybody (fresh) / left alone (plain) behind set_state + reinitialize
    for g, q, dq in ((fresh, q1, dq1), (plain, None, None)):
        if q is not None:
            cur_q, cur_dq = g.get_state()
            cur_q[:, MASK_A], cur_dq[:, MASK_A] = q[:, MASK_A], dq[:, MASK_A]
            g.set_state(cur_q, cur_dq)
        g.reinitialize()
    cfg = fresh.tasks[0]
    for on in (0, 1):
        cfg.passivity_enabled = on
        fresh.update_task_config(0, cfg)
    a.reset_robots(MASK_A, with_garbage(q1, MASK_A), with_garbage(dq1, MASK_A))
    b.reinitialize_robots(MASK_A)
    tu, tf, tp, ta, tb = (np.array(go(g, 120, 180)) for g in (untouched, fresh, plain, a, b))
    assert np.array_equal(ta[..., MASK_A], tf[..., MASK_A]) and np.array_equal(ta[..., ~MASK_A], tu[..., ~MASK_A])
    assert np.array_equal(tb[..., MASK_A], tp[..., MASK_A]) and np.array_equal(tb[..., ~MASK_A], tu[..., ~MASK_A])
    # the observer matters in this run: the twin that keeps it differs from the one that re-initialises it
    assert not np.array_equal(tb[..., MASK_A], ta[..., MASK_A])


def test_cached_pose_follows_a_reset_robot(monkeypatch):
    """after a tick and a simulation step the tasks' cached pose is no longer the state; a generator enabled later starts
    at the pose of a reset robot's new state and at the cached pose of every other robot"""
    s = scenario("idle_otg")
    r0, r1, a = (s.controller(monkeypatch) for _ in range(3))
    for c in (r0, r1, a):
        s.start(c)
        run(c, 3)
    r1.set_state(*mixed(r1, s, MASK_A))
    r1.reinitialize()
    a.reset_robots(MASK_A, with_garbage(s.q1, MASK_A), with_garbage(s.dq1, MASK_A))
    for c in (r0, r1, a):
        for t in range(2):
            cfg = c.tasks[t]
            cfg.use_internal_otg = 1
            c.update_task_config(t, cfg)
    snaps = [snapshot(c, s.kinds) for c in (a, r0, r1)]
    assert_columns(snaps[0], snaps[2], MASK_A, "selected, generators enabled")
    assert_columns(snaps[0], snaps[1], ~MASK_A, "unselected, generators enabled")
    # (the cached pose is not the state: in the untouched context the joint generator starts away from the current q)
    assert not np.array_equal(r0.get_jt_desired(1)[0], r0.get_state()[0])
    after = [flat(run(c, AFTER)) for c in (a, r0, r1)]
    assert_columns(after[0], after[2], MASK_A, "selected, periods after")
    assert_columns(after[0], after[1], ~MASK_A, "unselected, periods after")


def test_contact_and_payloads_survive_a_reset(monkeypatch):
    s = scenario("c3")
    rng = np.random.default_rng(9)
    mass, com = rng.uniform(0.2, 1.5, B), rng.normal(0, 0.03, (3, B))
    pos = wl.frame_jacobian(*wl.fk(s.q0.T))[1].T  # [3][B] control points: a floor through each
    point = pos + np.array([[0], [0], [0.001]])  # (1 mm deep at the start)
    stiffness = rng.uniform(500, 2000, B)
    normal = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, B))
    r0, a = (s.controller(monkeypatch) for _ in range(2))
    for c in (r0, a):
        c.set_link_payload(6, mass, com, None, target="both")
        c.set_contact(6, [wl.EE_FRAME_POS], point, normal, stiffness, np.full(B, 0.01), np.full(B, 0.2), sensor_task=0)
        s.start(c)
        run(c, HISTORY)
    before = (a.get_contact()[1], a.get_link_payload("controller")[1:], a.get_link_payload("plant")[1:])
    a.reset_robots(MASK_A, with_garbage(s.q1, MASK_A), with_garbage(s.dq1, MASK_A))
    after = (a.get_contact()[1], a.get_link_payload("controller")[1:], a.get_link_payload("plant")[1:])
    assert np.array_equal(before[0], after[0]) and a.get_contact()[0].n_points == 1
    for x, y in zip(before[1] + before[2], after[1] + after[2]):
        assert np.array_equal(x, y)
    assert np.array_equal(before[1][0], mass)
    assert_columns(flat(run(a, AFTER)), flat(run(r0, AFTER)), ~MASK_A, "unselected, periods after")


def test_errors():
    g = pkg.Controller(pkg.panda_model(), [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")], B)
    ok = np.ones(B, dtype=np.uint8)
    ptr = C.c_void_p(ok.ctypes.data)
    for rc in (g.lib.sai2b_reinitialize_robots(g.h, -1, None, 0), g.lib.sai2b_reset_robots(g.h, None, None, None, 0),
               g.lib.sai2b_reinitialize_robots(g.h, 2, ptr, 0), g.lib.sai2b_reinitialize_robots(g.h, -2, ptr, 0),
               g.lib.sai2b_reinitialize_robots(None, 0, ptr, 0), g.lib.sai2b_reset_robots(None, ptr, None, None, 0)):
        assert rc == _abi.INVALID_ARGUMENT
    assert g.lib.sai2b_reinitialize_robots(g.h, 2, ptr, 0) == _abi.INVALID_ARGUMENT and b"task" in g.lib.sai2b_last_error(g.h)
    assert g.lib.sai2b_reset_robots(g.h, None, None, None, 0) == _abi.INVALID_ARGUMENT and b"mask" in g.lib.sai2b_last_error(g.h)
    with pytest.raises(ValueError, match="task"):
        g.reinitialize_robots(ok, task=2)
    for bad in (np.ones(B - 1, dtype=np.uint8), np.ones(B, dtype=np.float64), np.ones((1, B), dtype=bool), None):
        with pytest.raises(ValueError):
            g.reset_robots(bad)
        with pytest.raises(ValueError):
            g.reinitialize_robots(bad)
    with pytest.raises(ValueError):
        g.reset_robots(ok, np.zeros((7, B - 1)))
    import torch

    with pytest.raises(ValueError):
        g.reset_robots(torch.ones(B, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):  # host rows with a device mask
        g.reset_robots(torch.ones(B, dtype=torch.bool, device="cuda"), np.zeros((7, B)))
    g.reset_robots(ok)  # and a valid call goes through: NULL rows keep the state
    g.reset_robots(torch.ones(B, dtype=torch.bool, device="cuda"))
    g.synchronize()
