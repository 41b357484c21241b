"""sai2b_apply_action on the GPU (-m gpu): one launch that maps an action [rows][B] to the goal rows of the chosen tasks
(include/sai2b.h "actions").

Goal rows are held to the numpy evaluation tests/action_reference.py at the bound tests/test_gpu_parity.py::
test_task_observers_between_ticks holds the same kinematic quantities to, |d| < 1e-12 max(1, |x|max); rows that are copies
or single products (an absolute position without a clamp, force / moment, untouched rows) must be equal bit for bit. The pose
and S q the reference starts from are the CPU oracle's. Every limit of the clamp tests sits in a gap of the reference's
unclamped values (asserted: no value within 1e-9 relative of it), so rounding cannot move a robot across it.

Measured on an MI355X (test_every_mode_and_block_combination prints it): the worst |d| over the 45 configurations of every
robot and batch is at most 0.001 of the bound."""
import ctypes as C
import itertools

import numpy as np
import pytest

import action_reference as ar
import oracle_lib as ol
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi
from sai2_primitives_perso_amd import workloads as wl
from test_gpu_observe import Scene, pick_threshold

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "two_mft", "sliding_base", "planar_4r"]
BATCHES = [1, 63, 65, 130, 4099]
MODES = ["delta_goal", "delta_current", "absolute"]
BLOCK_SETS = [c for r in range(1, 5) for c in itertools.combinations(ar.BLOCKS, r)]  # the 15 non-empty selections, in flag order
MFT_SCALES = dict(pos_scale=(0.05, 0.08, 0.03), ori_scale=0.4, force_scale=12.0, moment_scale=1.5)


def _bound(a, ref):
    return np.abs(a - ref).max(), 1e-12 * max(1.0, np.abs(ref).max())


def kinds_of(g):
    return [("jt", t.task_dof) if t.type == _abi.JOINT_TASK else ("mft",) for t in g.tasks]


def read_goals(g):
    """every task's goal rows as the library lays them out: MotionForceTask [30][B], JointTask [3 task_dof][B]"""
    return [np.concatenate(g.get_jt_goals(t) if k[0] == "jt" else g.get_mft_goals(t)) for t, k in enumerate(kinds_of(g))]


def write_goals(g, goals):
    for t, k in enumerate(kinds_of(g)):
        G = np.ascontiguousarray(goals[t])
        if k[0] == "jt":
            g.set_jt_goals(t, *[np.ascontiguousarray(x) for x in np.split(G, 3)])
        else:
            g.set_mft_goals(t, *[np.ascontiguousarray(G[a:b]) for a, b in ((0, 3), (3, 12), (12, 15), (15, 18), (18, 21), (21, 24))])
            g.set_mft_goal_wrench(t, np.ascontiguousarray(G[24:27]), np.ascontiguousarray(G[27:30]))


def selection_times_q(task, n, q):
    k0 = task.task_dof
    S = np.array(list(task.joint_selection)[: k0 * n]).reshape(k0, n)
    return S @ q


class Ground:
    """what the reference needs of a Scene: kinds, the oracle's pose per MotionForceTask, S q per JointTask, and the goals the
    scene's controller started with (restored before every test that uses the scene)"""

    def __init__(self, s):
        self.s, self.g, self.B = s, s.g, s.B
        self.kinds = kinds_of(s.g)
        self.pose = {}
        for t in s.mfts:
            st = s.o.get_mft_status(t)
            self.pose[t] = (st["pos"], st["rot"])
        self.Sq = {t: selection_times_q(s.g.tasks[t], s.n, s.q) for t, k in enumerate(self.kinds) if k[0] == "jt"}
        self.goals0 = read_goals(s.g)

    def restore(self):
        write_goals(self.g, self.goals0)
        assert all(np.array_equal(a, b) for a, b in zip(read_goals(self.g), self.goals0))

    def reference(self, tasks, clip, goals, action, mask=None, state_finite=None):
        return ar.apply_action(self.kinds, tasks, clip, goals, self.pose, self.Sq, action, mask, state_finite)

    def settings(self, mode, blocks, jt_mode=None, skip=()):
        """one mode and block selection for every MotionForceTask, jt_mode (default: the same) for every JointTask"""
        tasks = {}
        for t, k in enumerate(self.kinds):
            if t in skip:
                continue
            if k[0] == "mft":
                tasks[t] = dict(mode=mode, blocks=tuple(blocks), **MFT_SCALES)
            elif (jt_mode or mode) != "none":
                tasks[t] = dict(mode=jt_mode or mode, jt_scale=np.linspace(0.05, 0.12, k[1]))
        return tasks


@pytest.fixture(scope="module")
def grounds():
    cache = {}

    def get(robot, B):
        if (robot, B) not in cache:
            cache[(robot, B)] = Ground(Scene(robot, B))
        gr = cache[(robot, B)]
        gr.restore()
        return gr

    return get


def check_against_reference(gr, tasks, before, after, want, label):
    """after: the controller's goals; want: the reference's. Mapped rows at the bound, everything else bit for bit."""
    lay, _ = ar.layout(gr.kinds, tasks)
    worst = 0.0
    for t, k in enumerate(gr.kinds):
        s = tasks.get(t)
        touched = np.zeros(before[t].shape[0], bool)
        if s:
            if k[0] == "jt":
                touched[: k[1]] = True
                exact = s["mode"] == "absolute" and "jt_upper" not in s
            else:
                for name, rows in (("position", ar.MFT_POS), ("orientation", ar.MFT_ROT), ("force", ar.MFT_FORCE), ("moment", ar.MFT_MOMENT)):
                    if name in s["blocks"]:
                        touched[rows] = True
                exact = False
                for name, rows in (("force", ar.MFT_FORCE), ("moment", ar.MFT_MOMENT)):  # single products
                    if name in s["blocks"]:
                        assert np.array_equal(after[t][rows], want[t][rows]), (label, t, name)
                if "position" in s["blocks"] and s["mode"] == "absolute" and "pos_upper" not in s and "max_pos_lead" not in s:
                    assert np.array_equal(after[t][ar.MFT_POS], want[t][ar.MFT_POS]), (label, t, "absolute position")
            if exact:
                assert np.array_equal(after[t][touched], want[t][touched]), (label, t)
            if touched.any():
                err, bound = _bound(after[t][touched], want[t][touched])
                worst = max(worst, err / bound)
                assert err < bound, (label, t, err, bound)
        # velocity and acceleration rows, and the rows of tasks without a mode: as before
        assert np.array_equal(after[t][~touched], before[t][~touched]), (label, t, "untouched rows")
    return worst


# ---------------------------------------------------------------- 1. every mode x every block combination
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_every_mode_and_block_combination(grounds, robot, B):
    gr = grounds(robot, B)
    g = gr.g
    rng = np.random.default_rng(7)
    worst = 0.0
    for m, mode in enumerate(MODES):
        for i, blocks in enumerate(BLOCK_SETS):
            # JointTasks walk through the modes too (none included); with two MotionForceTasks the second sits out now and then
            jt_mode = (MODES + ["none"])[(i + m) % 4]
            skip = (gr.s.mfts[1],) if len(gr.s.mfts) > 1 and i % 5 == 4 else ()
            tasks = gr.settings(mode, blocks, jt_mode, skip)
            g.set_action(tasks=tasks)
            lay, rows = ar.layout(gr.kinds, tasks)
            assert g.action_rows() == rows and g.action_layout() == lay
            action = rng.uniform(-1.0, 1.0, (rows, B))
            before = read_goals(g)
            g.apply_action(action)
            after = read_goals(g)
            want, flags = gr.reference(tasks, False, before, action)
            worst = max(worst, check_against_reference(gr, tasks, before, after, want, (mode, blocks, jt_mode)))
            assert g.action_counts() == {"rejected": 0, "clipped": 0, "limited": 0}
    print(f"{robot} B={B}: worst |d| / bound over {len(MODES) * len(BLOCK_SETS)} configurations = {worst:.3f}")


# ---------------------------------------------------------------- 2. zero action
@pytest.mark.parametrize("B", [1, 65, 4099])
@pytest.mark.parametrize("robot", ROBOTS)
def test_zero_action_in_delta_goal_changes_nothing(grounds, robot, B):
    gr = grounds(robot, B)
    g = gr.g
    tasks = gr.settings("delta_goal", ar.BLOCKS[:2])
    g.set_action(tasks=tasks, clip_actions=True)
    before = read_goals(g)
    for zero in (0.0, -0.0):
        g.apply_action(np.full((g.action_rows(), B), zero))
        after = read_goals(g)
        for a, b in zip(after, before):
            assert (a == b).all()
    assert g.action_counts() == {"rejected": 0, "clipped": 0, "limited": 0}


# ---------------------------------------------------------------- 3. clip, box, lead, joint clamp
def limits_in_gaps(gr, tasks, goals, action):
    """box, lead and joint limits for `tasks`, each in a gap of the reference's values without that limit"""
    free, _ = gr.reference(tasks, True, goals, action)
    for t, k in enumerate(gr.kinds):
        s = tasks.get(t)
        if not s:
            continue
        if k[0] == "jt":
            n = k[1]
            s["jt_upper"] = np.array([pick_threshold(free[t][i], 1 - 1 / (3 * n))[0] for i in range(n)])
            s["jt_lower"] = np.full(n, -np.inf)
            s["jt_lower"][0] = min(pick_threshold(free[t][0], 0.05)[0], s["jt_upper"][0] - 1.0)
            assert np.abs(free[t][0] - s["jt_lower"][0]).min() > 1e-9 * max(1.0, np.abs(free[t][0]).max())
        else:
            p = free[t][ar.MFT_POS]
            s["pos_upper"] = np.array([pick_threshold(p[0], 0.9)[0], pick_threshold(p[1], 0.9)[0], np.inf])
            s["pos_lower"] = np.array([-np.inf, -np.inf, min(pick_threshold(p[2], 0.1)[0], p[2].max() + 1.0)])
    boxed, _ = gr.reference(tasks, True, goals, action)
    for t in gr.s.mfts:
        if t in tasks:
            dist = np.linalg.norm(boxed[t][ar.MFT_POS] - gr.pose[t][0], axis=0)
            tasks[t]["max_pos_lead"] = pick_threshold(dist, 2 / 3)[0]
    return tasks


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_clip_box_lead_and_joint_clamp(grounds, robot, B):
    gr = grounds(robot, B)
    g = gr.g
    mode = "delta_goal" if B % 2 else "delta_current"
    tasks = gr.settings(mode, ("position", "orientation"))
    _, rows = ar.layout(gr.kinds, tasks)
    rng = np.random.default_rng(11 + B)
    # a third of the robots has components beyond +-1
    action = rng.uniform(-0.98, 0.98, (rows, B)) * np.where(rng.uniform(size=B) < 1 / 3, 1.6, 1.0)
    assert np.abs(np.abs(action) - 1.0).min() > 1e-9
    before = read_goals(g)
    tasks = limits_in_gaps(gr, tasks, before, action)
    g.set_action(tasks=tasks, clip_actions=True)
    g.apply_action(action)
    after = read_goals(g)
    want, flags = gr.reference(tasks, True, before, action)
    check_against_reference(gr, tasks, before, after, want, (robot, B, mode))
    counts = {k: int(v.sum()) for k, v in flags.items()}
    print(f"{robot} B={B} {mode}: {counts}")
    assert g.action_counts() == counts
    # a value the reference put on a limit is on that limit exactly
    for t, k in enumerate(gr.kinds):
        s = tasks.get(t)
        if s and k[0] == "jt":
            hit = want[t][: k[1]] == s["jt_upper"][:, None]
            assert np.array_equal(after[t][: k[1]][hit], want[t][: k[1]][hit])
    if B >= 63:
        assert 0 < counts["clipped"] < B and 0 < counts["limited"] < B and counts["rejected"] == 0
    # without clipping the same action is scaled as it is
    g.set_action(tasks=gr.settings(mode, ("position", "orientation")))
    gr.restore()
    g.apply_action(action)
    want, flags = gr.reference(gr.settings(mode, ("position", "orientation")), False, before, action)
    check_against_reference(gr, gr.settings(mode, ("position", "orientation")), before, read_goals(g), want, "unclipped")
    assert g.action_counts() == {"rejected": 0, "clipped": 0, "limited": 0}


# ---------------------------------------------------------------- 4. non-finite actions
def scatter_nonfinite(action, rng):
    """NaN, +inf, -inf, each in one component of about 5 % of the robots: lane 0, lane 63 and the last robot among them"""
    rows, B = action.shape
    bad = np.unique(np.concatenate([[0, min(63, B - 1), B - 1], rng.choice(B, max(1, B // 20), replace=False)]))
    action = action.copy()
    for n, b in enumerate(bad):
        action[rng.integers(rows), b] = (np.nan, np.inf, -np.inf)[n % 3]
    return action, bad


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("robot", ["panda", "two_mft", "sliding_base"])
def test_nonfinite_actions_are_rejected(grounds, robot, B):
    gr = grounds(robot, B)
    g = gr.g
    rng = np.random.default_rng(13 + B)
    for mode, clip in (("delta_goal", True), ("delta_current", False), ("absolute", True)):
        tasks = gr.settings(mode, ar.BLOCKS)
        g.set_action(tasks=tasks, clip_actions=clip)
        action, bad = scatter_nonfinite(rng.uniform(-1.0, 1.0, (g.action_rows(), B)), rng)
        before = read_goals(g)
        g.apply_action(action)
        after = read_goals(g)
        for t in range(len(gr.kinds)):
            assert np.array_equal(after[t][:, bad], before[t][:, bad]), (mode, t)
        want, flags = gr.reference(tasks, clip, before, action)
        assert np.array_equal(np.flatnonzero(flags["rejected"]), bad)
        check_against_reference(gr, tasks, before, after, want, (robot, B, mode))
        assert g.action_counts() == {"rejected": len(bad), "clipped": 0, "limited": 0}


def test_a_state_that_is_not_finite_is_rejected_where_it_is_read(grounds):
    B = 130
    gr = grounds("two_mft", B)
    g, s = gr.g, gr.s
    q = s.q.copy()
    bad = np.array([0, 63, 64, 129])
    q[2, 0], q[6, 63], q[0, 64], q[3, 129] = np.nan, np.inf, -np.inf, np.nan
    g.set_state(q, None)
    finite = np.ones(B, bool)
    finite[bad] = False
    action = np.random.default_rng(2).uniform(-1, 1, (19, B))  # two MotionForceTasks with two blocks each, seven joints
    try:
        for mode, rejected in (("delta_current", len(bad)), ("delta_goal", 0)):
            tasks = gr.settings(mode, ("position", "orientation"))
            g.set_action(tasks=tasks)
            before = read_goals(g)
            g.apply_action(action)
            after = read_goals(g)
            want, flags = gr.reference(tasks, False, before, action, state_finite=finite)
            if rejected:
                for t in range(3):
                    assert np.array_equal(after[t][:, bad], before[t][:, bad])
            check_against_reference(gr, tasks, before, after, want, mode)
            assert g.action_counts() == {"rejected": rejected, "clipped": 0, "limited": 0} and int(flags["rejected"].sum()) == rejected
    finally:
        g.set_state(s.q, None)


# ---------------------------------------------------------------- 5. mask
@pytest.mark.parametrize("B", [63, 130, 4099])
def test_mask(grounds, B):
    gr = grounds("two_mft", B)
    g = gr.g
    rng = np.random.default_rng(17)
    tasks = gr.settings("delta_goal", ar.BLOCKS)
    action = rng.uniform(-1.5, 1.5, (ar.layout(gr.kinds, tasks)[1], B))
    assert np.abs(np.abs(action) - 1.0).min() > 1e-9
    tasks = limits_in_gaps(gr, tasks, gr.goals0, action)
    action[:, 3] = np.nan  # (the limits sit in gaps of a superset of the values that count)
    g.set_action(tasks=tasks, clip_actions=True)
    g.apply_action(action)
    full, full_counts = read_goals(g), g.action_counts()
    _, flags = gr.reference(tasks, True, gr.goals0, action)
    assert full_counts == {k: int(v.sum()) for k, v in flags.items()} and full_counts["rejected"] == 1
    gr.restore()
    mask = rng.uniform(size=B) < 0.4
    mask[[0, 3, B - 1]] = True
    for m in (mask, mask.astype(np.uint8) * 7):
        gr.restore()
        g.apply_action(action, m)
        part = read_goals(g)
        for t in range(3):
            assert np.array_equal(part[t][:, ~mask], gr.goals0[t][:, ~mask]) and np.array_equal(part[t][:, mask], full[t][:, mask])
        assert g.action_counts() == {k: int((v & mask).sum()) for k, v in flags.items()}
    gr.restore()
    g.apply_action(action, np.zeros(B, bool))
    assert all(np.array_equal(a, b) for a, b in zip(read_goals(g), gr.goals0))
    assert g.action_counts() == {"rejected": 0, "clipped": 0, "limited": 0}
    with pytest.raises(ValueError):
        g.apply_action(action, np.zeros(B + 1, bool))
    with pytest.raises(ValueError):
        g.apply_action(action[:-1])


# ---------------------------------------------------------------- 6. device pointers
@pytest.mark.parametrize("B", [65, 4099])
def test_device_tensors_on_another_stream_equal_the_host_path(grounds, B):
    import torch

    gr = grounds("sliding_base", B)
    g = gr.g
    rng = np.random.default_rng(19)
    tasks = gr.settings("delta_current", ar.BLOCKS)
    g.set_action(tasks=tasks, clip_actions=True)
    rows = g.action_rows()
    action = rng.uniform(-1.3, 1.3, (rows, B))
    mask = rng.uniform(size=B) < 0.7
    g.apply_action(action, mask)
    host, host_counts = read_goals(g), g.action_counts()
    gr.restore()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        # produced on this stream right before the call, and overwritten right after it: the stream contract orders both
        a_d = torch.from_numpy(action).cuda() * 1.0
        m_d = torch.from_numpy(mask).cuda() | False
        g.apply_action(a_d, m_d)
        a_d.fill_(float("nan"))
        m_d.fill_(True)
    dev, dev_counts = read_goals(g), g.action_counts()
    assert all(np.array_equal(a, b) for a, b in zip(dev, host)) and dev_counts == host_counts
    with pytest.raises(ValueError):
        g.apply_action(a_d, mask)  # a device tensor and a host mask
    stream.synchronize()


# ---------------------------------------------------------------- 7. the generators see it
def _otg_twins(kind, jerk, B):
    if kind == "headline":
        inp = wl.make_inputs(3, B=B, seed=31)
    elif kind == "three_level":
        inp = wl.make_inputs(4, B=B, seed=32)
    else:
        inp = wl.make_inputs(3, B=B, seed=33)

    def make():
        cfgs = []
        for t, (k, prm) in enumerate(inp["tasks"]):
            c = (pkg.joint_task_config(f"j{t}", prm.get("selection"), internal_otg=True) if k == "jt" else
                 pkg.motion_force_task_config(f"m{t}", partial=prm.get("partial"), internal_otg=True))
            c.internal_otg_jerk_limited = int(jerk)
            cfgs.append(c)
        if kind == "passivity":
            c = cfgs[0]
            c.force_space_dimension, c.closed_loop_force, c.passivity_enabled = 1, 1, 1
            for i in range(3):
                c.force_axis[i], c.ki_force[i] = (0.0, 0.0, 1.0)[i], 1.3
        g = pkg.Controller(pkg.panda_model(), cfgs, B)
        g.set_state(inp["q"], inp["dq"])
        g.reinitialize()
        return g

    return inp, make(), make()


@pytest.mark.parametrize("jerk", [False, True])
@pytest.mark.parametrize("kind", ["headline", "three_level", "passivity"])
def test_the_generators_see_the_new_goals(kind, jerk):
    B = 130
    inp, a, b = _otg_twins(kind, jerk, B)
    n_tasks = len(inp["tasks"])
    for g in (a, b):  # generators idle at their goals: a tick that finds nothing to do
        g.tick()
    rng = np.random.default_rng(37)
    kinds = kinds_of(a)
    blocks = ("position",) if kind == "three_level" else ("position", "orientation")
    tasks = {t: (dict(mode="absolute", jt_scale=1.0) if k[0] == "jt" else dict(mode="absolute", blocks=blocks)) for t, k in enumerate(kinds)}
    a.set_action(tasks=tasks)
    lay = a.action_layout()
    action = np.zeros((a.action_rows(), B))
    st = a.get_mft_status(0)
    action[lay["position0"]] = st["pos"] + rng.uniform(-0.05, 0.05, (3, B))
    if "orientation0" in lay:
        action[lay["orientation0"]] = rng.uniform(-0.2, 0.2, (3, B))
    q, _ = a.get_state()
    for t, k in enumerate(kinds):
        if k[0] == "jt":
            action[lay[f"joints{t}"]] = selection_times_q(a.tasks[t], 7, q) + rng.normal(0, 0.1, (k[1], B))
    a.apply_action(action)
    goals = read_goals(a)
    for t, k in enumerate(kinds):  # the same rows through the setters
        if k[0] == "jt":
            b.set_jt_goals(t, np.ascontiguousarray(goals[t][: k[1]]), None, None)
        else:
            b.set_mft_goals(t, np.ascontiguousarray(goals[t][0:3]), np.ascontiguousarray(goals[t][3:12]), None, None, None, None)
    assert all(np.array_equal(x, y) for x, y in zip(read_goals(b), goals))
    moved = False
    for k in range(3):
        ta, tb = a.tick(), b.tick()
        assert np.array_equal(ta, tb), (kind, jerk, k)
        for t, kd in enumerate(kinds):
            da, db = (a.get_jt_desired(t), b.get_jt_desired(t)) if kd[0] == "jt" else (a.get_mft_desired(t), b.get_mft_desired(t))
            assert all(np.array_equal(x, y) for x, y in zip(da, db)), (kind, jerk, k, t)
            assert all(np.array_equal(x, y) for x, y in zip(a.get_otg_status(t), b.get_otg_status(t))), (kind, jerk, k, t)
            if kd[0] == "mft":  # the generator left its old goal: it did see the new one
                moved = moved or not np.array_equal(da[0], st["pos"])
    assert moved


# ---------------------------------------------------------------- 8. DELTA_CURRENT reads the state as it is now
def test_delta_current_reads_the_state_as_it_is_now():
    B = 130
    inp = wl.make_inputs(3, B=B, seed=43)
    g = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B)
    o = ol.Oracle(ol.panda_model(), ol.task_configs(inp["tasks"]), B, threads=8)
    for c in (g, o):
        ol.load_inputs(c, inp)
    tasks = {0: dict(mode="delta_current", blocks=("position", "orientation"), **MFT_SCALES), 1: dict(mode="delta_current", jt_scale=0.1)}
    kinds = kinds_of(g)
    g.set_action(tasks=tasks)
    action = np.random.default_rng(5).uniform(-1, 1, (13, B))

    def expect(before):
        q, dq = g.get_state()
        o.set_state(q, dq)  # the oracle's pose of the controller's state as it is now
        st = o.get_mft_status(0)
        return ar.apply_action(kinds, tasks, False, before, {0: (st["pos"], st["rot"])}, {1: q}, action)[0]

    g.tick()
    for _ in range(5):
        g.sim_step(None, dt=0.002)  # the state moves; no tick in between: the cached pose is the old one
    assert np.abs(g.get_state()[0] - inp["q"]).max() > 1e-6
    before = read_goals(g)
    g.apply_action(action)
    after, want = read_goals(g), expect(before)
    for t in range(2):
        err, bound = _bound(after[t], want[t])
        assert err < bound, (t, err)
    st0 = _status_at(o, inp["q"], inp["dq"])  # the pose before the steps is another one: the cached pose was not used
    stale = ar.apply_action(kinds, tasks, False, before, {0: (st0["pos"], st0["rot"])}, {1: inp["q"]}, action)[0]
    assert np.abs(after[0][:3] - stale[0][:3]).max() > 1e-9
    # behind a deferred update_task_models: the update is flushed first (launched ahead of the action), the result is the same
    g.set_state(inp["q"], inp["dq"])
    g.update_task_models()
    l0 = g.counters()[0]
    before = read_goals(g)
    assert g.counters()[0] == l0  # deferred: nothing launched yet
    g.apply_action(action)
    assert g.counters()[0] > l0 + 1
    after, want = read_goals(g), expect(before)
    for t in range(2):
        err, bound = _bound(after[t], want[t])
        assert err < bound, (t, err)


def _status_at(o, q, dq):
    o.set_state(q, dq)
    return o.get_mft_status(0)


# ---------------------------------------------------------------- 9. the resident loop
def test_resident_loop_equals_the_loop_through_the_host():
    import torch

    B, PERIODS, GAIN = 130, 20, 8.0
    inp = wl.make_inputs(3, B=B, seed=77)
    rng = np.random.default_rng(3)
    q0 = wl.sample_poses(rng, B, reject_ratio=0.1).T.copy()
    dq0 = np.zeros((7, B))
    obs = dict(blocks=["q"], tasks=[0], task_blocks=["error"], max_joint_speed=[0.6] + [1e9] * 6, max_episode_steps=7)
    act = dict(tasks={0: dict(mode="delta_current", blocks=("position", "orientation"), pos_scale=0.02, ori_scale=0.05, max_pos_lead=0.03)},
               clip_actions=True)

    def controller():
        g = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B)
        ol.load_inputs(g, inp)
        g.set_observation(**obs)
        g.set_action(**act)
        return g

    dev, host = controller(), controller()
    lay = dev.observation_layout()
    err_rows = slice(lay["error0"].start, lay["error0"].start + 6)  # sigma-projected position and orientation error
    rows = dev.observation_rows()
    q0_d, dq0_d = torch.from_numpy(q0).cuda(), torch.from_numpy(dq0).cuda()
    done_d = torch.zeros(B, dtype=torch.uint8, device="cuda")
    out_d = torch.zeros((rows, B), dtype=torch.float64, device="cuda")
    seen = []
    for _ in range(PERIODS):  # nothing in this loop touches the host
        dev.tick(want_output=False)
        dev.sim_step(None)
        dev.observe(out=out_d, done=done_d)
        a_d = torch.clamp(GAIN * out_d[err_rows], -1.5, 1.5).contiguous()  # the policy: a fixed function of the observation
        dev.apply_action(a_d)
        dev.reset_robots(done_d, q0_d, dq0_d)
        seen.append((out_d.clone(), done_d.clone(), a_d))
    dev_counts = []
    resets = clipped = 0
    for k in range(PERIODS):
        host.tick(want_output=False)
        host.sim_step(None)
        out, done = host.observe()
        a = np.clip(GAIN * out[err_rows], -1.5, 1.5)
        host.apply_action(a)
        counts = host.action_counts()
        host.reset_robots(done, q0, dq0)
        assert np.array_equal(seen[k][0].cpu().numpy(), out) and np.array_equal(seen[k][1].cpu().numpy(), done), k
        assert np.array_equal(seen[k][2].cpu().numpy(), a), k
        resets += int((done != 0).sum())
        clipped += counts["clipped"]
    assert 0 < resets < B * PERIODS and clipped > 0
    assert dev.action_counts() == counts  # of the last period
    assert all(np.array_equal(x, y) for x, y in zip(read_goals(dev), read_goals(host)))
    (qa, dqa), (qb, dqb) = dev.get_state(), host.get_state()
    assert np.array_equal(qa, qb) and np.array_equal(dqa, dqb)
    assert np.array_equal(dev.tick(), host.tick())


# ---------------------------------------------------------------- 10. not configured, or cleared
def test_routing():
    B = 65
    inp = wl.make_inputs(3, B=B, seed=3)

    def controller():
        g = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), B)
        ol.load_inputs(g, inp)
        return g

    g, plain = controller(), controller()
    action = np.ones((7, B))
    before, goals = g.counters(), read_goals(g)
    for _ in range(2):  # before set_action, and after clear_action
        assert g.lib.sai2b_apply_action(g.h, C.c_void_p(action.ctypes.data), None, 0) == _abi.INVALID_ARGUMENT
        assert b"no action is configured" in g.lib.sai2b_last_error(g.h)
        assert g.lib.sai2b_get_action_counts(g.h, (C.c_int * 3)()) == _abi.INVALID_ARGUMENT
        assert g.lib.sai2b_action_layout(g.h, 1, 0, None, None) == _abi.INVALID_ARGUMENT
        assert g.action_rows() == -1
        with pytest.raises(ValueError, match="no action is configured"):
            g.apply_action(action)
        assert g.counters() == before
        g.set_action(tasks={1: dict(mode="absolute")})
        assert g.action_rows() == 7 and g.action_layout() == {"joints1": slice(0, 7)} and g.counters() == before
        g.clear_action()
    assert all(np.array_equal(a, b) for a, b in zip(read_goals(g), goals))
    with pytest.raises(ValueError, match="blocks are for a MotionForceTask"):
        g.set_action(tasks={1: dict(mode="absolute", blocks=("position",))})
    with pytest.raises(ValueError, match="unknown mode"):
        g.set_action(tasks={0: dict(mode="relative", blocks=("position",))})
    with pytest.raises(ValueError, match="unknown block"):
        g.set_action(tasks={0: dict(mode="absolute", blocks=("pose",))})
    with pytest.raises(ValueError, match="no task has a mode"):
        g.set_action(tasks={})
    assert g.action_rows() == -1
    # jt_limits="model": the model's joint limits
    cfg = g.action_config(tasks={1: dict(mode="absolute", jt_limits="model")})
    assert list(cfg.task[1].jt_lower)[:7] == list(g.model.q_lower)[:7] and list(cfg.task[1].jt_upper)[:7] == list(g.model.q_upper)[:7]
    # one launch per apply
    g.set_action(tasks={0: dict(mode="delta_current", blocks=ar.BLOCKS, max_pos_lead=0.1), 1: dict(mode="delta_goal")}, clip_actions=True)
    l0 = g.counters()[0]
    g.apply_action(np.zeros((19, B)))
    assert g.counters()[0] == l0 + 1
    g.clear_action()
    # ten ticks of a context that configured and cleared an action equal those of one that never did, launch for launch
    write_goals(g, goals)
    l0, p0 = g.counters()[0], plain.counters()[0]
    for k in range(10):
        assert np.array_equal(g.tick(), plain.tick()), k
        for c in (g, plain):
            c.sim_step(None)
    assert g.counters()[0] - l0 == plain.counters()[0] - p0
