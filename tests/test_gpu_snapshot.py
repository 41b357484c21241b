"""GPU tests (-m gpu) of the snapshot banks (sai2b_snapshot_save / _load / _export / _import: csrc/sai2b_snapshot.hip), through
pkg.Controller and pkg.SnapshotBank.

The feature adds no arithmetic, so every comparison between contexts is np.array_equal, on the torques, q, dq, the
observation rows, the done bytes and every buffer the Python layer can read; the one tolerance is the project's 1e-10 against
the CPU oracle (relative to max(1, the robot's largest torque)).

Scenarios, masks and the history are those of tests/test_gpu_subset_reset.py (batch 130 = two wavefronts and a 2-lane tail;
eight robots inside a blending region, 6 % of the batch, so that no batch-wide kernel switch engages; `generic` runs with
SAI2B_NO_FAST_PATH): integral gains on, every generator mid-trajectory, then 30 periods of tick -> sim_step(None) -> observe.
Two more: `popc`, a closed-loop-force MotionForceTask with its passivity observer on (the 1 024-entry ring is filled by a
sensed force that differs per period and per robot), and `plant`, with per-robot payloads, contact planes, joint dynamics and a
timed push that is still counting down for most robots when the history ends."""
import numpy as np
import pytest

import plumbing
import sai2_primitives_perso_amd as pkg
import test_gpu_subset_reset as sr
from sai2_primitives_perso_amd import _abi
from sai2_primitives_perso_amd import workloads as wl
from test_gpu_subset_reset import AFTER, B, HISTORY, assert_columns, flat

pytestmark = pytest.mark.gpu

EVERY = np.ones(B, dtype=bool)
BOTH = _abi.SNAP_EPISODE | _abi.SNAP_ENVIRONMENT


class Case:
    """a scenario of test_gpu_subset_reset with an observation configured, or one of the two scenarios of this file;
    variant 1 of `plant` has other payloads and planes"""

    def __init__(self, name, variant=0):
        self.name, self.variant = name, variant
        self.s = sr.scenario("c3" if name in ("popc", "plant") else name)
        self.kinds, self.n = self.s.kinds, self.s.n
        rng = np.random.default_rng([31, len(name), variant])
        self.sensed = rng.normal(0, 3.0, (HISTORY + 2 * AFTER + 2, 3, B))
        self.mass, self.com = rng.uniform(0.2, 1.5, B), rng.normal(0, 0.03, (3, B))
        self.stiffness = rng.uniform(500, 2000, B)
        self.depth = rng.uniform(0.0005, 0.002, B)
        self.damping = rng.uniform(0.05, 0.4, (self.n, B))
        self.push = rng.normal(0, 4.0, (3, B))
        self.push_steps = rng.integers(5, 90, B).astype(np.float64)  # some pushes are over after the history, most are not

    def controller(self, monkeypatch, configs=None):
        s = self.s
        for k, v in s.env.items():
            monkeypatch.setenv(k, v)
        try:
            cfgs = s.configs() if configs is None else configs
            if self.name == "popc":
                c = cfgs[0]
                c.force_space_dimension, c.closed_loop_force, c.passivity_enabled = 1, 1, 1
                for i in range(3):
                    c.force_axis[i], c.ki_force[i] = plumbing.FORCE_AXIS[i], 1.3
            g = pkg.Controller(s.model(), cfgs, B)
        finally:
            for k in s.env:
                monkeypatch.delenv(k)
        mft = [t for t, k in enumerate(self.kinds) if k == "mft" and t < len(g.tasks)]
        blocks = ("q", "dq", "tau", "episode_step") + (("contact",) if self.name == "plant" else ())
        if self.name == "plant":
            pos = wl.frame_jacobian(*wl.fk(s.q0.T))[1].T
            point = pos + np.array([[0], [0], [1.0]]) * self.depth
            normal = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, B))
            g.set_link_payload(6, self.mass, self.com, None, target="both")
            g.set_contact(6, [wl.EE_FRAME_POS], point, normal, self.stiffness, np.full(B, 0.01), np.full(B, 0.2), sensor_task=0)
            g.set_joint_dynamics(damping=self.damping, friction=0.05)
            g.set_external_wrench(6, self.push, None, self.push_steps)
        g.set_observation(blocks=blocks, tasks=mft, task_blocks=("pose", "error", "sensed"), max_episode_steps=HISTORY + 5,
                          max_joint_speed=1.0)
        return g

    def start(self, c):
        self.s.start(c)
        if self.name == "popc":
            c.set_mft_goal_wrench(0, np.tile(np.array(plumbing.FORCE_AXIS)[:, None] * 5.0, (1, B)), None)

    def period(self, c, k):
        """period k of the script: what is fed from outside (the sensed force of `popc`), tick, sim_step, observe"""
        if self.name == "popc":
            c.set_mft_sensed_wrench(0, self.sensed[k], None)
        tau = c.tick()
        c.sim_step(None)
        obs, done = c.observe()
        return (tau,) + tuple(c.get_state()) + (obs, done)

    def run(self, c, k0, k1):
        return [self.period(c, k) for k in range(k0, k1)]

    def contexts(self, count, monkeypatch):
        cs = [self.controller(monkeypatch) for _ in range(count)]
        for c in cs:
            self.start(c)
            self.run(c, 0, HISTORY)
        return cs

    def readable(self, c):
        """every buffer the Python layer can read"""
        out = sr.snapshot(c, self.kinds[:len(c.tasks)]) + [plumbing.device_rows(c, _abi.BUF_TAU, -1, self.n)]
        for t, k in enumerate(self.kinds[:len(c.tasks)]):
            if k == "mft":
                out.append(plumbing.device_rows(c, _abi.BUF_SENSED, t, 6))
        if self.name == "plant":
            out += self.environment(c)
            cs, js, ws = c.get_contact_state(), c.get_joint_dynamics_state(), c.get_external_wrench_state()
            out += [cs["depth"], cs["normal_force"], cs["wrench_world"], ws["wrench_world"], ws["torque"]]
            out += [js[k].reshape(-1, B) for k in ("applied_torque", "stop_torque", "dissipative_torque")]
            out.append(c.get_external_wrench()[1][6:7])  # the remaining periods
        return [np.asarray(a) for a in out]

    def environment(self, c):
        """what sai2b_reset_robots keeps: payloads, contact rows, joint rows, the force and moment rows of the push"""
        out = [c.get_contact()[1]] + list(c.get_link_payload("controller")[1:]) + list(c.get_link_payload("plant")[1:])
        out += [c.get_joint_dynamics()[1].reshape(-1, B), c.get_external_wrench()[1][:6]]
        return [np.asarray(a) for a in out]


_cases = {}


def case(name, variant=0):
    if (name, variant) not in _cases:
        _cases[(name, variant)] = Case(name, variant)
    return _cases[(name, variant)]


def other_goals(c, kinds):
    """every task tracks another robot's goal"""
    for t, k in enumerate(kinds):
        if k == "mft":
            g = c.get_mft_goals(t)
            c.set_mft_goals(t, np.roll(g[0], 3, axis=1), np.roll(g[1], 3, axis=1), None, None, None, None)
        else:
            c.set_jt_goals(t, np.roll(c.get_jt_goals(t)[0], 3, axis=1), None, None)


def saved_and_disturbed(cs, a, bank):
    """save every robot of `a`, then other goals and AFTER periods"""
    bank.save()
    assert bank.counts() == dict(moved=B, out_of_range=0, never_saved=0)
    other_goals(a, cs.kinds)
    return cs.run(a, HISTORY, HISTORY + AFTER)


# ---- 1. round trip


@pytest.mark.parametrize("name", ["c3", "jerk", "generic", "c4", "n4", "n8", "popc", "plant"])
def test_round_trip(name, monkeypatch):
    cs = case(name)
    a, twin = cs.contexts(2, monkeypatch)
    bank = a.snapshot_bank(B, BOTH if name == "plant" else _abi.SNAP_EPISODE)
    disturbed = saved_and_disturbed(cs, a, bank)
    bank.load()
    assert bank.counts() == dict(moved=B, out_of_range=0, never_saved=0)
    assert_columns(cs.readable(a), cs.readable(twin), EVERY, "after the load")
    ra, rt = cs.run(a, HISTORY, HISTORY + AFTER), cs.run(twin, HISTORY, HISTORY + AFTER)
    for k, (x, y) in enumerate(zip(ra, rt)):
        assert_columns(x, y, EVERY, f"period {k} after the load")
    assert_columns(cs.readable(a), cs.readable(twin), EVERY, "at the end")
    # the detour was one: the disturbed periods are not the twin's
    assert not np.array_equal(disturbed[-1][0], rt[-1][0])
    if name == "popc":  # the observer's ring is in use
        assert np.abs(np.array([r[0] for r in rt])).max() > 0
    if name == "plant":  # a push is still counting down, another is over
        steps = a.get_external_wrench()[1][6]
        assert (steps > 0).any() and (steps == 0).any()
    bank.close()


def test_round_trip_against_the_cpu_oracle(monkeypatch):
    """regular poses, as the oracle comparison of test_gpu_subset_reset: the oracle runs HISTORY + AFTER periods without interruption"""
    cs = case("regular")
    s = cs.s
    a = cs.controller(monkeypatch)
    o = s.oracle()
    cs.start(a)
    s.start(o)
    cs.run(a, 0, HISTORY)
    for _ in range(HISTORY):
        sr.period(o)
    bank = a.snapshot_bank(B)
    saved_and_disturbed(cs, a, bank)
    bank.load()
    worst = 0.0
    for k in range(AFTER):
        tg, to = cs.period(a, HISTORY + k)[0], sr.period(o)
        err = (np.abs(tg - to).max(axis=0) / np.maximum(np.abs(to).max(axis=0), 1.0)).max()
        print(f"period {k} after the load: torque error vs the uninterrupted oracle {err:.3e}")
        worst = max(worst, err)
    assert worst < 1e-10, worst


# ---- 2. masked load


@pytest.mark.parametrize("pose", ["q_is_pose", "pose_kept"])
@pytest.mark.parametrize("mask", ["A", "B"])
def test_masked_load(mask, pose, monkeypatch):
    """selected robots continue as the twin that was never disturbed, the others as a context that never loaded. Loaded
    straight after a tick (the state buffer is every robot's cached pose) and after a sim_step (the pose has a column of its
    own); a generator that changes its kind afterwards restarts at the cached pose, which makes the pose count."""
    cs, m = case("c3"), sr.MASKS[mask]
    a, r0, twin = cs.contexts(3, monkeypatch)
    bank = a.snapshot_bank(B)
    saved_and_disturbed(cs, a, bank)
    other_goals(r0, cs.kinds)
    cs.run(r0, HISTORY, HISTORY + AFTER)
    if pose == "q_is_pose":
        for c in (a, r0):
            c.tick()
    bank.load(mask=m)
    assert bank.counts() == dict(moved=int(m.sum()), out_of_range=0, never_saved=0)
    for c in (a, r0, twin):
        cfg = c.tasks[1]
        cfg.internal_otg_jerk_limited = 1
        c.update_task_config(1, cfg)
    snaps = [cs.readable(c) for c in (a, twin, r0)]
    assert_columns(snaps[0], snaps[1], m, "selected, after the load")
    assert_columns(snaps[0], snaps[2], ~m, "unselected, after the load")
    runs = [flat(cs.run(c, HISTORY, HISTORY + AFTER)) for c in (a, twin, r0)]
    assert_columns(runs[0], runs[1], m, "selected, periods after")
    assert_columns(runs[0], runs[2], ~m, "unselected, periods after")
    assert not np.array_equal(runs[1][0][:, m], runs[2][0][:, m])  # the two references differ
    with pytest.raises(ValueError, match="otg_state of task 1|otg3_traj of task 1"):  # the layout has changed with the generator
        bank.save()


# ---- 3. clone


def test_clone(monkeypatch):
    cs = case("regular")
    a, twin = cs.contexts(2, monkeypatch)
    import torch

    bank = a.snapshot_bank(1)
    only = np.zeros(B, dtype=bool)
    only[70] = True
    bank.save(slots=np.zeros(B, dtype=np.int32), mask=only)
    assert bank.counts() == dict(moved=1, out_of_range=0, never_saved=0)
    bank.load(slots=torch.zeros(B, dtype=torch.int32, device="cuda"))
    assert bank.counts() == dict(moved=B, out_of_range=0, never_saved=0)
    for k in range(AFTER):
        x, y = cs.period(a, HISTORY + k), cs.period(twin, HISTORY + k)
        for u, v in zip(x, y):
            assert np.array_equal(u, np.repeat(v[..., 70:71], B, axis=-1)), k
    # not a stuck batch: with goals of their own the copies part
    rng = np.random.default_rng(3)
    a.set_jt_goals(1, a.get_jt_goals(1)[0] + 0.2 * rng.uniform(-1, 1, (7, B)), None, None)
    tau = cs.run(a, HISTORY + AFTER, HISTORY + 2 * AFTER)[-1][0]
    assert (np.abs(tau - tau[:, 70:71]).max(axis=0) > 0).sum() >= B - 1


# ---- 4. a bank unlike the batch


def test_bank_unlike_the_batch(monkeypatch):
    cs = case("c3")
    a, r0, twin = cs.contexts(3, monkeypatch)
    src = np.array([1, 62, 65, 3, 127])  # the robot slot i is saved from (slot 3 is not saved); regular poses, so that the copies
    # do not raise the share of robots in a blending region
    save_slots = np.full(B, -1, dtype=np.int32)
    save_slots[src] = np.arange(5)
    save_mask = np.zeros(B, dtype=bool)
    save_mask[src] = True
    save_mask[3] = False
    save_mask[[7, 8]] = True  # selected, slot -1
    save_slots[8] = 5  # selected, slot = capacity
    bank = a.snapshot_bank(5)
    with pytest.raises(ValueError, match="capacity"):
        bank.save()
    bank.save(save_slots, save_mask)
    assert bank.counts() == dict(moved=4, out_of_range=2, never_saved=0)
    other_goals(a, cs.kinds)
    other_goals(r0, cs.kinds)
    for c in (a, r0):
        cs.run(c, HISTORY, HISTORY + AFTER)
    rng = np.random.default_rng(11)
    slots = rng.choice(np.array([-1, 0, 1, 2, 3, 4, 5, 7], dtype=np.int32), B)
    slots[:8] = [-1, 0, 1, 2, 3, 4, 5, 7]
    mask = rng.uniform(size=B) < 0.8
    mask[:8] = True
    bank.load(slots, mask)
    good = mask & np.isin(slots, [0, 1, 2, 4])
    assert bank.counts() == dict(moved=int(good.sum()), out_of_range=int((mask & ((slots < 0) | (slots > 4))).sum()),
                                 never_saved=int((mask & (slots == 3)).sum()))
    assert good.sum() > 20 and (mask & (slots == 3)).sum() > 3
    origin = np.where(good, src[np.clip(slots, 0, 4)], 0)  # the twin's column a loaded robot continues as
    for k in range(AFTER):
        x, y, z = (cs.period(c, HISTORY + k) for c in (a, twin, r0))
        for u, v, w in zip(x, y, z):
            assert np.array_equal(u[..., good], v[..., origin[good]]), ("loaded", k)
            assert np.array_equal(u[..., ~good], w[..., ~good]), ("left alone", k)


# ---- 5. environment group


def test_environment_group(monkeypatch):
    p_case, q_case = case("plant"), case("plant", 1)
    p = p_case.contexts(1, monkeypatch)[0]
    q, q2 = q_case.contexts(2, monkeypatch)
    assert not np.array_equal(p_case.environment(p)[0], q_case.environment(q)[0])
    bank_p, bank_q = p.snapshot_bank(B, BOTH), q.snapshot_bank(B, BOTH)
    bank_p.save()
    bank_q.import_(bank_p.export())
    bank_q.load()
    assert_columns(p_case.readable(q), p_case.readable(p), EVERY, "after the load")
    assert_columns(flat(p_case.run(q, HISTORY, HISTORY + AFTER)), flat(p_case.run(p, HISTORY, HISTORY + AFTER)), EVERY, "periods after")
    # the episode group alone: the second context's payloads, planes, joint rows and pushes stay its own
    epi_p, epi_q = p.snapshot_bank(B, _abi.SNAP_EPISODE), q2.snapshot_bank(B, _abi.SNAP_EPISODE)
    before = q_case.environment(q2)
    epi_p.save()
    epi_q.import_(epi_p.export())
    epi_q.load()
    for x, y in zip(before, q_case.environment(q2)):
        assert np.array_equal(x, y)
    assert np.array_equal(q2.get_state()[0], p.get_state()[0])
    with pytest.raises(ValueError, match="block q"):  # a blob of other groups
        epi_q.import_(bank_p.export())


# ---- 6. checkpoint


@pytest.mark.parametrize("name", ["c3", "jerk"])
def test_checkpoint(name, monkeypatch):
    cs = case(name)
    a, twin = cs.contexts(2, monkeypatch)
    bank = a.snapshot_bank(B)
    bank.save()
    blob = bank.export()
    assert blob.dtype == np.uint8 and blob.size == bank.export_size()
    bank.close()
    a.close()
    fresh = cs.controller(monkeypatch)
    bank = fresh.snapshot_bank(B)
    bank.import_(blob)
    bank.load()
    assert_columns(flat(cs.run(fresh, HISTORY, HISTORY + AFTER)), flat(cs.run(twin, HISTORY, HISTORY + AFTER)), EVERY, "periods after")


def test_foreign_blobs_and_changed_layouts(monkeypatch):
    cs = case("c3")
    a = cs.contexts(1, monkeypatch)[0]
    bank = a.snapshot_bank(B)
    bank.save()
    blob = bank.export()
    jerk = case("jerk").contexts(1, monkeypatch)[0]  # the JointTask's generator is jerk-limited
    fewer = cs.controller(monkeypatch, configs=cs.s.configs()[:1])  # one task fewer
    for c, ccase, block in ((jerk, case("jerk"), "otg_state of task 1"), (fewer, cs, "of task 1")):
        other = c.snapshot_bank(B)
        before = ccase.readable(c)
        with pytest.raises(ValueError, match=block):
            other.import_(blob)
        other.load()  # nothing was imported: no slot is valid, no robot moves
        assert other.counts() == dict(moved=0, out_of_range=0, never_saved=B)
        assert_columns(ccase.readable(c), before, EVERY, "after the refused import")
    with pytest.raises(ValueError):
        a.snapshot_bank(2 * B).import_(blob)  # another capacity
    with pytest.raises(ValueError):
        bank.import_(blob[:-1])
    with pytest.raises(ValueError):
        bank.import_(np.zeros(blob.size, dtype=np.uint8))
    with pytest.raises(ValueError):
        a.snapshot_bank(0)
    # a contact the bank did not know about
    env = a.snapshot_bank(B, BOTH)
    pos = wl.frame_jacobian(*wl.fk(cs.s.q0.T))[1].T
    a.set_contact(6, [wl.EE_FRAME_POS], pos, np.tile(np.array([[0.0], [0.0], [1.0]]), (1, B)), np.full(B, 800.0))
    before = cs.readable(a)
    for b in (env, bank):
        with pytest.raises(ValueError, match="contact"):
            b.save()
        with pytest.raises(ValueError, match="contact"):
            b.load()
    assert_columns(cs.readable(a), before, EVERY, "after the refused calls")
    foreign = jerk.snapshot_bank(B)
    with pytest.raises(ValueError, match="another context"):
        a._rc(a.lib.sai2b_snapshot_save(a.h, foreign.h, None, None, 0))


# ---- 7. sizes


def _small(b, monkeypatch):
    """config 3 with both generators on and the integral gains, b robots"""
    inp = wl.make_inputs(3, B=b, seed=5)
    cfgs = [pkg.motion_force_task_config("m", internal_otg=True), pkg.joint_task_config("j", internal_otg=True)]
    for c in cfgs:
        plumbing._gains(c, False)
    g = pkg.Controller(pkg.panda_model(), cfgs, b)
    g.set_observation(blocks=("q", "episode_step"), max_episode_steps=7)
    g.set_state(inp["q"], inp["dq"])
    g.reinitialize()
    rng = np.random.default_rng(b)
    g.set_jt_goals(1, g.get_jt_desired(1)[0] + 0.1 * rng.uniform(-1, 1, (7, b)), None, None)
    return g


def _periods(g, n):
    out = []
    for _ in range(n):
        tau = g.tick()
        g.sim_step(None)
        out += [tau, *g.get_state(), *g.observe()]
    return out


@pytest.mark.parametrize("b", [1, 63, 64, 65, 4099])
def test_sizes(b, monkeypatch):
    a, twin = _small(b, monkeypatch), _small(b, monkeypatch)
    for g in (a, twin):
        _periods(g, 6)
    table = a.snapshot_layout(_abi.SNAP_EPISODE)
    words = a.snapshot_words(_abi.SNAP_EPISODE)
    assert words == sum(r["rows"] * r["elem_bytes"] // 4 for r in table) and words > 0
    assert {r["block"] for r in table if r["elem_bytes"] == 4} == {"istate", "episode_step"}
    cap = b + 3
    bank = a.snapshot_bank(cap)
    assert bank.export_size() == _abi.SNAPSHOT_HEADER_BYTES + words * 4 * cap + cap
    bank.save()
    assert bank.counts() == dict(moved=b, out_of_range=0, never_saved=0)
    valid = bank.export()[-cap:]
    assert valid[:b].all() and not valid[b:].any()
    a.set_jt_goals(1, np.roll(a.get_jt_goals(1)[0], 1, axis=1) + 0.05, None, None)
    _periods(a, 3)
    bank.load()
    assert bank.counts() == dict(moved=b, out_of_range=0, never_saved=0)
    for x, y in zip(_periods(a, 4), _periods(twin, 4)):
        assert np.array_equal(x, y)


def test_nan_payloads_survive(monkeypatch):
    """8-byte words move as they are: a NaN with a payload in a goal row comes back bit for bit"""
    a = _small(65, monkeypatch)
    odd = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000001, 0x7FF0000000000000, 0x8000000000000000], dtype=np.uint64).view(np.float64)
    goal = a.get_jt_goals(1)[0]
    goal[0, :4] = odd
    a.set_jt_goals(1, goal, None, None)
    bank = a.snapshot_bank(65)
    bank.save()
    a.set_jt_goals(1, np.zeros((7, 65)), None, None)
    bank.load()
    assert np.array_equal(a.get_jt_goals(1)[0].view(np.uint64), goal.view(np.uint64))


# ---- 8. stream contract


def test_stream_contract(monkeypatch):
    import torch

    cs = case("c3")
    a, h = cs.contexts(2, monkeypatch)
    rng = np.random.default_rng(21)
    slots = rng.permutation(B).astype(np.int32)
    mask = rng.uniform(size=B) < 0.6
    banks = [c.snapshot_bank(B) for c in (a, h)]
    for c, bank in zip((a, h), banks):
        bank.save()
        other_goals(c, cs.kinds)
        cs.run(c, HISTORY, HISTORY + 3)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        # filled by kernels on the caller's stream immediately before the call, overwritten immediately after it
        big = torch.randn(1 << 22, device="cuda").cumsum(0)  # (work ahead of the producers)
        d_slots = torch.from_numpy(slots).cuda() * 1 + (big[0] * 0).to(torch.int32)
        d_mask = torch.from_numpy(mask).cuda() & True
        banks[0].load(d_slots, d_mask)
        d_slots.fill_(-1)
        d_mask.zero_()
    banks[1].load(slots, mask)
    assert banks[0].counts() == banks[1].counts() == dict(moved=int(mask.sum()), out_of_range=0, never_saved=0)
    assert_columns(cs.readable(a), cs.readable(h), EVERY, "after the load")
    assert_columns(flat(cs.run(a, HISTORY, HISTORY + AFTER)), flat(cs.run(h, HISTORY, HISTORY + AFTER)), EVERY, "periods after")
    stream.synchronize()
