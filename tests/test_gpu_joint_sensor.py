"""GPU tests (-m gpu) of the joint sensors (csrc/sai2b_joint_sensor.hip: joint_sense_kernel; include/sai2b.h "joint sensors")
against tests/joint_sensor_reference.py and against twin contexts.

1: identity: with the ideal rows the measured pair is the truth bit for bit, and twelve periods of tick, sim_step(None),
   observe_reward, apply_action, reset_robots, with a goal change, a generator that changes its kind and a space
   re-parametrised between sim_step and the tick (all three read the cached pose), are bit-equal on every output to a twin
   without the feature: C3, C4, the generic route, a jerk-limited generator, 4 and 8 joints (tests/test_gpu_subset_reset.py's
   scenarios, 130 robots).
2: the law: each effect alone and all together at D = 3, everything at D = 8, both velocity modes, on planar_4r, six_r, Panda
   and sliding_base, B = 1, 5, 63, 64, 65, 200 and 4 099: after every sim_step the measured pair against the restatement fed
   the device's truth. Tolerances as on the CPU (1e-12 rad, 1e-10 rad/s; quantised positions exact; robots with some
   x / quantum within 1e-9 of a tie, decided by the reference, are left out of that period and of the later ones their
   history or filter carries it into: at most 1e-4 of all readings). A pure delay is bit-equal to the truth recorded d
   periods earlier, and to the first reading until d have passed.
3: who reads what: a context with offset and noise against a twin without the feature whose state is set to the measured
   pair: torques on every route (fast, cert, self, group, the task-level calls), observe rows and done bytes, delta_current
   goals; the truth after sim_step(tau) against a twin given the same truth and the same tau.
4: resets: reset_robots and reset_robots_sampled, set_state, reinitialize_robots. 5: shards. 6: snapshot banks. 7: the closed
   loop against numpy + the CPU oracle, and the resident loop with torch tensors against the loop through numpy. 8: device
   rows, rows rewritten between steps, argument checks that leave the context as it was, clear_joint_sensor."""
import ctypes as C

import numpy as np
import pytest

import external_wrench_cases as wc
import hardware_cases as hc
import joint_sensor_reference as jr
import oracle_lib as ol
import plumbing
import sai2_primitives_perso_amd as pkg
import test_gpu_subset_reset as sr
from sai2_primitives_perso_amd import _abi, sharding

pytestmark = pytest.mark.gpu

Q_TOL, V_TOL = 1e-12, 1e-10
SEED = 20261020
DT, SUBSTEPS = hc.DT, hc.SUBSTEPS
B = sr.B
EVERY = np.ones(B, dtype=bool)
FRAME_POS = (0.01, 0.02, 0.06)


def _rows(n, B, effect, D, seed=0):
    """per-robot rows with only `effect` on (delay: d cycling 0..D over the batch; 'all': everything); some joints of some robots
    keep a zero parameter inside a wavefront that draws"""
    rng = np.random.default_rng([n, B, seed, 31])
    rows = jr.ideal_rows(n, B)
    if effect in ("delay", "all") and D:
        rows[0] = np.arange(B) % (D + 1)
    if effect in ("offset", "all"):
        rows[1 : 1 + n] = rng.uniform(-0.02, 0.02, (n, B))
    if effect in ("noise", "all"):
        rows[1 + n : 1 + 2 * n] = rng.uniform(1e-4, 2e-3, (n, B))
        rows[1 + n, ::3] = 0.0
    if effect in ("quantum", "all"):
        rows[1 + 2 * n : 1 + 3 * n] = rng.uniform(1e-5, 1e-3, (n, B))
        rows[1 + 2 * n + 1, ::4] = 0.0
    if effect in ("velocity_noise", "all"):
        rows[1 + 3 * n : 1 + 4 * n] = rng.uniform(1e-3, 5e-2, (n, B))
        rows[1 + 3 * n, 1::3] = 0.0
    if effect in ("filter", "all"):
        rows[1 + 4 * n :] = rng.uniform(0.1, 1.0, (n, B))
        rows[1 + 4 * n, ::5] = 1.0
    return rows


def _controller(case):
    n = int(case["model"].dof)
    cfgs = [pkg.motion_force_task_config("m", link=case["link"], frame_pos=FRAME_POS, robot_dof=n), pkg.joint_task_config("j", robot_dof=n)]
    return pkg.Controller(case["model"], cfgs, case["q"].shape[1])


def _compare(got, ref, quantum, keep, what):
    """measured pair of the device against the restatement's, for the robots of `keep`"""
    qg, dqg = got
    qr, dqr = ref
    exact = (quantum > 0.0) & keep
    assert np.array_equal(qg[exact], qr[exact]), what
    eq, ev = np.abs(qg - qr)[:, keep].max(initial=0.0), np.abs(dqg - dqr)[:, keep].max(initial=0.0)
    assert eq < Q_TOL and ev < V_TOL, (what, eq, ev)
    return eq, ev


# ---------------------------------------------------------------------------------------------- 1: identity
def _mft(s):
    return s.kinds.index("mft")


def _equip(c, s):
    t = _mft(s)
    c.set_observation(blocks=("q", "dq", "tau", "limit_margin"), tasks=[t], task_blocks=("pose", "twist", "error"), success_tasks=[t], pos_tolerance=0.02,
                      ori_tolerance=10.0, joint_limit_margin=0.02, max_joint_speed=0.8, nonfinite=True)
    c.set_reward(terms=dict(alive=1.0, joint_speed=-0.01, torque=-0.001))
    c.set_action(tasks={t: dict(mode="delta_current", blocks=("position",), pos_scale=0.02, max_pos_lead=0.03)}, clip_actions=True)


def _other_goals(c, kinds):
    for t, k in enumerate(kinds):
        if k == "mft":
            g = c.get_mft_goals(t)
            c.set_mft_goals(t, np.roll(g[0], 3, axis=1), np.roll(g[1], 3, axis=1), None, None, None, None)
        else:
            c.set_jt_goals(t, np.roll(c.get_jt_goals(t)[0], 3, axis=1), None, None)


def _loop(c, s, periods, reparam=True):
    """the resident loop through numpy; -> every output of every period"""
    t = _mft(s)
    err = c.observation_layout()[f"error{t}"]
    last_jt = len(s.kinds) - 1
    out = []
    for k in range(periods):
        tau = c.tick()
        c.sim_step(None)
        if k == 3:
            _other_goals(c, s.kinds)
        if k == 5 and reparam:  # the generator changes its kind: it restarts at the cached pose
            cfg = c.tasks[last_jt]
            cfg.internal_otg_jerk_limited = 0 if cfg.internal_otg_jerk_limited else 1
            for i in range(cfg.task_dof):
                cfg.otg_max_jerk[i] = 25.0 + i
            c.update_task_config(last_jt, cfg)
        if k == 8 and reparam and s.name not in ("c4", "n4"):  # a force space appears: the spaces are re-parametrised at the cached pose
            cfg = c.tasks[t]
            cfg.force_space_dimension = 1
            for i in range(3):
                cfg.force_axis[i] = plumbing.FORCE_AXIS[i]
            c.update_task_config(t, cfg)
        obs, done, rew, _ = c.observe_reward(terms=False)
        c.apply_action(np.clip(8.0 * obs[err.start : err.start + 3], -1.5, 1.5))
        mask = (done != 0) | (sr.MASK_A if k % 4 == 2 else False)
        c.reset_robots(mask, s.q1, s.dq1)
        out.append([tau, *c.get_state(), obs, done, rew, *c.get_measured_state()] + sr.snapshot(c, s.kinds))
    return out


@pytest.mark.parametrize("name", ["c3", "c4", "generic", "jerk", "n4", "n8"])
def test_identity(name, monkeypatch):
    s = sr.scenario(name)
    a, twin = sr.contexts(s, 2, monkeypatch)
    a.set_joint_sensor(max_delay=3)
    for c in (a, twin):
        _equip(c, s)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_measured_state(), a.get_state()))
    ra, rt = _loop(a, s, 12), _loop(twin, s, 12)
    resets = 0
    for k, (x, y) in enumerate(zip(ra, rt)):
        sr.assert_columns(x, y, EVERY, f"period {k}")
        assert np.array_equal(x[1], x[6]) and np.array_equal(x[2], x[7]), k  # measured == truth
        resets += int((x[4] != 0).sum())
    assert 0 < resets < 12 * B
    st = a.joint_sensor_state()
    last = ra[-1][4] != 0  # robots reset in the last period were seeded by it
    assert st["clock"].max() <= 13 and np.all(st["clock"][last] == 1) and st["episode"].max() >= 1
    # and back: one view again, still the twin
    a.clear_joint_sensor()
    assert a.device_buffer(_abi.BUF_Q_MEASURED) is None and a.device_buffer(_abi.BUF_JOINT_SENSOR) is None
    for k, (x, y) in enumerate(zip(_loop(a, s, 3, reparam=False), _loop(twin, s, 3, reparam=False))):
        sr.assert_columns(x, y, EVERY, f"period {k} after the clear")


# ---------------------------------------------------------------------------------------------- 2: the law
LAW = [("planar_4r", 1, "all", 3, 1), ("planar_4r", 65, "offset", 3, 0), ("planar_4r", 200, "quantum", 3, 1), ("six_r", 5, "noise", 3, 0),
       ("six_r", 63, "all", 8, 1), ("six_r", 64, "velocity_noise", 3, 1), ("panda", 63, "filter", 3, 0), ("panda", 64, "all", 3, 0),
       ("panda", 65, "quantum", 3, 0), ("panda", 200, "all", 8, 0), ("panda", 4099, "all", 3, 1), ("sliding_base", 5, "all", 8, 1),
       ("sliding_base", 64, "noise", 3, 1), ("sliding_base", 65, "filter", 3, 1), ("sliding_base", 200, "velocity_noise", 3, 0),
       ("sliding_base", 1, "offset", 3, 0)]


def test_the_law_cases_cover_every_effect_size_and_batch():
    assert {c[2] for c in LAW} == {"offset", "noise", "quantum", "velocity_noise", "filter", "all"}
    assert {c[0] for c in LAW} == {"planar_4r", "six_r", "panda", "sliding_base"} and {c[1] for c in LAW} == {1, 5, 63, 64, 65, 200, 4099}
    assert {(c[3], c[4]) for c in LAW if c[2] == "all"} == {(3, 0), (3, 1), (8, 0), (8, 1)}


@pytest.mark.parametrize("robot, B, effect, D, mode", LAW)
def test_the_law(robot, B, effect, D, mode):
    case = wc.draw(robot, B)
    n = int(case["model"].dof)
    periods = 2 * D + 4
    rows = _rows(n, B, effect, D)
    g = _controller(case)
    g.set_state(case["q"], case["dq"])
    g.set_joint_sensor(rows, max_delay=D, velocity_mode=mode, seed=SEED)
    ref = jr.JointSensorReference(n, B, D, rows, mode, SEED)
    quantum = rows[1 + 2 * n : 1 + 3 * n]
    tainted = np.zeros(B, dtype=bool)  # robots whose history, filter or difference carries a reading that sat on a tie
    readings = left_out = 0
    worst = [0.0, 0.0]
    want = ref.seed(case["q"], case["dq"])
    cmds = hc.commands(case, periods)
    for p in range(periods + 1):
        if p:
            g.sim_step(cmds[p - 1], DT, SUBSTEPS, False)
            want = ref.step(*g.get_state(), DT)
        tainted |= ref.near_half.any(axis=0)
        readings, left_out = readings + B, left_out + int(tainted.sum())
        eq, ev = _compare(g.get_measured_state(), want, quantum, ~tainted, (p, effect))
        worst = [max(worst[0], eq), max(worst[1], ev)]
        st = g.joint_sensor_state()
        assert np.all(st["clock"] == p + 1) and not st["episode"].any()
    print(f"{robot} B={B} {effect} D={D} mode={mode}: {readings} readings, {left_out} left out, worst {worst[0]:.2e} rad {worst[1]:.2e} rad/s")
    assert left_out <= 1e-4 * readings
    q, dq = g.get_state()
    qm, dqm = g.get_measured_state()
    if effect != "filter":
        assert not np.array_equal(q, qm) or not np.array_equal(dq, dqm)
    # the views of the two buffers are the same numbers
    assert np.array_equal(plumbing.device_rows(g, _abi.BUF_Q_MEASURED, -1, n), qm) and np.array_equal(plumbing.device_rows(g, _abi.BUF_DQ_MEASURED, -1, n), dqm)


@pytest.mark.parametrize("robot, B, D, periods", [("planar_4r", 200, 3, 9), ("panda", 65, 3, 9), ("sliding_base", 64, 3, 9), ("six_r", 5, 8, 19), ("panda", 5, 8, 19)])
def test_delay_alone(robot, B, D, periods):
    """the measured pair of period p is, bit for bit, the truth of period max(p - d_b, 0); D = 3 with d_b cycling 0..3 over 9
    periods (the history wraps twice), D = 8 with d_b = 8 over 19"""
    case = wc.draw(robot, B)
    n = int(case["model"].dof)
    rows = jr.ideal_rows(n, B)
    rows[0] = np.arange(B) % (D + 1) if D == 3 else D
    g = _controller(case)
    g.set_state(case["q"], case["dq"])
    g.set_joint_sensor(rows, max_delay=D)
    truth = [np.stack(g.get_state())]
    cmds = hc.commands(case, periods)
    cols = np.arange(B)
    for p in range(1, periods + 1):
        g.sim_step(cmds[p - 1], DT, SUBSTEPS, False)
        truth.append(np.stack(g.get_state()))
        want = np.stack(truth)[np.maximum(p - rows[0].astype(int), 0), :, :, cols]  # [B][2][n]
        got = np.stack(g.get_measured_state())
        assert np.array_equal(got, want.transpose(1, 2, 0)), p
    assert not np.array_equal(truth[0], truth[1])


# ---------------------------------------------------------------------------------------------- 3: who reads what
def _noisy(c, n, **kw):
    """offset, noise, velocity noise and a filter; no delay, no quantum"""
    rows = _rows(n, c.B, "all", 0, seed=5)
    rows[1 + 2 * n : 1 + 3 * n] = 0.0
    c.set_joint_sensor(rows, seed=SEED, **kw)


@pytest.mark.parametrize("name", ["c3", "c4", "generic", "jerk", "n4", "n8"])
def test_who_reads_what(name, monkeypatch):
    """the controller side of `a` (offset, noise, filter; no quantum) reads the measured pair: a twin without the feature whose
    STATE is that pair gives the same torques, observations, done bytes and delta_current goals; the plant of `a` reads the
    truth: a third context given the same truth and the same torques ends at the same state"""
    s = sr.scenario(name)
    a, twin, plant = sr.contexts(s, 3, monkeypatch)
    _noisy(a, s.n)
    for c in (a, twin):
        _equip(c, s)
    t = _mft(s)
    for k in range(4):
        qm, dqm = a.get_measured_state()
        q, dq = a.get_state()
        assert not np.array_equal(qm, q)
        twin.set_state(qm, dqm)
        plant.set_state(q, dq)
        ta, tt = a.tick(), twin.tick()
        assert np.array_equal(ta, tt), k
        (oa, da), (ot, dt_) = a.observe(), twin.observe()
        assert np.array_equal(oa, ot) and np.array_equal(da, dt_), k
        lay = a.observation_layout()
        assert np.array_equal(oa[lay["q"]], qm) and np.array_equal(oa[lay["dq"]], dqm)
        act = np.random.default_rng(k).uniform(-1, 1, (a.action_rows(), B))
        a.apply_action(act)
        twin.apply_action(act)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_mft_goals(t), twin.get_mft_goals(t))), k
        a.sim_step(None)
        plant.sim_step(ta)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), plant.get_state())), k
        twin.sim_step(None)  # (keeps its tasks' bookkeeping going; its state is replaced at the top)
    # the status getters read the measured view too
    qm, dqm = a.get_measured_state()
    twin.set_state(qm, dqm)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_mft_velocity(t), twin.get_mft_velocity(t)))
    # get_bias is the plant's
    plant.set_state(*a.get_state())
    assert np.array_equal(a.get_bias(True), plant.get_bias(True))


def test_who_reads_what_task_level_calls_and_split_calls(monkeypatch):
    s = sr.scenario("c3")
    a, twin = sr.contexts(s, 2, monkeypatch)
    _noisy(a, s.n)
    twin.set_state(*a.get_measured_state())
    for c in (a, twin):
        c.update_task_models()
    assert np.array_equal(a.compute_control_torques(), twin.compute_control_torques())
    a.sim_step(None)
    twin.set_state(*a.get_measured_state())
    out = []
    for c in (a, twin):
        c.task_update_model(0)
        t0 = c.task_compute_torques(0)
        out.append(t0)
    assert np.array_equal(out[0], out[1]) and np.abs(out[0]).max() > 0
    a.sim_step(None)
    twin.set_state(*a.get_measured_state())
    m = sr.MASK_B
    for c in (a, twin):
        c.reinitialize_robots(m)
    sr.assert_columns(sr.snapshot(a, s.kinds)[2:], sr.snapshot(twin, s.kinds)[2:], EVERY, "reinitialize_robots reads the measured view")
    for c in (a, twin):
        c.reinitialize()
    sr.assert_columns(sr.snapshot(a, s.kinds)[2:], sr.snapshot(twin, s.kinds)[2:], EVERY, "reinitialize reads the measured view")
    assert np.array_equal(a.tick(), twin.tick())


# ---------------------------------------------------------------------------------------------- 4: resets
@pytest.mark.parametrize("sampled", [False, True])
def test_resets(sampled, monkeypatch):
    s = sr.scenario("c3")
    a, never = sr.contexts(s, 2, monkeypatch)
    rows = _rows(s.n, B, "all", 3, seed=9)
    rows[1 + 2 * s.n : 1 + 3 * s.n] = 0.0
    for c in (a, never):
        c.set_joint_sensor(rows, max_delay=3, seed=SEED)
        sr.run(c, 3)
    ref = jr.JointSensorReference(s.n, B, 3, rows, 0, SEED)
    mask = sr.MASK_A
    before = a.joint_sensor_state()
    if sampled:
        for c in (a, never):
            c.set_reset_sampler(seed=4, goal_tasks=())
        a.reset_robots_sampled(mask)
    else:
        a.reset_robots(mask, s.q1, s.dq1)
    st = a.joint_sensor_state()
    assert np.array_equal(st["clock"], np.where(mask, 1, before["clock"])) and np.array_equal(st["episode"], before["episode"] + mask)
    q, dq = a.get_state()
    if not sampled:
        assert np.array_equal(q[:, mask], s.q1[:, mask]) and np.array_equal(dq[:, mask], s.dq1[:, mask])
    ref.e[:] = before["episode"]
    want = ref.seed(q, dq, mask, next_episode=True)
    got = a.get_measured_state()
    assert np.abs(got[0] - want[0])[:, mask].max() < Q_TOL and np.abs(got[1] - want[1])[:, mask].max() < V_TOL
    assert not np.array_equal(got[0][:, mask], q[:, mask])
    # the tasks were re-initialised at the TRUE start pose: a twin without the feature reset to the same truth has the same goals
    plain = s.controller(monkeypatch)
    s.start(plain)
    plain.reset_robots(mask, q, dq)
    t = _mft(s)
    for x, y in zip(a.get_mft_goals(t)[:2], plain.get_mft_goals(t)[:2]):
        assert np.array_equal(x[:, mask], y[:, mask])
    assert np.array_equal(a.get_jt_goals(1)[0][:, mask], q[:, mask])
    # unselected robots: a context that never made the call, now and three periods on
    sr.assert_columns(sr.snapshot(a, s.kinds) + list(a.get_measured_state()), sr.snapshot(never, s.kinds) + list(never.get_measured_state()), ~mask, "unselected")
    ra, rn = sr.flat(sr.run(a, 3)), sr.flat(sr.run(never, 3))
    sr.assert_columns(ra, rn, ~mask, "unselected, periods after")
    # set_state re-seeds every robot, the episode kept
    e = a.joint_sensor_state()["episode"]
    a.set_state(s.q0, s.dq0)
    st = a.joint_sensor_state()
    assert np.all(st["clock"] == 1) and np.array_equal(st["episode"], e)
    ref.e[:] = e
    want = ref.seed(s.q0, s.dq0)
    got = a.get_measured_state()
    assert np.abs(got[0] - want[0]).max() < Q_TOL and np.abs(got[1] - want[1]).max() < V_TOL and np.array_equal(a.get_state()[0], s.q0)


# ---------------------------------------------------------------------------------------------- 5: shards
def test_two_shards_equal_one_context():
    Bw = 4099
    case = wc.draw("panda", Bw)
    rows = _rows(7, Bw, "all", 3, seed=2)
    cmds = hc.commands(case, 6)
    whole = _controller(case)
    whole.set_state(case["q"], case["dq"])
    whole.set_joint_sensor(rows, max_delay=3, seed=SEED, velocity_mode="finite_difference")
    parts = []
    for rank in range(2):
        lo, hi = sharding.shard_bounds(Bw, 2, rank)
        sub = dict(case, q=np.ascontiguousarray(case["q"][:, lo:hi]), dq=np.ascontiguousarray(case["dq"][:, lo:hi]))
        g = _controller(sub)
        g.set_state(sub["q"], sub["dq"])
        sharding.set_joint_sensor(g, 2, rank, Bw, rows, max_delay=3, seed=SEED, velocity_mode="finite_difference")
        assert g.joint_sensor()[0].first_robot == lo
        parts.append((g, lo, hi))
    for p in range(6):
        whole.sim_step(cmds[p], DT, SUBSTEPS, False)
        w = np.stack(whole.get_measured_state())
        for g, lo, hi in parts:
            g.sim_step(np.ascontiguousarray(cmds[p][:, lo:hi]), DT, SUBSTEPS, False)
            assert np.array_equal(np.stack(g.get_measured_state()), w[:, :, lo:hi]), p


# ---------------------------------------------------------------------------------------------- 6: snapshot banks
def test_snapshot_banks(monkeypatch):
    import test_gpu_snapshot as ts

    cs = ts.case("plant")
    s = cs.s
    rows = _rows(s.n, B, "all", 3, seed=3)

    def make():
        g = cs.controller(monkeypatch)
        cs.start(g)
        act, sen = g.hardware_rows(delay=np.arange(B) % 3, lag=0.6, noise=0.05)
        g.set_hardware(act, sen, max_delay=2, seed=11)
        g.set_joint_sensor(rows, max_delay=3, seed=SEED, velocity_mode="finite_difference")
        cs.run(g, 0, 6)
        return g

    def readable(g):
        st = g.joint_sensor_state()
        return cs.readable(g) + list(g.get_measured_state()) + [g.joint_sensor()[1], st["clock"][None].astype(float), st["episode"][None].astype(float)]

    a, twin = make(), make()
    both = _abi.SNAP_EPISODE | _abi.SNAP_ENVIRONMENT
    names = {r["block"] for r in a.snapshot_layout(both)}
    assert set(_abi.SNAP_JOINT_SENSOR_BLOCKS) <= names
    hist = [r for r in a.snapshot_layout(both) if r["block"] == "joint_sensor_history"][0]
    assert hist["rows"] == 4 * 2 * s.n
    bank = a.snapshot_bank(B, both)
    bank.save()
    # disturb: other goals, other rows, a reset, periods
    ts.other_goals(a, cs.kinds)
    a.set_joint_sensor(jr.ideal_rows(s.n, B), max_delay=3, seed=SEED, velocity_mode="finite_difference")
    a.reset_robots(sr.MASK_B, s.q1, s.dq1)
    cs.run(a, 6, 9)
    bank.load()
    sr.assert_columns(readable(a), readable(twin), EVERY, "after the load")
    for k, (x, y) in enumerate(zip(cs.run(a, 6, 12), cs.run(twin, 6, 12))):
        sr.assert_columns(x, y, EVERY, f"period {k} after the load")
    sr.assert_columns(readable(a), readable(twin), EVERY, "at the end")
    # clone: every robot continues as robot 7
    import torch

    bank.save()
    bank.load(slots=torch.full((B,), 7, dtype=torch.int32, device="cuda"))
    qm, dqm = a.get_measured_state()
    assert np.array_equal(qm, np.repeat(qm[:, 7:8], B, axis=1)) and np.all(a.joint_sensor_state()["clock"] == a.joint_sensor_state()["clock"][7])
    # export / import into a fresh context set up alike
    twin_bank = twin.snapshot_bank(B, both)
    twin_bank.save()
    blob = twin_bank.export()
    fresh = make()
    cs.run(fresh, 6, 8)
    fb = fresh.snapshot_bank(B, both)
    fb.import_(blob)
    fb.load()
    sr.assert_columns(readable(fresh), readable(twin), EVERY, "imported")
    for k, (x, y) in enumerate(zip(cs.run(fresh, 12, 15), cs.run(twin, 12, 15))):
        sr.assert_columns(x, y, EVERY, f"period {k} after the import")
    # a bank made before set_joint_sensor is refused, and the message names the block
    plain = cs.controller(monkeypatch)
    cs.start(plain)
    early = plain.snapshot_bank(B)
    early.save()
    plain.set_joint_sensor()
    for move in (early.save, early.load):
        with pytest.raises(ValueError, match="joint_sensor_q"):
            move()


# ---------------------------------------------------------------------------------------------- 7: closed loop
def test_closed_loop_against_numpy_and_the_cpu_oracle(monkeypatch):
    """the headline hierarchy, 100 periods with offset, noise and filtered tachometer velocity (no quantisation): the oracle
    ticks on the restatement's measured pair and steps the truth"""
    s = sr.scenario("regular")
    g, o = s.controller(monkeypatch), s.oracle()
    n = s.n
    rows = jr.make_rows(n, B, offset=np.random.default_rng(1).uniform(-0.01, 0.01, (n, B)), noise=2e-4, velocity_noise=5e-3,
                        velocity_alpha=np.random.default_rng(2).uniform(0.3, 1.0, (n, B)))
    for c in (g, o):
        s.start(c)
    g.set_joint_sensor(rows, seed=SEED)
    ref = jr.JointSensorReference(n, B, 0, rows, 0, SEED)
    q, dq = s.q0.copy(), s.dq0.copy()
    qm, dqm = ref.seed(q, dq)
    worst = [0.0, 0.0]
    for k in range(100):
        o.set_state(qm, dqm)
        tau = o.tick()
        o.set_state(q, dq)
        o.sim_step(tau)
        q, dq = o.get_state()
        qm, dqm = ref.step(q, dq, 0.001)
        g.tick(want_output=False)
        g.sim_step(None)
        gq, gdq = g.get_measured_state()
        worst = [max(worst[0], np.abs(gq - qm).max()), max(worst[1], np.abs(gdq - dqm).max())]
    print(f"closed loop, 100 periods: measured pair against numpy + oracle {worst[0]:.2e} rad {worst[1]:.2e} rad/s")
    assert worst[0] < Q_TOL and worst[1] < V_TOL
    tq, tdq = g.get_state()
    assert np.abs(tq - q).max() < Q_TOL and np.abs(tdq - dq).max() < V_TOL


def test_resident_loop_with_torch_equals_the_loop_through_numpy(monkeypatch):
    import torch

    s = sr.scenario("c3")
    dev, host = sr.contexts(s, 2, monkeypatch)
    rows = _rows(s.n, B, "all", 3, seed=4)
    host.set_joint_sensor(rows, max_delay=3, seed=SEED)
    t = _mft(s)
    seen = []
    with torch.cuda.stream(torch.cuda.Stream()):
        d = f"cuda:{dev._device}"
        # the rows built on the device from device tensors
        rows_d = dev.joint_sensor_rows(delay=torch.from_numpy(rows[0]).to(d), offset=torch.from_numpy(rows[1 : 1 + s.n]).to(d),
                                       noise=torch.from_numpy(rows[1 + s.n : 1 + 2 * s.n]).to(d), quantum=torch.from_numpy(rows[1 + 2 * s.n : 1 + 3 * s.n]).to(d),
                                       velocity_noise=torch.from_numpy(rows[1 + 3 * s.n : 1 + 4 * s.n]).to(d),
                                       velocity_alpha=torch.from_numpy(rows[1 + 4 * s.n :]).to(d))
        assert rows_d.is_cuda and np.array_equal(rows_d.cpu().numpy(), rows) and np.array_equal(host.joint_sensor_rows(*[rows[0]] + [rows[1 + k * s.n : 1 + (k + 1) * s.n] for k in range(5)]), rows)
        dev.set_joint_sensor(rows_d, max_delay=3, seed=SEED)
        for c in (dev, host):
            _equip(c, s)
        err = dev.observation_layout()[f"error{t}"]
        qm_d, dqm_d = dev.measured_state()
        q1_d, dq1_d = torch.from_numpy(s.q1).cuda(), torch.from_numpy(s.dq1).cuda()
        done_d = torch.zeros(B, dtype=torch.uint8, device="cuda")
        out_d = torch.zeros((dev.observation_rows(), B), dtype=torch.float64, device="cuda")
        rew_d = torch.zeros(B, dtype=torch.float64, device="cuda")
        for _ in range(12):  # nothing in this loop touches the host
            dev.tick(want_output=False)
            dev.sim_step(None)
            dev.observe_reward(out=out_d, done=done_d, reward=rew_d, terms=False)
            dev.apply_action(torch.clamp(8.0 * out_d[err.start : err.start + 3], -1.5, 1.5).contiguous())
            dev.reset_robots(done_d, q1_d, dq1_d)
            seen.append([x.clone() for x in (out_d, done_d, rew_d)])
        dev.synchronize()
        torch.cuda.current_stream().synchronize()
        views = [qm_d.cpu().numpy(), dqm_d.cpu().numpy()]
    for k in range(12):
        host.tick(want_output=False)
        host.sim_step(None)
        obs, done, rew, _ = host.observe_reward(terms=False)
        host.apply_action(np.clip(8.0 * obs[err.start : err.start + 3], -1.5, 1.5))
        host.reset_robots(done, s.q1, s.dq1)
        for x, y in zip(seen[k], (obs, done, rew)):
            assert np.array_equal(x.cpu().numpy(), y), k
    assert all(np.array_equal(x, y) for x, y in zip(views, host.get_measured_state()))
    assert all(np.array_equal(x, y) for x, y in zip(dev.get_measured_state(), host.get_measured_state()))


# ---------------------------------------------------------------------------------------------- 8: the rest
def test_device_rows_and_rows_rewritten_between_steps():
    import torch

    case = wc.draw("sliding_base", 65)
    n, Bc = 8, 65
    r0, r1 = _rows(n, Bc, "all", 3, seed=6), _rows(n, Bc, "all", 3, seed=7)
    g, h = _controller(case), _controller(case)
    for c in (g, h):
        c.set_state(case["q"], case["dq"])
    g.set_joint_sensor(torch.from_numpy(r0).cuda(), max_delay=3, seed=SEED)
    h.set_joint_sensor(r0, max_delay=3, seed=SEED)
    assert np.array_equal(g.joint_sensor()[1], r0)
    cmds = hc.commands(case, 6)
    ref = jr.JointSensorReference(n, Bc, 3, r0, 0, SEED)
    ref.seed(case["q"], case["dq"])
    for p in range(6):
        if p == 3:  # a device-resident producer rewrites the rows; the next step reads them
            g.synchronize()
            hip = C.CDLL(pkg._abi.LIB_PATH).hipMemcpy
            hip.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            assert hip(g.device_buffer(_abi.BUF_JOINT_SENSOR, -1), np.ascontiguousarray(r1).ctypes.data, r1.nbytes, 1) == 0
            ref.rows = r1.copy()
        g.sim_step(cmds[p], DT, SUBSTEPS, False)
        want = ref.step(*g.get_state(), DT)
        keep = ~ref.near_half.any(axis=0)
        _compare(g.get_measured_state(), want, ref.rows[1 + 2 * n : 1 + 3 * n], keep, p)
        if p < 3:
            h.sim_step(cmds[p], DT, SUBSTEPS, False)
            assert all(np.array_equal(x, y) for x, y in zip(g.get_measured_state(), h.get_measured_state()))
    # rows written by a device are not inspected: a NaN delay acts as 0
    bad = jr.ideal_rows(n, Bc)
    bad[0] = np.nan
    g.set_joint_sensor(torch.from_numpy(bad).cuda(), max_delay=3)
    g.sim_step(cmds[0], DT, SUBSTEPS, False)
    assert all(np.array_equal(x, y) for x, y in zip(g.get_measured_state(), g.get_state()))


def test_argument_checks_leave_the_context_as_it_was():
    case = wc.draw("panda", 5)
    n, Bc = 7, 5
    g = _controller(case)
    g.set_state(case["q"], case["dq"])
    # without the feature: NULL buffers, the defaults, the truth
    assert all(g.device_buffer(w) is None for w in (_abi.BUF_Q_MEASURED, _abi.BUF_DQ_MEASURED, _abi.BUF_JOINT_SENSOR))
    cfg, rows = g.joint_sensor()
    assert (cfg.max_delay, cfg.velocity_mode, cfg.seed) == (0, 0, 0) and np.array_equal(rows, jr.ideal_rows(n, Bc))
    assert not g.joint_sensor_state()["clock"].any() and all(np.array_equal(x, y) for x, y in zip(g.get_measured_state(), g.get_state()))
    with pytest.raises(ValueError, match="no joint sensor is set"):
        g.measured_state()
    good = _rows(n, Bc, "all", 3)
    g.set_joint_sensor(good, max_delay=3, seed=5, velocity_mode="finite_difference")
    g.sim_step(case["tau"], DT, SUBSTEPS, False)
    before = (g.joint_sensor()[1], *g.get_measured_state(), g.joint_sensor_state()["clock"])

    def bad(row, value, message, **kw):
        r = good.copy()
        r[row, 2] = value
        with pytest.raises(ValueError, match=message):
            g.set_joint_sensor(r, **dict(dict(max_delay=3), **kw))

    bad(0, 4, "the delay must be an integer in \\[0, max_delay\\]")
    bad(0, 1.5, "the delay must be an integer in \\[0, max_delay\\]")
    bad(0, -1, "the delay must be an integer in \\[0, max_delay\\]")
    bad(0, np.nan, "the delay must be an integer in \\[0, max_delay\\]")
    bad(1, np.inf, "the offset o must be finite")
    bad(1 + n, -1e-3, "the position noise s must be finite and not negative")
    bad(1 + 2 * n, np.nan, "the quantum Delta must be finite and not negative")
    bad(1 + 3 * n, -1.0, "the velocity noise r must be finite and not negative")
    bad(1 + 4 * n, 0.0, "the velocity filter coefficient alpha must be in \\(0, 1\\]")
    bad(1 + 4 * n, 1.5, "the velocity filter coefficient alpha must be in \\(0, 1\\]")
    with pytest.raises(ValueError, match="max_delay must be in"):
        g.set_joint_sensor(good, max_delay=9)
    with pytest.raises(ValueError, match="velocity_mode"):
        g.set_joint_sensor(good, velocity_mode="encoder")
    with pytest.raises(ValueError, match="velocity_mode must be 0"):
        g.set_joint_sensor(good, velocity_mode=2)
    with pytest.raises(ValueError, match="expected an array of shape"):
        g.set_joint_sensor(good[:, :4])
    cfgc = _abi.JointSensorConfig(max_delay=-1)
    assert g.lib.sai2b_set_joint_sensor(g.h, C.byref(cfgc), None, 0) == _abi.INVALID_ARGUMENT and b"max_delay" in g.lib.sai2b_last_error(g.h)
    assert g.lib.sai2b_set_joint_sensor(g.h, None, None, 0) == _abi.INVALID_ARGUMENT
    after = (g.joint_sensor()[1], *g.get_measured_state(), g.joint_sensor_state()["clock"])
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    cfg = g.joint_sensor()[0]
    assert (cfg.max_delay, cfg.velocity_mode, cfg.seed, cfg.first_robot) == (3, 1, 5, 0)
    # clear: one view, the state buffers keep the truth
    truth = g.get_state()
    g.clear_joint_sensor()
    g.clear_joint_sensor()
    assert g.device_buffer(_abi.BUF_Q_MEASURED) is None and all(np.array_equal(x, y) for x, y in zip(g.get_state(), truth))
    assert all(np.array_equal(x, y) for x, y in zip(g.get_measured_state(), truth))
