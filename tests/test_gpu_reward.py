"""sai2b_observe_reward on the GPU (include/sai2b.h "rewards and episode returns"): observe plus, in the same launch, the
reward of every robot and its episode accumulators.

1: every term alone and all together against tests/reward_reference.py on rows of the CPU oracle, within the project's bound
   for observation rows, 1e-12 max(1, |term|max); ALIVE, and DONE on the device's own byte, exact.
2: the reward is, bit for bit, the fold of the device's own term rows with the weights in layout order.
3: out, done, episode counters and done counts are those of sai2b_observe on a twin; a plain observe leaves the reward's state.
4: the accumulators over 12 calls, bit for bit, for gamma 0.9, 1 and 0; TORQUE_RATE and tau_prev.
5: non-finite rewards are replaced and counted and disturb nobody.  6: reset.  7: snapshot banks.  8: the resident loop.
9: host outputs equal device outputs, and outputs that are not wanted change nothing.  10: routing."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import reward_reference as rr
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi
from sai2_primitives_perso_amd import workloads as wl
from test_gpu_observe import PER_TASK, Scene, counts_of, tuned_criteria

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "planar_4r", "sliding_base", "two_mft"]
BATCHES = [1, 63, 65, 130, 4099]
WEIGHT = dict(alive=0.25, joint_speed=-0.01, torque=-1e-4, torque_rate=-1e-3, limit=-3.0, done=1.0)
TASK_WEIGHT = dict(pos=-1.0, pos_sq=-2.0, pos_tanh=0.7, ori=-0.3, ori_sq=-0.4, ori_tanh=0.5, lin_vel_sq=-0.05, ang_vel_sq=-0.02,
                   force_err_sq=-0.003, force_excess=-0.1)
DONE_VALUE = dict(success=10.0, joint_limit=-5.0, speed=-2.5, nonfinite=-20.0, force=-7.0, timeout=0.125)
SOFT_MARGIN, FORCE_SOFT_LIMIT = 0.3, 7.0
assert list(WEIGHT) == list(rr.TERMS) == list(_abi.REW_TERMS) and list(TASK_WEIGHT) == list(rr.TASK_TERMS) == list(_abi.REW_TASK_TERMS)


def _scales(t):
    return dict(pos_scale=0.1 * (t + 1), ori_scale=0.3 + 0.2 * t, force_soft_limit=FORCE_SOFT_LIMIT + t)


def reward_kwargs(mfts, terms=WEIGHT, task_terms=TASK_WEIGHT, gamma=0.9, nonfinite_reward=-123.0, soft_margin=SOFT_MARGIN):
    """keyword arguments of Controller.reward_config: the named terms with the weights above; task t's weights are scaled by
    1 + t / 2 so that two tasks do not share one"""
    tasks = {t: dict(terms={k: v * (1 + 0.5 * t) for k, v in task_terms.items()}, **_scales(t)) for t in mfts} if task_terms else None
    return dict(terms=dict(terms), tasks=tasks, done_value=DONE_VALUE, limit_soft_margin=soft_margin, gamma=gamma, nonfinite_reward=nonfinite_reward)


def layout_weights(lay, mfts):
    """weight of every term row, in layout order"""
    w = {}
    for name, row in lay.items():
        if name in WEIGHT:
            w[row] = WEIGHT[name]
        else:
            base = name.rstrip("0123456789")
            t = int(name[len(base):])
            w[row] = TASK_WEIGHT[base] * (1 + 0.5 * t)
    return [w[r] for r in sorted(w)]


def _close(a, ref):
    return np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.fixture(scope="module")
def scenes():
    """(Scene, reference rows, goal forces) per robot and batch: the oracle's rows are computed once and left unchanged"""
    cache = {}

    def get(robot, B):
        if (robot, B) not in cache:
            s = Scene(robot, B)
            rng = np.random.default_rng(7000 + B)
            goal_force = {}
            for t in s.mfts:
                goal_force[t] = rng.normal(0, 4, (3, B))
                for c in (s.o, s.g):
                    c.set_mft_goal_wrench(t, goal_force[t], rng.normal(0, 1, (3, B)))
            cache[(robot, B)] = (s, s.reference(), goal_force)
        return cache[(robot, B)]

    return get


def reference_rows(s, ref, goal_force, done, soft_margin, tau_prev=None, valid=None):
    """name -> [B] of every term, from the oracle's rows"""
    B = s.B
    tau_prev = np.zeros_like(s.tau) if tau_prev is None else tau_prev
    valid = np.zeros(B, bool) if valid is None else valid
    value = np.array([DONE_VALUE[k] for k in _abi.DONE_BITS])
    rows = rr.global_terms(s.dq, s.tau, tau_prev, valid, ref["limit_margin"][0], soft_margin, done, value)
    for t in s.mfts:
        sc = _scales(t)
        tt = rr.task_terms(s.g.tasks[t], ref[f"pose{t}"][3:], ref[f"twist{t}"], ref[f"error{t}"][6], ref[f"error{t}"][7], ref[f"sensed{t}"][:3],
                           goal_force[t], sc["pos_scale"], sc["ori_scale"], sc["force_soft_limit"])
        rows.update({f"{k}{t}": v for k, v in tt.items()})
    return rows


def observation_kwargs(s, ref):
    """every block and every criterion, thresholds from the oracle's values (tests/test_gpu_observe.py)"""
    kw, _ = tuned_criteria(s, ref)
    merged = {k: v for name in kw for k, v in kw[name].items()}
    return dict(blocks=list(_abi.OBS_BLOCKS), tasks=s.mfts, task_blocks=PER_TASK, max_episode_steps=50, **merged)


# ---------------------------------------------------------------- 1. and 2. terms against the reference, reward against the terms
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_terms_match_the_reference_and_the_reward_is_their_fold(scenes, robot, B):
    s, ref, goal_force = scenes(robot, B)
    g = s.g
    obs = observation_kwargs(s, ref)
    # the knee of the limit hinge from the oracle's margins: about half of the robots are inside it
    soft = float(np.median(ref["limit_margin"][0])) + (0.1 if B == 1 else 0.0)
    kwargs = functools.partial(reward_kwargs, soft_margin=soft)
    # all together
    g.set_observation(**obs)
    g.set_reward(**kwargs(s.mfts))
    lay = g.reward_layout()
    assert g.reward_rows() == 6 + 10 * len(s.mfts) and list(lay) == list(WEIGHT) + [f"{k}{t}" for t in s.mfts for k in TASK_WEIGHT]
    assert sorted(lay.values()) == list(range(g.reward_rows())) and list(lay.values()) == sorted(lay.values())
    out, done, reward, terms = g.observe_reward(terms=None)
    want = reference_rows(s, ref, goal_force, done, soft)
    for name, row in lay.items():
        err = np.abs(terms[row] - want[name]).max()
        print(f"{robot} B={B} {name}: max |d| = {err:.3e} (|x|max {np.abs(want[name]).max():.3g})")
        assert _close(terms[row], want[name]), name
    assert np.array_equal(terms[lay["alive"]], np.ones(B)) and np.array_equal(terms[lay["done"]], want["done"])
    assert np.array_equal(terms[lay["torque_rate"]], np.zeros(B))  # the first call has no tau_prev
    if B > 1:  # the criteria are tuned to about a third of the robots each
        assert (done != 0).any() and (terms[lay["done"]] != 0).any()
        assert (terms[lay["limit"]] > 0).any() and (terms[lay["limit"]] == 0).any()
        assert all((terms[lay[f"force_excess{t}"]] > 0).any() and (terms[lay[f"force_excess{t}"]] == 0).any() for t in s.mfts)
    assert np.array_equal(reward, rr.fold(list(terms), layout_weights(lay, s.mfts))) and np.isfinite(reward).all()
    assert g.reward_counts() == dict(closed=int((done != 0).sum()), replaced=0)
    # every term alone: its row is the row of the whole (bit for bit: the same instructions on the same inputs), its reward its fold
    for name, w in WEIGHT.items():
        g.set_observation(**obs)
        g.set_reward(**kwargs(s.mfts, terms={name: w}, task_terms=None))
        assert g.reward_rows() == 1 and g.reward_layout() == {name: 0}
        _, done1, r1, t1 = g.observe_reward(out=False, terms=None)
        assert np.array_equal(done1, done) and _close(t1[0], want[name]) and np.array_equal(t1[0], terms[lay[name]]), name
        assert np.array_equal(r1, rr.fold([t1[0]], [w])), name
    for name, w in TASK_WEIGHT.items():
        g.set_observation(**obs)
        g.set_reward(**kwargs(s.mfts, terms={}, task_terms={name: w}))
        assert g.reward_layout() == {f"{name}{t}": k for k, t in enumerate(s.mfts)}
        _, done1, r1, t1 = g.observe_reward(out=False, terms=None)
        for k, t in enumerate(s.mfts):
            assert _close(t1[k], want[f"{name}{t}"]), (name, t)
        assert np.array_equal(r1, rr.fold(list(t1), [w * (1 + 0.5 * t) for t in s.mfts])), name
    # the observation stores nothing and no criterion is on: the reward still visits its tasks
    g.set_observation(blocks=["q"])
    g.set_reward(**kwargs(s.mfts))
    _, done0, r0, t0 = g.observe_reward(out=False, terms=None)
    assert not done0.any()
    for name, row in lay.items():
        assert _close(t0[row], np.zeros(B) if name == "done" else want[name]), name
    assert np.array_equal(r0, rr.fold(list(t0), layout_weights(lay, s.mfts)))
    g.clear_reward()


# ---------------------------------------------------------------- contexts of the headline hierarchy without an oracle
def make_inputs(B, seed=77):
    inp = wl.make_inputs(3, B=B, seed=seed)
    rng = np.random.default_rng(seed)
    inp["sensed"] = (rng.normal(0, 5, (3, B)), rng.normal(0, 1, (3, B)))
    inp["goal_wrench"] = (rng.normal(0, 4, (3, B)), rng.normal(0, 1, (3, B)))
    return inp


OBS = dict(blocks=["q", "dq", "tau", "limit_margin", "episode_step"], tasks=[0], task_blocks=PER_TASK, max_joint_speed=[0.6] + [1e9] * 6,
           joint_limit_margin=0.05, nonfinite=True, force_tasks=[0], max_sensed_force=12.0, max_episode_steps=5)


def controller(inp, reward=True, obs=OBS, **kw):
    g = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), inp["q"].shape[1])
    ol.load_inputs(g, inp)
    g.set_mft_sensed_wrench(0, *inp["sensed"])
    g.set_mft_goal_wrench(0, *inp["goal_wrench"])
    if obs:
        g.set_observation(**obs)
    if reward:
        g.set_reward(**reward_kwargs([0], **kw))
    return g


def reward_buffers(g):
    g.synchronize()
    state, episode = g.reward_state()
    return state.cpu().numpy(), episode.cpu().numpy()


# ---------------------------------------------------------------- 3. observe is still observe
@pytest.mark.parametrize("B", BATCHES)
def test_observe_is_still_observe(B):
    inp = make_inputs(B)
    a, b = controller(inp), controller(inp, reward=False)
    for k in range(7):  # past the timeout: the episode counters restart on both
        ta, tb = a.tick(), b.tick()
        assert np.array_equal(ta, tb)
        for c in (a, b):
            c.sim_step(None)
        out_a, done_a, _, _ = a.observe_reward()
        out_b, done_b = b.observe()
        assert np.array_equal(out_a, out_b) and np.array_equal(done_a, done_b), k
        assert a.done_counts() == b.done_counts() == counts_of(done_b), k
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state()))
    # a plain observe on the context with a reward: what sai2b_observe gives, and the reward's buffers stay as they are
    state0, episode0 = reward_buffers(a)
    out_a, done_a = a.observe()
    out_b, done_b = b.observe()
    assert np.array_equal(out_a, out_b) and np.array_equal(done_a, done_b)
    state1, episode1 = reward_buffers(a)
    assert np.array_equal(state0, state1) and np.array_equal(episode0, episode1)


# ---------------------------------------------------------------- 4. the accumulators
@pytest.mark.parametrize("gamma", [0.9, 1.0, 0.0])
def test_accumulators_over_twelve_calls(gamma):
    B = 130
    inp = make_inputs(B, seed=5)
    g = controller(inp, gamma=gamma)
    lay, olay = g.reward_layout(), g.observation_layout()
    ref = rr.start_state(B)
    tau_prev, valid = np.zeros((7, B)), np.zeros(B, bool)
    closed_total = 0
    lengths = set()
    for k in range(12):
        tau = g.tick()
        g.sim_step(None)
        out, done, reward, terms = g.observe_reward(terms=None)
        assert np.array_equal(out[olay["tau"]], tau)
        # TORQUE_RATE: 0 without a valid tau_prev (the first call, the call after a done), else against the previous torques
        rate = np.where(valid, ((tau - tau_prev) ** 2).sum(axis=0), 0.0)
        assert np.array_equal(terms[lay["torque_rate"]][~valid], np.zeros((~valid).sum())), k
        assert _close(terms[lay["torque_rate"]], rate), k
        if k:
            assert valid.any() and (terms[lay["torque_rate"]][valid] > 0).all(), k
        assert np.array_equal(reward, rr.fold(list(terms), layout_weights(lay, [0]))), k
        rr.accumulate(ref, reward, done, out[olay["episode_step"]][0].astype(np.int32), gamma)
        stats = g.episode_stats()
        state, episode = reward_buffers(g)
        for name, row in (("ret", 0), ("disc", 1), ("last_return", 2)):
            assert np.array_equal(state[row], ref[name]) and np.array_equal(stats["discount" if name == "disc" else name], ref[name]), (k, name)
        assert np.array_equal(episode[0], ref["last_length"]) and np.array_equal(stats["last_length"], ref["last_length"]), k
        assert np.array_equal(state[3:], tau) and np.array_equal(episode[1], (done == 0).astype(np.int32)), k
        assert g.reward_counts() == dict(closed=int((done != 0).sum()), replaced=0), k
        tau_prev, valid = tau, done == 0
        closed_total += int((done != 0).sum())
        lengths |= set(ref["last_length"][done != 0])
    # robots ended episodes at different steps, every robot at least twice (the timeout is 5), and not all in one call
    assert closed_total >= 2 * B and len(lengths) > 1 and max(lengths) == 5
    if gamma == 0.0:
        assert set(np.unique(ref["disc"])) <= {0.0, 1.0}


# ---------------------------------------------------------------- 5. non-finite
def test_nonfinite_rewards_are_replaced_counted_and_disturb_nobody():
    B = 130
    inp = make_inputs(B, seed=11)
    clean, g = controller(inp), controller(inp)
    for c in (clean, g):
        c.tick()
    bad_q, bad_goal = np.array([0, 63, 64, 129]), np.array([5, 65, 100])
    q, dq = g.get_state()
    q[2, 0], q[6, 63], q[0, 64], q[3, 129] = np.nan, np.nan, np.nan, np.nan
    g.set_state(q, None)
    force, moment = inp["goal_wrench"][0].copy(), inp["goal_wrench"][1]
    force[0, 5], force[1, 65], force[2, 100] = np.nan, np.nan, np.nan
    g.set_mft_goal_wrench(0, force, moment)
    _, done_c, r_c, t_c = clean.observe_reward(terms=None)
    _, done, r, t = g.observe_reward(terms=None)
    bad = np.concatenate([bad_q, bad_goal])
    good = np.ones(B, bool)
    good[bad] = False
    assert np.array_equal(r[bad], np.full(bad.size, -123.0)) and np.isfinite(r).all()
    assert np.array_equal(r[good], r_c[good]) and np.array_equal(t[:, good], t_c[:, good]) and np.array_equal(done[good], done_c[good])
    assert np.array_equal(done[bad_q], np.full(bad_q.size, _abi.DONE_NONFINITE, np.uint8)) and np.array_equal(done[bad_goal], done_c[bad_goal])
    lay = g.reward_layout()
    assert np.isnan(t[lay["force_err_sq0"]][bad_goal]).all()  # the term rows keep what was computed
    assert g.reward_counts() == dict(closed=int((done != 0).sum()), replaced=bad.size)
    assert clean.reward_counts() == dict(closed=int((done_c != 0).sum()), replaced=0)
    # the replaced reward is what the accumulators took
    stats, stats_c = g.episode_stats(), clean.episode_stats()
    took = np.where(done != 0, stats["last_return"], stats["ret"])
    assert np.array_equal(took, r) and np.array_equal(stats["ret"][good], stats_c["ret"][good])


# ---------------------------------------------------------------- 6. reset
def test_reset_starts_the_selected_robots_returns():
    B = 130
    inp = make_inputs(B, seed=13)
    a, b = controller(inp), controller(inp)
    for _ in range(6):  # past the timeout: every robot has a last episode
        for c in (a, b):
            c.tick()
            c.sim_step(None)
            c.observe_reward(out=False, done=False, reward=False)
    state0, episode0 = reward_buffers(b)
    assert state0[2].any() and (episode0[0] > 0).all() and episode0[1].any() and (state0[1] != 1).any()
    mask = np.zeros(B, bool)
    mask[[0, 1, 62, 63, 64, 65, 100, 129]] = True
    l0 = a.counters()[0]
    a.reset_robots(mask)
    assert a.counters()[0] == l0 + 2  # the reset and the reward's own small launch
    state, episode = reward_buffers(a)
    assert np.array_equal(state[0][mask], np.zeros(mask.sum())) and np.array_equal(state[1][mask], np.ones(mask.sum()))
    assert not episode[1][mask].any()
    assert np.array_equal(state[2], state0[2]) and np.array_equal(episode[0], episode0[0])  # last_* are kept, for every robot
    assert np.array_equal(state[:, ~mask], state0[:, ~mask]) and np.array_equal(episode[:, ~mask], episode0[:, ~mask])
    # the next call of a reset robot has no TORQUE_RATE
    a.tick()
    a.sim_step(None)
    terms = a.observe_reward(out=False, done=False, reward=False, terms=None)[3]
    assert not terms[a.reward_layout()["torque_rate"]][mask].any()
    # a re-initialisation alone changes nothing
    state1, episode1 = reward_buffers(a)
    l0 = a.counters()[0]
    a.reinitialize_robots(mask)
    assert a.counters()[0] == l0 + 1
    state2, episode2 = reward_buffers(a)
    assert np.array_equal(state1, state2) and np.array_equal(episode1, episode2)
    # device mask
    import torch

    a.reset_robots(torch.from_numpy(~mask).cuda())
    state3, episode3 = reward_buffers(a)
    assert not state3[0][~mask].any() and (state3[1][~mask] == 1).all() and not episode3[1][~mask].any()
    assert np.array_equal(state3[:, mask], state2[:, mask]) and np.array_equal(state3[2], state2[2]) and np.array_equal(episode3[0], episode2[0])


# ---------------------------------------------------------------- 7. snapshot banks
def _period(c, n=1):
    seen = []
    for _ in range(n):
        c.tick()
        c.sim_step(None)
        out, done, reward, terms = c.observe_reward(terms=None)
        seen.append((out, done, reward, terms) + reward_buffers(c))
    return seen


def _same(xs, ys):
    return all(np.array_equal(x, y, equal_nan=True) for px, py in zip(xs, ys) for x, y in zip(px, py))


def test_snapshot_banks_hold_the_accumulators():
    import torch

    B = 130
    inp = make_inputs(B, seed=17)
    a, twin = controller(inp), controller(inp)
    early = a.snapshot_bank(B)  # made after set_reward: the layout has the two blocks
    _period(a, 3), _period(twin, 3)
    bank = a.snapshot_bank(B)
    bank.save()
    _period(a, 3)  # three more periods, then back
    bank.load()
    assert _same(_period(a, 5), _period(twin, 5))
    # export and import into a fresh context
    fresh = controller(inp)
    _period(fresh, 3)
    bank.save()  # a's state is the twin's now
    bank_f = fresh.snapshot_bank(B)
    bank_f.import_(bank.export())
    bank_f.load()
    assert _same(_period(fresh, 5), _period(twin, 5))
    # clone one slot into all robots: every robot continues as robot 7 of the bank does
    one = controller(inp)
    _period(one, 3)
    bank_1 = one.snapshot_bank(B)
    bank_1.save()
    bank_1.load(slots=torch.full((B,), 7, dtype=torch.int32, device="cuda"))
    state, episode = reward_buffers(one)
    assert (state == state[:, 7:8]).all() and (episode == episode[:, 7:8]).all()
    seen = _period(one, 2)
    for p in seen:
        for x in p:
            assert np.array_equal(x, np.repeat(x[..., 7:8], B, axis=-1), equal_nan=True)
    # a bank made before set_reward is refused, and the message names the block
    plain = controller(inp, reward=False)
    before = plain.snapshot_bank(B)
    before.save()
    plain.set_reward(**reward_kwargs([0]))
    for move in (before.save, before.load):
        with pytest.raises(ValueError, match="reward_state"):
            move()
    early.save()  # the layout of `a` has not changed since


# ---------------------------------------------------------------- 8. the resident loop
def test_resident_loop_equals_the_loop_through_the_host():
    import torch

    B, PERIODS, GAIN = 130, 20, 8.0
    inp = make_inputs(B)
    rng = np.random.default_rng(3)
    q0 = wl.sample_poses(rng, B, reject_ratio=0.1).T.copy()
    dq0 = np.zeros((7, B))
    act = dict(tasks={0: dict(mode="delta_current", blocks=("position", "orientation"), pos_scale=0.02, ori_scale=0.05, max_pos_lead=0.03)},
               clip_actions=True)
    dev, host = controller(inp), controller(inp)
    for c in (dev, host):
        c.set_action(**act)
    lay = dev.observation_layout()
    err_rows = slice(lay["error0"].start, lay["error0"].start + 6)
    seen = []
    with torch.cuda.stream(torch.cuda.Stream()):
        q0_d, dq0_d = torch.from_numpy(q0).cuda(), torch.from_numpy(dq0).cuda()
        done_d = torch.zeros(B, dtype=torch.uint8, device="cuda")
        out_d = torch.zeros((dev.observation_rows(), B), dtype=torch.float64, device="cuda")
        reward_d = torch.zeros(B, dtype=torch.float64, device="cuda")
        terms_d = torch.zeros((dev.reward_rows(), B), dtype=torch.float64, device="cuda")
        for _ in range(PERIODS):  # nothing in this loop touches the host
            dev.tick(want_output=False)
            dev.sim_step(None)
            dev.observe_reward(out=out_d, done=done_d, reward=reward_d, terms=terms_d)
            a_d = torch.clamp(GAIN * out_d[err_rows], -1.5, 1.5).contiguous()  # the policy: a fixed function of the observation
            dev.apply_action(a_d)
            dev.reset_robots(done_d, q0_d, dq0_d)
            seen.append([x.clone() for x in (out_d, done_d, reward_d, terms_d)])
        torch.cuda.current_stream().synchronize()
    resets = 0
    for k in range(PERIODS):
        host.tick(want_output=False)
        host.sim_step(None)
        got = host.observe_reward(terms=None)
        host.apply_action(np.clip(GAIN * got[0][err_rows], -1.5, 1.5))
        host.reset_robots(got[1], q0, dq0)
        for x, y in zip(seen[k], got):
            assert np.array_equal(x.cpu().numpy(), y), k
        resets += int((got[1] != 0).sum())
    assert 0 < resets < B * PERIODS
    for x, y in zip(reward_buffers(dev), reward_buffers(host)):
        assert np.array_equal(x, y)
    sd, sh = dev.episode_stats(), host.episode_stats()
    assert all(np.array_equal(sd[k], sh[k]) for k in sd) and sd["last_return"].any()
    assert np.array_equal(dev.tick(), host.tick())


# ---------------------------------------------------------------- 9. host output equals device output
def test_host_output_equals_device_output_and_unwanted_outputs_change_nothing():
    import torch

    B = 65
    inp = make_inputs(B, seed=19)
    a, b, c = controller(inp), controller(inp), controller(inp)
    out_d = torch.zeros((a.observation_rows(), B), dtype=torch.float64, device="cuda")
    done_d = torch.zeros(B, dtype=torch.uint8, device="cuda")
    reward_d = torch.zeros(B, dtype=torch.float64, device="cuda")
    terms_d = torch.zeros((a.reward_rows(), B), dtype=torch.float64, device="cuda")
    for k in range(7):
        for g in (a, b, c):
            g.tick()
            g.sim_step(None)
        a.observe_reward(out=out_d, done=done_d, reward=reward_d, terms=terms_d)
        torch.cuda.synchronize()
        got = b.observe_reward(terms=None)
        for x, y in zip((out_d, done_d, reward_d, terms_d), got):
            assert np.array_equal(x.cpu().numpy(), y), k
        # nothing wanted: one launch that still advances the counters and the accumulators
        l0 = c.counters()[0]
        assert c.observe_reward(out=False, done=False, reward=False, terms=False) == (None, None, None, None)
        assert c.counters()[0] == l0 + 1
        assert c.done_counts() == b.done_counts() and c.reward_counts() == b.reward_counts()
        for x, y, z in zip(reward_buffers(a), reward_buffers(b), reward_buffers(c)):
            assert np.array_equal(x, y) and np.array_equal(y, z), k
    # only the reward, as a device tensor
    a.tick(), b.tick()
    assert a.observe_reward(out=False, done=False, reward=reward_d, terms=False)[2] is reward_d
    torch.cuda.synchronize()
    assert np.array_equal(reward_d.cpu().numpy(), b.observe_reward()[2])
    with pytest.raises(ValueError, match="mixing host arrays and device tensors"):
        a.observe_reward(out=False, done=False, reward=reward_d, terms=np.zeros((a.reward_rows(), B)))
    with pytest.raises(ValueError, match="reward must be"):
        a.observe_reward(reward=np.zeros(B + 1))
    with pytest.raises(ValueError, match="terms must be"):
        a.observe_reward(terms=np.zeros((a.reward_rows() + 1, B)))


# ---------------------------------------------------------------- 10. routing
def test_routing():
    B = 65
    inp = make_inputs(B, seed=3)
    g, plain = controller(inp, reward=False, obs=None), controller(inp, reward=False, obs=None)
    r, t = np.zeros(B), np.zeros((1, B))
    cfg = g.reward_config(terms=dict(alive=1.0))
    before = g.counters()

    def refused(text):
        assert g.lib.sai2b_observe_reward(g.h, None, None, C.c_void_p(r.ctypes.data), C.c_void_p(t.ctypes.data), 0) == _abi.INVALID_ARGUMENT
        assert text in g.lib.sai2b_last_error(g.h) and g.counters() == before and not r.any() and not t.any()

    # no observation: no reward can be set, nothing is launched
    refused(b"no observation is configured")
    assert g.lib.sai2b_set_reward(g.h, C.byref(cfg)) == _abi.INVALID_ARGUMENT and b"no observation is configured" in g.lib.sai2b_last_error(g.h)
    with pytest.raises(ValueError, match="no observation is configured"):
        g.set_reward(terms=dict(alive=1.0))
    assert g.reward_rows() == -1 and not g.device_buffer(_abi.BUF_REWARD_STATE) and not g.device_buffer(_abi.BUF_REWARD_EPISODE)
    # an observation and no reward
    g.set_observation(blocks=["q"], nonfinite=True)
    for _ in range(2):  # before set_reward, and after clear_reward
        refused(b"no reward is configured")
        assert g.lib.sai2b_get_reward_counts(g.h, (C.c_int * 2)()) == _abi.INVALID_ARGUMENT
        assert g.lib.sai2b_get_episode_stats(g.h, None, None, None, None) == _abi.INVALID_ARGUMENT
        assert g.lib.sai2b_reward_layout(g.h, 1, -1, None, None) == _abi.INVALID_ARGUMENT
        with pytest.raises(ValueError, match="no reward is configured"):
            g.observe_reward()
        g.set_reward(terms=dict(alive=1.0))
        assert g.reward_rows() == 1 and g.counters() == before
        assert g.device_buffer(_abi.BUF_REWARD_STATE) and g.device_buffer(_abi.BUF_REWARD_EPISODE)
        g.clear_reward()
        assert g.reward_rows() == -1 and not g.device_buffer(_abi.BUF_REWARD_STATE)
    # a reward and the observation cleared
    g.set_reward(terms=dict(alive=1.0))
    g.clear_observation()
    refused(b"no observation is configured")
    g.set_observation(blocks=["q"], nonfinite=True)
    with pytest.raises(ValueError, match="not a MotionForceTask"):
        g.set_reward(tasks={1: dict(terms=dict(pos=1.0))})
    with pytest.raises(ValueError, match="unknown reward term"):
        g.set_reward(terms=dict(bonus=1.0))
    # one launch per call, whatever is selected
    g.set_reward(**reward_kwargs([0]))
    l0 = g.counters()[0]
    g.observe_reward(terms=None)
    assert g.counters()[0] == l0 + 1
    # a context that never sets a reward launches what it did: per tick, per observe, per reset
    plain.set_observation(blocks=["q"], nonfinite=True)
    mask = np.arange(B) % 3 == 0
    for call, extra in ((lambda c: c.tick(), 0), (lambda c: c.sim_step(None), 0), (lambda c: c.observe(), 0), (lambda c: c.reset_robots(mask), 1),
                        (lambda c: c.reinitialize_robots(mask), 0)):
        l0, p0 = g.counters()[0], plain.counters()[0]
        call(g), call(plain)
        assert g.counters()[0] - l0 == plain.counters()[0] - p0 + extra
    g.clear_reward()
    l0, p0 = g.counters()[0], plain.counters()[0]
    g.reset_robots(mask), plain.reset_robots(mask)
    assert g.counters()[0] - l0 == plain.counters()[0] - p0
    assert np.array_equal(g.tick(), plain.tick())
