"""GPU tests (-m gpu) of sai2b_end_episodes (csrc/sai2b_collision.hip: end_episodes_kernel; include/sai2b.h "collision
proximity"), B = 65 and 200, host arrays and device tensors.

Five periods of tick, sim_step, observe_reward with a timeout of 3 steps. A first call at period 1 (made by the context under
test AND by its twin: common history) ends the episodes of every fourth robot, so that at period 3 the others time out by
themselves and these do not. The call under test runs at period 3 with a scattered `extra`; the twin does not make it.
  selected, not done: last_return bit-equal to ret before the call, last_length equal to the counter, ret = 0, disc = 1, the next
    observe_reward reports EPISODE_STEP 1 and a TORQUE_RATE term of exactly 0;
  selected, already done: every accumulator bit-equal to the twin, the byte gains the bit;
  unselected: bit-equal to the twin through period 5, their bytes of done_inout and the guard bytes around it untouched;
  the count is exact. Without a reward, and without an observation, the call does the part that exists.
The resident loop tick, sim_step, observe_reward, collision_query, end_episodes, reset_robots_sampled with torch tensors gives
flags, done bytes, returns and states bit-equal to the same loop through numpy staging, over ten periods."""
import numpy as np
import pytest

import collision_cases as cc
import external_wrench_cases as wc
import plumbing
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

pytestmark = pytest.mark.gpu

TIMEOUT = 3
# of the resident loop: pairs of spheres on links four apart (the cell's twelve spheres overlap along the arm, so the default
# pairs flag nearly every robot); with these margins a minority of the robots is flagged
MARGINS = (0.02, 0.05, 0.0)
PAIRS = ((0, 4), (0, 5), (0, 6), (1, 5), (1, 6), (2, 6))


def _controller(case):
    n = int(case["model"].dof)
    cfgs = [pkg.motion_force_task_config("m", link=case["link"], frame_pos=(0.01, 0.02, 0.06), robot_dof=n), pkg.joint_task_config("j", robot_dof=n)]
    c = pkg.Controller(case["model"], cfgs, case["q"].shape[1])
    c.set_state(case["q"], 0.2 * case["dq"])
    return c


def _equip(c, observation=True, reward=True):
    if observation:
        c.set_observation(blocks=("q", "episode_step"), max_episode_steps=TIMEOUT, nonfinite=True)
    if reward:
        c.set_reward(terms=dict(alive=1.0, joint_speed=-0.01, torque=-0.001, torque_rate=-0.01), gamma=0.97)


def _accumulators(c):
    """the reward's accumulators: state [3 + dof][B] (ret, disc, last_return, tau_prev), episode [2][B] int32 (last_length, valid)"""
    n, B = c.dof, c.B
    st = plumbing.device_rows(c, _abi.BUF_REWARD_STATE, -1, 3 + n)
    ep = plumbing.device_rows(c, _abi.BUF_REWARD_EPISODE, -1, 1).view(np.int32).reshape(2, B)
    return st, ep


def _period(c):
    c.tick(want_output=False)
    c.sim_step(None)
    return c.observe_reward(terms=None)


@pytest.mark.parametrize("B, on_device, bit", [(65, True, 64), (200, False, 128), (65, False, 64), (200, True, 128)])
def test_end_episodes_at_period_three(B, on_device, bit):
    case = wc.draw("panda", B)
    a, twin = _controller(case), _controller(case)
    for c in (a, twin):
        _equip(c)
    step_row = a.observation_layout()["episode_step"].start
    rate_row = a.reward_layout()["torque_rate"]
    early = np.arange(B) % 4 == 1
    extra = np.zeros(B, dtype=np.uint8)
    extra[np.random.default_rng(B).random(B) < 0.4] = 1
    extra[:8] = [1, 1, 0, 0, 1, 0, 3, 0]  # both kinds of robot selected and left alone for certain; any non-zero byte selects
    sel = extra != 0
    for p in range(1, 6):
        ra, rt = _period(a), _period(twin)
        obs, done = ra[0], ra[1]
        if p <= 3:
            for x, y in zip(ra, rt):
                assert np.array_equal(x, y), p
        if p == 1:  # common history: every fourth robot's episode ends here, in both contexts
            assert not done.any()
            for c, d in ((a, done), (twin, rt[1])):
                c.end_episodes(d, early.astype(np.uint8), 128)
                assert np.array_equal(d != 0, early) and c.end_episode_count() == int(early.sum())
        if p == 3:
            by_itself = done != 0
            assert np.array_equal(by_itself, ~early) and (done[by_itself] == _abi.DONE_BITS["timeout"]).all()
            assert (sel & by_itself).any() and (sel & ~by_itself).any() and (~sel & by_itself).any() and (~sel & ~by_itself).any()
            counter = np.where(by_itself, 0, obs[step_row]).astype(np.int32)
            st0, ep0 = _accumulators(a)
            if on_device:
                import torch

                guard = torch.full((B + 128,), 0x5A, dtype=torch.uint8, device="cuda")
                guard[64 : 64 + B] = torch.from_numpy(done).cuda()
                d_dev = guard[64 : 64 + B]
                a.end_episodes(d_dev, torch.from_numpy(extra).cuda(), bit)
                a.synchronize()
                h = guard.cpu().numpy()
                assert (h[:64] == 0x5A).all() and (h[64 + B :] == 0x5A).all()
                after = h[64 : 64 + B].copy()
            else:
                after = done.copy()
                a.end_episodes(after, extra, bit)
            assert np.array_equal(after[~sel], done[~sel]) and np.array_equal(after[sel], done[sel] | bit)
            closed = sel & ~by_itself
            assert a.end_episode_count() == int(closed.sum())
            st1, ep1 = _accumulators(a)
            stt, ept = _accumulators(twin)
            # selected, not done: closed as step 5 closes an episode
            assert np.array_equal(st1[2, closed], st0[0, closed]) and np.array_equal(ep1[0, closed], counter[closed]) and (counter[closed] == 2).all()
            assert (st1[0, closed] == 0.0).all() and (st1[1, closed] == 1.0).all() and (ep1[1, closed] == 0).all()
            assert np.array_equal(st1[3:, closed], st0[3:, closed])  # tau_prev itself is left as it is: it is invalid
            # everyone else: the twin's accumulators
            assert np.array_equal(st1[:, ~closed], stt[:, ~closed]) and np.array_equal(ep1[:, ~closed], ept[:, ~closed])
            assert np.array_equal(st0, stt) and np.array_equal(ep0, ept)
        if p == 4:
            closed = sel & early
            assert (obs[step_row, closed] == 1.0).all() and (ra[3][rate_row, closed] == 0.0).all()
            others = ~closed
            assert (ra[3][rate_row, others & early] != 0.0).any()
            for x, y in zip(ra, rt):
                assert np.array_equal(x[..., others], y[..., others]), p
            # the twin's early robots time out now; those the call closed do not
            assert (rt[1][early] != 0).all() and (done[closed] == 0).all()
        if p == 5:
            others = ~(sel & early)
            for x, y in zip(ra, rt):
                assert np.array_equal(x[..., others], y[..., others]), p
    sa, st = a.episode_stats(), twin.episode_stats()
    for k in sa:
        assert np.array_equal(sa[k][others], st[k][others]), k


@pytest.mark.parametrize("B", [65, 200])
def test_the_call_does_the_part_that_exists(B):
    case = wc.draw("panda", B)
    extra = (np.arange(B) % 3 == 0).astype(np.uint8)
    # no observation, no reward: the bytes and the count
    c = _controller(case)
    done = np.zeros(B, dtype=np.uint8)
    done[::2] = 4
    want = np.where(extra != 0, done | 64, done)
    c.end_episodes(done, extra)
    assert np.array_equal(done, want) and c.end_episode_count() == int(((extra != 0) & (want == 64)).sum())
    # an observation alone: its counter restarts
    _equip(c, reward=False)
    step_row = c.observation_layout()["episode_step"].start
    for _ in range(2):
        obs, done = c.observe()
    assert (obs[step_row] == 2).all() and not done.any()
    c.end_episodes(done, extra, 128)
    assert np.array_equal(done, np.where(extra != 0, 128, 0)) and c.end_episode_count() == int(extra.sum())
    obs, done = c.observe()
    assert np.array_equal(obs[step_row], np.where(extra != 0, 1.0, 3.0))
    # a reward whose observation was cleared afterwards: the accumulators, with a length of 0
    _equip(c)
    for _ in range(2):
        _period(c)
    c.clear_observation()
    st0, _ = _accumulators(c)
    done = np.zeros(B, dtype=np.uint8)
    c.end_episodes(done, extra)
    st1, ep1 = _accumulators(c)
    on = extra != 0
    assert np.array_equal(st1[2, on], st0[0, on]) and (st1[0, on] == 0).all() and (st1[1, on] == 1).all() and (ep1[0, on] == 0).all() and (ep1[1, on] == 0).all()
    assert np.array_equal(st1[:, ~on], st0[:, ~on])
    # argument checks
    for bad in (0, 1, 32, 63, 65, 192, 256):
        with pytest.raises(ValueError, match="bit"):
            c.end_episodes(done, extra, bad)
    with pytest.raises(ValueError):
        c.end_episodes(done[:-1], extra)
    assert c.lib.sai2b_end_episodes(c.h, None, extra.ctypes.data, 64, 0) == _abi.INVALID_ARGUMENT
    assert c.lib.sai2b_end_episodes(c.h, done.ctypes.data, None, 64, 0) == _abi.INVALID_ARGUMENT


def test_resident_loop_with_torch_equals_the_loop_through_numpy():
    import torch

    cell = cc.LOOP_CELL
    case = cc.draw(cell)
    B, n = case["B"], case["n"]
    rng = np.random.default_rng(11)
    dq = rng.normal(0, 0.3, (n, B))

    def make():
        cfgs = [pkg.motion_force_task_config("m", link=n - 1, frame_pos=(0.01, 0.02, 0.06), robot_dof=n), pkg.joint_task_config("j", robot_dof=n)]
        c = pkg.Controller(case["model"], cfgs, B)
        c.set_state(case["q"], dq)
        c.set_observation(blocks=("q", "dq", "episode_step"), max_episode_steps=4, max_joint_speed=1.0, nonfinite=True)
        c.set_reward(terms=dict(alive=1.0, joint_speed=-0.01, torque_rate=-0.01), gamma=0.98)
        c.set_collision(c.collision_config(case["idx"], case["cen"], case["rad"], n_planes=1, n_obstacles=2, blocks=("distance", "gradient"),
                                           margin_plane=MARGINS[0], margin_obstacle=MARGINS[1], margin_self=MARGINS[2], pairs=PAIRS), case["env"])
        c.set_reset_sampler(seed=5)
        return c

    dev, host = make(), make()
    seen = []
    with torch.cuda.stream(torch.cuda.Stream()):
        out_d = torch.zeros((dev.observation_rows(), B), dtype=torch.float64, device="cuda")
        done_d = torch.zeros(B, dtype=torch.uint8, device="cuda")
        rew_d = torch.zeros(B, dtype=torch.float64, device="cuda")
        col_d = torch.zeros((dev.collision_rows(), B), dtype=torch.float64, device="cuda")
        flags_d = torch.zeros(B, dtype=torch.uint8, device="cuda")
        for _ in range(10):  # nothing in this loop touches the host
            dev.tick(want_output=False)
            dev.sim_step(None)
            dev.observe_reward(out=out_d, done=done_d, reward=rew_d, terms=False)
            dev.collision_query(col_d, flags_d)
            dev.end_episodes(done_d, flags_d)
            dev.reset_robots_sampled(done_d)
            seen.append([x.clone() for x in (out_d, done_d, rew_d, col_d, flags_d)])
        dev.synchronize()
        torch.cuda.current_stream().synchronize()
    ended = collided = 0
    for k in range(10):
        host.tick(want_output=False)
        host.sim_step(None)
        obs, done, rew, _ = host.observe_reward(terms=False)
        col, flags = host.collision_query()
        host.end_episodes(done, flags)
        host.reset_robots_sampled(done)
        for x, y in zip(seen[k], (obs, done, rew, col, flags)):
            assert np.array_equal(x.cpu().numpy(), y), k
        ended += int((done != 0).sum())
        collided += int(((done & 64) != 0).sum())
    assert 0 < collided < ended < 10 * B  # some episodes ended by a collision, some by a built-in criterion alone
    sd, sh = dev.episode_stats(), host.episode_stats()
    assert all(np.array_equal(sd[k], sh[k]) for k in sd)
    assert all(np.array_equal(x, y) for x, y in zip(dev.get_state(), host.get_state()))
