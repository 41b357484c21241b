"""GPU tests (-m gpu) of the collision proximity (csrc/sai2b_collision.hip: collision_kernel; include/sai2b.h "collision
proximity") against tests/collision_reference.py (numpy on the independent URDF chain) and against twin contexts. Small shapes.

1: the law: planar_4r, six_r, Panda and sliding_base (prismatic joint 0) at B = 1, 63, 64, 65, 200 and one Panda cell at 4 099
   (tests/collision_cases.py: one sphere on the last link, 12 over the arm, 16 over world, inner and last links; a pitched base;
   0 / 1 / 2 planes; 0 / 1 / 4 obstacles; pair mask empty / default / all; a NaN plane on every third robot; q that is not finite).
   Distances, normals, gradients and centres within 1e-12, indices, flags and the device counts exact.
   tests/test_collision_reference.py asserts on the CPU that every robot of every cell is well separated, so none is left out.
2: every block subset stores exactly its rows, guard rows around the output and guard bytes around the flags untouched.
3: view: with a joint sensor carrying a calibration offset, view = 1 is the reference at the measured q, view = 0 at the true q.
4: a configured but unqueried context, and a cleared one, run tick, sim_step and observe_reward bit-equal to a twin that never set
   the feature, over six periods.
5: rows written through SAI2B_BUF_COLLISION by a torch op are what the next query reads. 6: two shards are bit-equal to one
   context of 200. 7: argument checks leave the context as it was; no launch without a configuration."""
import itertools

import numpy as np
import pytest

import collision_cases as cc
import joint_sensor_reference as jr
import sai2_primitives_perso_amd as pkg
import test_gpu_subset_reset as sr
from sai2_primitives_perso_amd import _abi, sharding

pytestmark = pytest.mark.gpu

TOL = 1e-12
ALL = ("distance", "index", "normal", "gradient", "centres")


def _controller(case, B=None):
    n = case["n"]
    cfgs = [pkg.motion_force_task_config("m", link=n - 1, frame_pos=(0.01, 0.02, 0.06), robot_dof=n), pkg.joint_task_config("j", robot_dof=n)]
    return pkg.Controller(case["model"], cfgs, case["B"] if B is None else B)


def _config(c, case, cell, blocks=ALL, view="truth"):
    return c.collision_config(case["idx"], case["cen"], case["rad"], n_planes=case["P"], n_obstacles=case["O"], blocks=blocks,
                              margin_plane=cc.MARGINS[0], margin_obstacle=cc.MARGINS[1], margin_self=cc.MARGINS[2], view=view, pairs=cell[5])


def _compare(out, flags, ev, ref, what):
    """the device's rows and flags against the reference's; a robot whose q is not finite: the flags alone"""
    assert np.array_equal(flags, ev["flags"]), what
    ok = ev["flags"] != 8
    want = ref.output_rows(ev, ALL)
    n3 = 3
    assert np.array_equal(out[n3 : 2 * n3, ok], want[n3 : 2 * n3, ok]), (what, "index")
    a, r = out[:, ok], want[:, ok]
    assert np.array_equal(np.isinf(a), np.isinf(r)) and not np.isnan(a).any(), what
    fin = np.isfinite(r)
    err = np.abs(a[fin] - r[fin]).max(initial=0.0)
    assert err < TOL, (what, err)
    return err


# ---------------------------------------------------------------------------------------------- 1: the law
def test_the_cells_cover_what_the_issue_lists():
    assert {c[0] for c in cc.CELLS} == set(cc.ROBOTS) and {c[1] for c in cc.CELLS} == {1, 63, 64, 65, 200, 4099}
    assert {c[2] for c in cc.CELLS} == {"last", "arm", "full16"} and {c[3] for c in cc.CELLS} == {0, 1, 2} and {c[4] for c in cc.CELLS} >= {0, 1, 4}
    assert {c[5] for c in cc.CELLS} == {"none", "default", "all"} and any(c[6] for c in cc.CELLS) and any(c[7] for c in cc.CELLS) and any(c[8] for c in cc.CELLS)
    for robot in cc.ROBOTS:
        assert {c[1] for c in cc.CELLS if c[0] == robot} >= set(cc.BATCHES)


@pytest.mark.parametrize("cell", cc.CELLS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-P{c[3]}-O{c[4]}-{c[5]}")
def test_the_law(cell):
    case, ev = cc.evaluated(cell)
    g = _controller(case)
    g.set_state(case["q"], np.zeros_like(case["q"]))
    g.set_collision(_config(g, case, cell), case["env"])
    out, flags = g.collision_query()
    err = _compare(out, flags, ev, case["reference"], cell)
    counts = g.collision_counts()
    assert [counts[k] for k in ("plane", "obstacle", "self", "nonfinite", "any")] == ev["counts"], cell
    print(f"{cell[:6]}: worst {err:.2e}, counts {ev['counts']}")
    # the flags alone, and the rows alone, are the same launch with one output less
    _, f2 = g.collision_query(out=False)
    o2, _ = g.collision_query(flags=False)
    assert np.array_equal(f2, flags) and np.array_equal(o2, out, equal_nan=True)
    cfg, rows = g.get_collision()
    assert cfg.n_spheres == len(case["idx"]) and (case["env"] is None or np.array_equal(rows, case["env"], equal_nan=True))


def test_every_flag_bit_and_the_empty_category_occur_in_the_cells():
    seen, empty = set(), 0
    for cell in cc.CELLS:
        _, ev = cc.evaluated(cell)
        seen |= set(ev["flags"].tolist())
        empty += int((ev["index"] < 0).sum())
    assert {1, 2, 4, 8} <= {b for f in seen for b in (1, 2, 4, 8) if f & b} and 0 in seen and empty > 0


# ---------------------------------------------------------------------------------------------- 2: block subsets
SUBSET_CELL = cc.SUBSET_CELL


def test_every_block_subset_stores_exactly_its_rows():
    import torch

    case, ev = cc.evaluated(SUBSET_CELL)
    B, n, S = case["B"], case["n"], len(case["idx"])
    g = _controller(case)
    g.set_state(case["q"], np.zeros_like(case["q"]))
    sizes = dict(distance=3, index=3, normal=9, gradient=3 * n, centres=3 * S)
    for k in range(len(ALL) + 1):
        for blocks in itertools.combinations(ALL, k):
            g.set_collision(_config(g, case, SUBSET_CELL, blocks), case["env"])
            rows = sum(sizes[b] for b in blocks)
            assert g.collision_rows() == rows
            lay = g.collision_layout()
            assert set(lay) & set(ALL) == set(blocks)
            buf = torch.full((rows + 2, B), -7.25, dtype=torch.float64, device="cuda")
            fbuf = torch.full((B + 128,), 0xA5, dtype=torch.uint8, device="cuda")
            out, flags = buf[1 : 1 + rows], fbuf[64 : 64 + B]
            g.collision_query(out if rows else False, flags)
            g.synchronize()
            h, fh = buf.cpu().numpy(), fbuf.cpu().numpy()
            assert (h[0] == -7.25).all() and (h[-1] == -7.25).all() and (fh[:64] == 0xA5).all() and (fh[64 + B :] == 0xA5).all(), blocks
            assert np.array_equal(fh[64 : 64 + B], ev["flags"]), blocks
            want = case["reference"].output_rows(ev, blocks) if rows else np.zeros((0, B))
            got = h[1 : 1 + rows]
            assert not (got == -7.25).any(), blocks
            fin = np.isfinite(want)
            assert np.array_equal(np.isinf(got), np.isinf(want)) and np.abs(got[fin] - want[fin]).max(initial=0.0) < TOL, blocks
            first = 0
            for b in blocks:  # the layout names the rows of every block and of its categories
                assert lay[b] == slice(first, first + sizes[b]), (blocks, b)
                if b != "centres":
                    per = sizes[b] // 3
                    assert [lay[f"{b}_{c}"] for c in _abi.COL_CATEGORIES] == [slice(first + per * c, first + per * (c + 1)) for c in range(3)]
                first += sizes[b]


# ---------------------------------------------------------------------------------------------- 3: view
def test_view_selects_the_measured_or_the_true_q():
    cell = cc.VIEW_CELL
    case = cc.draw(cell)
    n, B = case["n"], case["B"]
    g = _controller(case)
    g.set_state(case["q"], np.zeros_like(case["q"]))
    rows = jr.ideal_rows(n, B)
    rows[1 : 1 + n] = np.random.default_rng(3).uniform(-0.05, 0.05, (n, B))
    g.set_joint_sensor(rows)
    qm, _ = g.get_measured_state()
    assert np.abs(qm - case["q"]).max() > 0.01
    ref = case["reference"]
    for view, q in (("measured", qm), ("truth", case["q"])):
        g.set_collision(_config(g, case, cell, view=view), case["env"])
        out, flags = g.collision_query()
        ev = ref.evaluate(q, case["env"])
        assert (ev["gap"] > 1e-9).all() and (ev["norm"] > 1e-3).all() and (np.abs(ev["distance"] - np.array(cc.MARGINS)[:, None]) > 1e-9).all()
        _compare(out, flags, ev, ref, view)
    # without a joint sensor view = 1 reads the truth
    g.clear_joint_sensor()
    g.set_collision(_config(g, case, cell, view="measured"), case["env"])
    assert np.array_equal(g.collision_query()[0], out, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 4: nothing else changes
def _equip(c, s):
    t = s.kinds.index("mft")
    c.set_observation(blocks=("q", "dq", "tau", "limit_margin", "episode_step"), tasks=[t], task_blocks=("pose", "twist", "error"), joint_limit_margin=0.02,
                      max_joint_speed=0.8, nonfinite=True, max_episode_steps=4)
    c.set_reward(terms=dict(alive=1.0, joint_speed=-0.01, torque=-0.001, torque_rate=-0.001))


def _periods(c, s, k):
    out = []
    for _ in range(k):
        tau = c.tick()
        c.sim_step(None)
        obs, done, rew, _ = c.observe_reward(terms=False)
        out.append([tau, *c.get_state(), obs, done, rew] + sr.snapshot(c, s.kinds))
    return out


def test_a_configured_or_cleared_context_runs_bit_equal_to_a_twin(monkeypatch):
    s = sr.scenario("c3")
    a, b, twin = sr.contexts(s, 3, monkeypatch)
    cell = cc.TWIN_CELL
    assert cell[1] == sr.B
    case = cc.draw(cell)
    for c in (a, b, twin):
        _equip(c, s)
    launches = a.counters()[0]
    for c in (a, b):
        c.set_collision(_config(c, case, cell), case["env"])
    assert a.counters()[0] == launches  # configuring launches nothing
    b.collision_query()
    b.clear_collision()
    assert b.collision_rows() == -1 and b.device_buffer(_abi.BUF_COLLISION) is None and a.device_buffer(_abi.BUF_COLLISION) is not None
    every = np.ones(sr.B, dtype=bool)
    ra, rb, rt = (_periods(c, s, 6) for c in (a, b, twin))
    for k in range(6):
        sr.assert_columns(ra[k], rt[k], every, f"configured, period {k}")
        sr.assert_columns(rb[k], rt[k], every, f"cleared, period {k}")


# ---------------------------------------------------------------------------------------------- 5: device rows
def test_rows_written_by_a_torch_op_are_what_the_next_query_reads():
    import torch

    cell = cc.TORCH_CELL
    case = cc.draw(cell)
    P = case["P"]
    g = _controller(case)
    g.set_state(case["q"], np.zeros_like(case["q"]))
    g.set_collision(_config(g, case, cell), torch.from_numpy(case["env"]).cuda())  # device rows are copied as they are
    assert np.array_equal(g.get_collision()[1], case["env"])
    ref = case["reference"]
    _compare(*g.collision_query(), ref.evaluate(case["q"], case["env"]), ref, "device rows")
    g.synchronize()
    env = g.collision_env()
    env[6 * P : 6 * P + 3] += 0.07  # the first obstacle moves
    env[6 * P + 4 : 6 * P + 8, ::4] = float("nan")  # the second disappears for every fourth robot
    torch.cuda.synchronize()
    moved = case["env"].copy()
    moved[6 * P : 6 * P + 3] += 0.07
    moved[6 * P + 4 : 6 * P + 8, ::4] = np.nan
    ev = ref.evaluate(case["q"], moved)
    assert (ev["gap"] > 1e-9).all() and (ev["norm"] > 1e-3).all() and (np.abs(ev["distance"] - np.array(cc.MARGINS)[:, None]) > 1e-9).all()
    _compare(*g.collision_query(), ev, ref, "rows rewritten")
    assert not np.array_equal(ev["distance"], ref.evaluate(case["q"], case["env"])["distance"])


# ---------------------------------------------------------------------------------------------- 6: shards
def test_two_shards_are_bit_equal_to_one_context():
    cell = cc.SHARD_CELL
    case = cc.draw(cell)
    B = case["B"]
    one = _controller(case)
    one.set_state(case["q"], np.zeros_like(case["q"]))
    one.set_collision(_config(one, case, cell), case["env"])
    out, flags = one.collision_query()
    total = np.zeros(5, dtype=int)
    for rank in range(2):
        lo, hi = sharding.shard_bounds(B, 2, rank)
        c = _controller(case, hi - lo)
        c.set_state(np.ascontiguousarray(case["q"][:, lo:hi]), np.zeros((case["n"], hi - lo)))
        sharding.set_collision(c, 2, rank, B, _config(c, case, cell), case["env"])
        o, f = c.collision_query()
        assert np.array_equal(o, out[:, lo:hi], equal_nan=True) and np.array_equal(f, flags[lo:hi]), rank
        total += np.array(list(c.collision_counts().values()))
    assert total.tolist() == list(one.collision_counts().values())


# ---------------------------------------------------------------------------------------------- 7: argument checks
def test_argument_checks_leave_the_context_as_it_was():
    cell = cc.ARG_CELL
    case = cc.draw(cell)
    g = _controller(case)
    g.set_state(case["q"], np.zeros_like(case["q"]))
    launches = g.counters()[0]
    for call in (g.collision_query, g.collision_counts, g.get_collision, g.collision_layout):
        with pytest.raises(ValueError):
            call()
    assert g.collision_rows() == -1 and g.device_buffer(_abi.BUF_COLLISION) is None and g.counters()[0] == launches
    cfg = _config(g, case, cell)
    g.set_collision(cfg, case["env"])
    out, flags = g.collision_query()
    bad = case["env"].copy()
    bad[3:6, 5] *= 1.001  # a normal that is not a unit vector
    with pytest.raises(ValueError, match="unit length"):
        g.set_collision(cfg, bad)
    bad = case["env"].copy()
    bad[12 + 3, 7] = -0.1  # a negative obstacle radius
    with pytest.raises(ValueError, match="radius"):
        g.set_collision(cfg, bad)
    worse = _config(g, case, cell)
    worse.link[2] = 7
    with pytest.raises(ValueError, match="link"):
        g.set_collision(worse, case["env"])
    o2, f2 = g.collision_query()
    assert np.array_equal(o2, out, equal_nan=True) and np.array_equal(f2, flags) and np.array_equal(g.get_collision()[1], case["env"])
    # no rows: everything absent until a producer writes them
    g.set_collision(cfg, None)
    o3, f3 = g.collision_query()
    lay = g.collision_layout()
    assert np.isinf(o3[lay["distance_plane"]]).all() and np.isinf(o3[lay["distance_obstacle"]]).all() and (o3[lay["index_plane"]] == -1).all()
    assert not (f3 & 3).any() and not o3[lay["normal_plane"]].any() and not o3[lay["gradient_obstacle"]].any()
    assert np.array_equal(o3[lay["distance_self"]], out[lay["distance_self"]])
