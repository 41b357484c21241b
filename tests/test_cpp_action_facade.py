"""The action members of the C++ facade (include/Sai2PrimitivesBatched.h: setAction, clearAction, actionRows, actionLayout,
applyAction, actionCounts), compiled with g++ against the C ABI the way tests/test_cpp_observation_facade.py builds its
program (tests/cpp/action_facade_test.cpp): the device-free argument checks; on the GPU ShardedRobotController::applyAction
on 257 robots over two uneven shards with a mask straddling the boundary, bit-equal to one context; and
sharding.apply_action on the same split."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def action_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "action_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "action_facade_test.cpp"),
         "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_action_members_compile_and_reject_bad_arguments(action_bin):
    r = subprocess.run([action_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 11


@pytest.mark.gpu
def test_cpp_sharded_apply_action_equals_one_context(action_bin):
    r = subprocess.run([action_bin, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and "FAIL" not in r.stdout and r.stdout.count("ok ") == 19


@pytest.mark.gpu
def test_python_sharded_apply_action_equals_one_context():
    import sai2_primitives_perso_amd as pkg
    from sai2_primitives_perso_amd import sharding
    from sai2_primitives_perso_amd import workloads as wl
    from test_gpu_action import read_goals

    B, world = 257, 2
    inp = wl.make_inputs(3, B=B, seed=91)
    act = dict(tasks={0: dict(mode="delta_current", blocks=("position", "orientation", "force"), pos_scale=0.05, ori_scale=0.3, force_scale=9.0,
                              max_pos_lead=0.04), 1: dict(mode="delta_goal", jt_scale=0.1, jt_limits="model")}, clip_actions=True)
    rng = np.random.default_rng(4)
    action = rng.uniform(-1.4, 1.4, (16, B))
    action[3, 7], action[9, 200] = np.nan, -np.inf
    mask = rng.uniform(size=B) < 0.8

    def controller(lo, hi):
        g = pkg.Controller(pkg.panda_model(), pkg.task_configs(inp["tasks"]), hi - lo)
        g.set_state(np.ascontiguousarray(inp["q"][:, lo:hi]), np.ascontiguousarray(inp["dq"][:, lo:hi]))
        g.set_mft_goals(0, *[np.ascontiguousarray(inp["mft0"][k][:, lo:hi]) for k in ("pos", "rot", "v", "w", "a", "alpha")])
        g.set_jt_goals(1, *[np.ascontiguousarray(inp["jt1"][k][:, lo:hi]) for k in ("q", "dq", "ddq")])
        g.set_action(**act)
        return g

    one = controller(0, B)
    one.apply_action(action, mask)
    whole, counts = read_goals(one), one.action_counts()
    assert counts["rejected"] == int(mask[7]) + int(mask[200]) and counts["clipped"] > 0
    total = dict.fromkeys(counts, 0)
    bounds = [sharding.shard_bounds(B, world, r) for r in range(world)]
    assert bounds[0][1] - bounds[0][0] != bounds[1][1] - bounds[1][0]
    for rank, (lo, hi) in enumerate(bounds):
        g = controller(lo, hi)
        sharding.apply_action(g, world, rank, action, mask)
        for a, b in zip(read_goals(g), whole):
            assert np.array_equal(a, b[:, lo:hi]), rank
        for k, v in g.action_counts().items():
            total[k] += v
    assert total == counts
