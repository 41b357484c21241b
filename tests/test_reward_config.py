"""CPU-only: the host-only entry points of the reward feature (sai2b_default_reward, sai2b_validate_reward,
sai2b_sizeof_reward_config, sai2b_reward_config_layout) through ctypes: the defaults, every rejection include/sai2b.h lists
for the configuration, the layout arithmetic, and the size of the ctypes mirror. Without a GPU there is no context, so "no
reward without an observation" is checked here as far as the host goes (a NULL context) and on a context in
tests/test_gpu_reward.py."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS, TASK_TERMS = list(_abi.REW_TERMS.values()), list(_abi.REW_TASK_TERMS.values())


def _lib():
    return _abi.load_library()


def _default():
    cfg = _abi.RewardConfig()
    assert _lib().sai2b_default_reward(C.byref(cfg)) == _abi.OK
    return cfg


def _tasks(dof=7):
    """[MotionForceTask, JointTask, MotionForceTask]: tasks 0 and 2 are MotionForceTasks"""
    return [pkg.motion_force_task_config("m", robot_dof=dof, link=dof - 1), pkg.joint_task_config("j", robot_dof=dof),
            pkg.motion_force_task_config("n", robot_dof=dof, link=dof - 2)]


def _validate(cfg, tasks, dof=7):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_reward(None if cfg is None else C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def _layout(cfg, term, task=-1):
    first, n, total = C.c_int(), C.c_int(), C.c_int()
    rc = _lib().sai2b_reward_config_layout(C.byref(cfg), term, task, C.byref(first), C.byref(n), C.byref(total))
    return rc, first.value, n.value, total.value


def test_size_of_the_mirror_is_the_librarys():
    assert _lib().sai2b_sizeof_reward_config() == C.sizeof(_abi.RewardConfig)
    fields = ("weight", "task_weight", "done_value", "limit_soft_margin", "pos_scale", "force_soft_limit", "gamma", "nonfinite_reward")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sai2b.h"\nint main(){printf("%zu", sizeof(sai2b_reward_config));\n'
           + "".join(f'printf(" %zu", offsetof(sai2b_reward_config, {f}));\n' for f in fields) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")], check=True)
        out = subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(_abi.RewardConfig)] + [getattr(_abi.RewardConfig, f).offset for f in fields]


def test_flag_values_match_the_header():
    header = open(os.path.join(ROOT, "include", "sai2b.h")).read()
    for table in (_abi.REW_TERMS, _abi.REW_TASK_TERMS):
        for name, value in table.items():
            m = re.search("SAI2B_REW_" + name.upper() + r"\s*=\s*(\d+)", header)
            assert m and int(m.group(1)) == value, name
        assert list(table.values()) == [1 << k for k in range(len(table))]
    assert (_abi.REWARD_TERMS, _abi.REWARD_TASK_TERMS) == (len(_abi.REW_TERMS), len(_abi.REW_TASK_TERMS)) == (6, 10)
    assert re.search(r"SAI2B_BUF_REWARD_STATE = 18", header) and re.search(r"SAI2B_BUF_REWARD_EPISODE = 19", header)
    assert (_abi.BUF_REWARD_STATE, _abi.BUF_REWARD_EPISODE) == (18, 19)


def test_default_selects_nothing_and_is_rejected_for_that_alone():
    cfg = _default()
    d = _abi.struct_to_dict(cfg)
    assert (d["terms"], d["task_mask"], d["task_terms"], d["gamma"], d["nonfinite_reward"], d["limit_soft_margin"]) == (0, 0, 0, 1.0, 0.0, 0.0)
    assert d["pos_scale"] == [1.0] * 4 and d["ori_scale"] == [1.0] * 4 and d["force_soft_limit"] == [0.0] * 4
    assert not any(cfg.weight) and not any(w for row in cfg.task_weight for w in row) and not any(cfg.done_value)
    assert _validate(cfg, _tasks()) == (_abi.INVALID_ARGUMENT, "reward: no term is selected")
    cfg.terms = _abi.REW_TERMS["alive"]
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    assert _validate(cfg, [pkg.joint_task_config("j")]) == (_abi.OK, "")  # global terms need no MotionForceTask


def _set(name, value):
    return lambda c: setattr(c, name, value)


def _item(name, index, value):
    return lambda c: getattr(c, name).__setitem__(index, value)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("edit, message", [
    (_set("terms", 64), "reward: unknown bits in terms"),
    (_set("terms", -1), "reward: unknown bits in terms"),
    (_set("task_terms", 1024), "reward: unknown bits in task_terms"),
    (_set("task_mask", 2), "reward: task_mask selects a task that is not a MotionForceTask"),  # the JointTask
    (_set("task_mask", 8), "reward: task_mask selects a task that is not a MotionForceTask"),  # past the tasks
    (_set("task_mask", 1 << 5), "reward: task_mask selects a task that is not a MotionForceTask"),
    (_set("task_mask", 0), "reward: task_terms needs a task in task_mask"),
    (_set("task_terms", 0), "reward: task_mask needs a term in task_terms"),
    (_item("weight", 3, NAN), "reward: weights must be finite"),
    (_item("weight", 0, INF), "reward: weights must be finite"),
    (lambda c: c.task_weight[2].__setitem__(9, -INF), "reward: weights must be finite"),
    (lambda c: c.task_weight[1].__setitem__(0, NAN), "reward: weights must be finite"),  # also for a task that is not selected
    (_item("done_value", 5, NAN), "reward: done_value must be finite"),
    (_item("pos_scale", 0, INF), "reward: scales must be finite"),
    (_item("ori_scale", 3, NAN), "reward: scales must be finite"),
    (_item("pos_scale", 0, 0.0), "reward: POS_TANH needs pos_scale > 0"),
    (_item("pos_scale", 2, -1.0), "reward: POS_TANH needs pos_scale > 0"),
    (_item("ori_scale", 2, 0.0), "reward: ORI_TANH needs ori_scale > 0"),
    (_item("force_soft_limit", 0, -1e-3), "reward: force_soft_limit must be finite and >= 0"),
    (_item("force_soft_limit", 3, INF), "reward: force_soft_limit must be finite and >= 0"),
    (_set("limit_soft_margin", -0.1), "reward: limit_soft_margin must be finite and >= 0"),
    (_set("limit_soft_margin", NAN), "reward: limit_soft_margin must be finite and >= 0"),
    (_set("gamma", -1e-9), "reward: gamma must be in [0, 1]"),
    (_set("gamma", 1.0 + 1e-9), "reward: gamma must be in [0, 1]"),
    (_set("gamma", NAN), "reward: gamma must be in [0, 1]"),
    (_set("nonfinite_reward", INF), "reward: nonfinite_reward must be finite"),
    (lambda c: (setattr(c, "terms", 0), setattr(c, "task_terms", 0), setattr(c, "task_mask", 0)), "reward: no term is selected"),
])
def test_validate_rejects(edit, message):
    cfg = _default()
    cfg.terms, cfg.task_mask, cfg.task_terms = 63, 0b101, 1023
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    edit(cfg)
    rc, msg = _validate(cfg, _tasks())
    assert rc == _abi.INVALID_ARGUMENT and msg == message
    assert _lib().sai2b_last_error(None).decode() == message


def test_validate_accepts_the_edges_and_routes_by_robot_size():
    cfg = _default()
    cfg.terms, cfg.task_mask, cfg.task_terms = 63, 0b101, 1023
    cfg.gamma = 0.0
    assert _validate(cfg, _tasks())[0] == _abi.OK
    cfg.gamma = 1.0
    cfg.pos_scale[1] = cfg.ori_scale[1] = 0.0  # task 1 is not selected: its scales are not divided by
    assert _validate(cfg, _tasks())[0] == _abi.OK
    cfg.task_terms = 1023 & ~(_abi.REW_TASK_TERMS["pos_tanh"] | _abi.REW_TASK_TERMS["ori_tanh"])
    cfg.pos_scale[0] = cfg.ori_scale[2] = 0.0  # no TANH term: no scale is divided by
    assert _validate(cfg, _tasks())[0] == _abi.OK
    for dof in (4, 6, 8):
        assert _validate(cfg, _tasks(dof), dof=dof) == (_abi.OK, "")
    assert _validate(cfg, _tasks(), dof=5)[0] == _abi.UNSUPPORTED  # no build for a 5-joint robot
    assert _validate(None, _tasks())[0] == _abi.INVALID_ARGUMENT


def test_layout_every_single_term():
    for k, flag in enumerate(TERMS):
        cfg = _default()
        cfg.terms = flag
        for other in TERMS:
            assert _layout(cfg, other) == ((_abi.OK, 0, 1, 1) if other == flag else (_abi.OK, -1, 0, 1))
        assert _layout(cfg, 1, 0) == (_abi.OK, -1, 0, 1)
    for flag in TASK_TERMS:
        cfg = _default()
        cfg.task_mask, cfg.task_terms = 0b100, flag
        for other in TASK_TERMS:
            assert _layout(cfg, other, 2) == ((_abi.OK, 0, 1, 1) if other == flag else (_abi.OK, -1, 0, 1))
            assert _layout(cfg, other, 0) == (_abi.OK, -1, 0, 1)


def test_layout_all_terms_and_two_tasks():
    cfg = _default()
    cfg.terms, cfg.task_mask, cfg.task_terms = 63, 0b101, 1023
    total = 6 + 2 * 10
    for k, flag in enumerate(TERMS):
        assert _layout(cfg, flag) == (_abi.OK, k, 1, total)
    for k, flag in enumerate(TASK_TERMS):
        assert _layout(cfg, flag, 0) == (_abi.OK, 6 + k, 1, total)
        assert _layout(cfg, flag, 2) == (_abi.OK, 16 + k, 1, total)
        assert _layout(cfg, flag, 1) == (_abi.OK, -1, 0, total)
    # a sparse selection: TORQUE, DONE; tasks 0 and 2 with POS_SQ, ANG_VEL_SQ, FORCE_EXCESS
    cfg.terms = _abi.REW_TERMS["torque"] | _abi.REW_TERMS["done"]
    cfg.task_terms = _abi.REW_TASK_TERMS["pos_sq"] | _abi.REW_TASK_TERMS["ang_vel_sq"] | _abi.REW_TASK_TERMS["force_excess"]
    total = 2 + 2 * 3
    assert _layout(cfg, _abi.REW_TERMS["alive"]) == (_abi.OK, -1, 0, total)
    assert _layout(cfg, _abi.REW_TERMS["torque"]) == (_abi.OK, 0, 1, total) and _layout(cfg, _abi.REW_TERMS["done"]) == (_abi.OK, 1, 1, total)
    for t, base in ((0, 2), (2, 5)):
        assert _layout(cfg, _abi.REW_TASK_TERMS["pos_sq"], t) == (_abi.OK, base, 1, total)
        assert _layout(cfg, _abi.REW_TASK_TERMS["ang_vel_sq"], t) == (_abi.OK, base + 1, 1, total)
        assert _layout(cfg, _abi.REW_TASK_TERMS["force_excess"], t) == (_abi.OK, base + 2, 1, total)
        assert _layout(cfg, _abi.REW_TASK_TERMS["pos"], t) == (_abi.OK, -1, 0, total)
    # tasks without task terms, and the reverse: no task rows
    cfg.terms, cfg.task_mask, cfg.task_terms = 1, 0b11, 0
    assert _layout(cfg, 1, 0) == (_abi.OK, -1, 0, 1)
    cfg.task_mask, cfg.task_terms = 0, 1023
    assert _layout(cfg, 1, 0) == (_abi.OK, -1, 0, 1)


def test_layout_rejects_bad_queries():
    cfg = _default()
    cfg.terms = 63
    for term, task in ((0, -1), (3, -1), (64, -1), (1024, 0), (1, -2), (1, 4)):
        assert _layout(cfg, term, task)[0] == _abi.INVALID_ARGUMENT, (term, task)


def test_without_a_context_nothing_is_set():
    lib = _lib()
    cfg = _default()
    cfg.terms = 1
    assert lib.sai2b_set_reward(None, C.byref(cfg)) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_clear_reward(None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_observe_reward(None, None, None, None, None, 0) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_reward_counts(None, (C.c_int * 2)()) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_episode_stats(None, None, None, None, None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_reward_layout(None, 1, -1, None, None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_reward_rows(None) == -1


def test_set_reward_without_an_observation_fails_in_the_source():
    """sai2b_set_reward refuses a context without an observation before it allocates anything (the call itself needs a GPU:
    tests/test_gpu_reward.py::test_routing makes it)"""
    src = open(os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc", "sai2b_host.cpp")).read()
    body = src[src.index('extern "C" int sai2b_set_reward('):]
    body = body[:body.index("\n}\n")]
    assert body.index("!ctx->obs_on") < body.index("dev_alloc") and "no observation is configured" in body
