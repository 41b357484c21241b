"""CPU-only: the host-only entry points of the observation feature (sai2b_default_observation, sai2b_validate_observation,
sai2b_sizeof_observation_config, sai2b_observation_config_layout) through ctypes: the defaults, every rejection
include/sai2b.h lists for the configuration, the layout arithmetic, and the size of the ctypes mirror."""
import ctypes as C
import os
import subprocess

import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    return _abi.load_library()


def _default():
    cfg = _abi.ObservationConfig()
    assert _lib().sai2b_default_observation(C.byref(cfg)) == _abi.OK
    return cfg


def _tasks(dof=7):
    """[MotionForceTask, JointTask]: task 0 is the only MotionForceTask"""
    return [pkg.motion_force_task_config("m", robot_dof=dof, link=dof - 1), pkg.joint_task_config("j", robot_dof=dof)]


def _validate(cfg, tasks, dof=7):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_observation(None if cfg is None else C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def _layout(cfg, block, task=-1, dof=7):
    first, n, total = C.c_int(), C.c_int(), C.c_int()
    rc = _lib().sai2b_observation_config_layout(C.byref(cfg), dof, block, task, C.byref(first), C.byref(n), C.byref(total))
    return rc, first.value, n.value, total.value


def test_size_of_the_mirror_is_the_librarys():
    assert _lib().sai2b_sizeof_observation_config() == C.sizeof(_abi.ObservationConfig)
    # and the C compiler's, from the header
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sai2b.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(sai2b_observation_config), offsetof(sai2b_observation_config, pos_tolerance), offsetof(sai2b_observation_config, max_sensed_force));return 0;}\n'
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")], check=True)
        out = subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(_abi.ObservationConfig), _abi.ObservationConfig.pos_tolerance.offset,
                                     _abi.ObservationConfig.max_sensed_force.offset]


def test_flag_values_match_the_header():
    header = open(os.path.join(ROOT, "include", "sai2b.h")).read()
    import re

    for prefix, table in (("SAI2B_OBS_", {**_abi.OBS_BLOCKS, **_abi.OBS_TASK_BLOCKS}), ("SAI2B_DONE_", _abi.DONE_BITS)):
        for name, value in table.items():
            m = re.search(prefix + name.upper() + r"\s*=\s*(\d+)", header)
            assert m and int(m.group(1)) == value, name
    assert _abi.DONE_REASONS == 6 and list(_abi.DONE_BITS.values()) == [1 << k for k in range(6)]


def test_default_is_valid_and_empty():
    cfg = _default()
    d = _abi.struct_to_dict(cfg)
    assert all(v == 0 for k, v in d.items() if not isinstance(v, list)) and all(x == 0 for x in d["max_joint_speed"])
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    assert _layout(cfg, _abi.OBS_Q) == (_abi.OK, -1, 0, 0)
    assert _validate(cfg, [pkg.joint_task_config("j")]) == (_abi.OK, "")  # nothing observed: no MotionForceTask needed


def _set(name, value):
    return lambda c: setattr(c, name, value)


@pytest.mark.parametrize("edit, message", [
    (_set("blocks", 64), "observation: unknown bits in blocks"),
    (_set("blocks", -1), "observation: unknown bits in blocks"),
    (_set("task_blocks", 16), "observation: unknown bits in task_blocks"),
    (_set("criteria", 64), "observation: unknown bits in criteria"),
    (_set("task_mask", 2), "observation: task_mask selects a task that is not a MotionForceTask"),  # the JointTask
    (_set("task_mask", 4), "observation: task_mask selects a task that is not a MotionForceTask"),  # past the tasks
    (_set("task_mask", 1 << 5), "observation: task_mask selects a task that is not a MotionForceTask"),
    (_set("success_task_mask", 3), "observation: success_task_mask selects a task that is not a MotionForceTask"),
    (_set("force_task_mask", 2), "observation: force_task_mask selects a task that is not a MotionForceTask"),
    (_set("pos_tolerance", -1e-3), "observation: thresholds must be finite and >= 0"),
    (_set("ori_tolerance", float("nan")), "observation: thresholds must be finite and >= 0"),
    (_set("joint_limit_margin", float("inf")), "observation: thresholds must be finite and >= 0"),
    (_set("max_sensed_force", -1.0), "observation: thresholds must be finite and >= 0"),
    (lambda c: c.max_joint_speed.__setitem__(6, -0.1), "observation: max_joint_speed must be finite and >= 0"),
    (lambda c: c.max_joint_speed.__setitem__(0, float("nan")), "observation: max_joint_speed must be finite and >= 0"),
    (_set("max_episode_steps", -1), "observation: max_episode_steps must be >= 0"),
    (lambda c: (setattr(c, "criteria", _abi.DONE_TIMEOUT), setattr(c, "max_episode_steps", 0)), "observation: TIMEOUT needs max_episode_steps >= 1"),
    (lambda c: (setattr(c, "criteria", _abi.DONE_SUCCESS), setattr(c, "success_task_mask", 0)), "observation: SUCCESS needs a task in success_task_mask"),
    (lambda c: (setattr(c, "criteria", _abi.DONE_FORCE), setattr(c, "force_task_mask", 0)), "observation: FORCE needs a task in force_task_mask"),
])
def test_validate_rejects(edit, message):
    cfg = _default()
    cfg.blocks, cfg.task_mask, cfg.task_blocks = _abi.OBS_Q | _abi.OBS_CONTACT, 1, _abi.OBS_POSE | _abi.OBS_ERROR
    cfg.criteria, cfg.success_task_mask, cfg.force_task_mask, cfg.max_episode_steps = 63, 1, 1, 10
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    edit(cfg)
    rc, msg = _validate(cfg, _tasks())
    assert rc == _abi.INVALID_ARGUMENT and msg == message
    assert _lib().sai2b_last_error(None).decode() == message


def test_validate_ignores_speed_entries_past_the_robot_and_other_sizes():
    cfg = _default()
    cfg.max_joint_speed[7] = -1.0  # a 7-joint robot has no joint 7
    assert _validate(cfg, _tasks())[0] == _abi.OK
    assert _validate(cfg, _tasks(8), dof=8)[0] == _abi.INVALID_ARGUMENT
    for dof in (4, 6, 8):
        assert _validate(_default(), _tasks(dof), dof=dof) == (_abi.OK, "")
    assert _validate(_default(), _tasks(), dof=5)[0] == _abi.UNSUPPORTED  # no build for a 5-joint robot
    assert _validate(None, _tasks())[0] == _abi.INVALID_ARGUMENT


@pytest.mark.parametrize("dof", [4, 6, 7, 8])
def test_layout_arithmetic(dof):
    n = dof
    cfg = _default()
    # everything, two observed tasks (0 and 2): globals in flag order, then per task POSE TWIST ERROR SENSED
    cfg.blocks, cfg.task_mask, cfg.task_blocks = 63, 0b101, 15
    g = {1: (0, n), 2: (n, n), 4: (2 * n, n), 8: (3 * n, 1), 16: (3 * n + 1, 1), 32: (3 * n + 2, 14)}
    total = 3 * n + 16 + 2 * 32
    for block, (first, rows) in g.items():
        assert _layout(cfg, block, dof=dof) == (_abi.OK, first, rows, total)
    t0 = 3 * n + 16
    per = {1: (0, 12), 2: (12, 6), 4: (18, 8), 8: (26, 6)}
    for block, (off, rows) in per.items():
        assert _layout(cfg, block, 0, dof=dof) == (_abi.OK, t0 + off, rows, total)
        assert _layout(cfg, block, 2, dof=dof) == (_abi.OK, t0 + 32 + off, rows, total)
        assert _layout(cfg, block, 1, dof=dof) == (_abi.OK, -1, 0, total)  # task 1 is not observed
    # a sparse selection: DQ, EPISODE_STEP; task 1 with TWIST and SENSED
    cfg.blocks, cfg.task_mask, cfg.task_blocks = _abi.OBS_DQ | _abi.OBS_EPISODE_STEP, 0b10, _abi.OBS_TWIST | _abi.OBS_SENSED
    total = n + 1 + 12
    assert _layout(cfg, _abi.OBS_Q, dof=dof) == (_abi.OK, -1, 0, total)
    assert _layout(cfg, _abi.OBS_DQ, dof=dof) == (_abi.OK, 0, n, total)
    assert _layout(cfg, _abi.OBS_EPISODE_STEP, dof=dof) == (_abi.OK, n, 1, total)
    assert _layout(cfg, _abi.OBS_TWIST, 1, dof=dof) == (_abi.OK, n + 1, 6, total)
    assert _layout(cfg, _abi.OBS_POSE, 1, dof=dof) == (_abi.OK, -1, 0, total)
    assert _layout(cfg, _abi.OBS_SENSED, 1, dof=dof) == (_abi.OK, n + 7, 6, total)
    # tasks observed but no per-task block, and the reverse: no rows
    cfg.blocks, cfg.task_mask, cfg.task_blocks = 0, 0b11, 0
    assert _layout(cfg, _abi.OBS_POSE, 0, dof=dof) == (_abi.OK, -1, 0, 0)
    cfg.task_mask, cfg.task_blocks = 0, 15
    assert _layout(cfg, _abi.OBS_POSE, 0, dof=dof) == (_abi.OK, -1, 0, 0)


def test_layout_rejects_bad_queries():
    cfg = _default()
    cfg.blocks = 63
    for block, task in ((0, -1), (3, -1), (64, -1), (16, 0), (1, -2), (1, 4)):
        assert _layout(cfg, block, task)[0] == _abi.INVALID_ARGUMENT, (block, task)


def test_null_context_is_a_bad_argument():
    lib = _lib()
    cfg = _default()
    assert lib.sai2b_set_observation(None, C.byref(cfg)) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_clear_observation(None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_observe(None, None, None, 0) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_done_counts(None, (C.c_int * 7)()) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_observation_layout(None, 1, -1, None, None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_observation_rows(None) == -1
