"""CPU-only: the host-only entry points of the action feature (sai2b_default_action, sai2b_validate_action,
sai2b_sizeof_action_config, sai2b_action_config_layout) through ctypes: the defaults, every rejection include/sai2b.h lists
for the configuration with its message, the layout arithmetic, and the size of the ctypes mirror."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _lib():
    return _abi.load_library()


def _default():
    cfg = _abi.ActionConfig()
    assert _lib().sai2b_default_action(C.byref(cfg)) == _abi.OK
    return cfg


def _tasks(dof=7):
    """[MotionForceTask, JointTask]"""
    return [pkg.motion_force_task_config("m", robot_dof=dof, link=dof - 1), pkg.joint_task_config("j", robot_dof=dof)]


def _validate(cfg, tasks, dof=7):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_action(None if cfg is None else C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def _layout(cfg, tasks, block, task):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    first, n, total = C.c_int(), C.c_int(), C.c_int()
    rc = _lib().sai2b_action_config_layout(C.byref(cfg), arr, len(tasks), block, task, C.byref(first), C.byref(n), C.byref(total))
    return rc, first.value, n.value, total.value


def _valid():
    """position + orientation deltas on the MotionForceTask, the joints of the JointTask"""
    cfg = _default()
    cfg.task[0].mode, cfg.task[0].blocks = _abi.ACT_DELTA_GOAL, _abi.ACT_POSITION | _abi.ACT_ORIENTATION
    cfg.task[1].mode = _abi.ACT_ABSOLUTE
    return cfg


def test_size_of_the_mirror_is_the_librarys():
    assert _lib().sai2b_sizeof_action_config() == C.sizeof(_abi.ActionConfig)
    # and the C compiler's, from the header
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sai2b.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(sai2b_action_config), '
           "sizeof(sai2b_action_task), offsetof(sai2b_action_config, task), offsetof(sai2b_action_task, max_pos_lead), "
           "offsetof(sai2b_action_task, jt_upper));return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")], check=True)
        out = subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(_abi.ActionConfig), C.sizeof(_abi.ActionTask), _abi.ActionConfig.task.offset,
                                     _abi.ActionTask.max_pos_lead.offset, _abi.ActionTask.jt_upper.offset]


def test_enum_values_match_the_header():
    header = open(os.path.join(ROOT, "include", "sai2b.h")).read()
    for name, value in {**_abi.ACT_MODES, **_abi.ACT_BLOCKS}.items():
        m = re.search("SAI2B_ACT_" + name.upper() + r"\s*=\s*(\d+)", header)
        assert m and int(m.group(1)) == value, name
    assert list(_abi.ACT_BLOCKS.values()) == [1, 2, 4, 8]


def test_defaults():
    cfg = _default()
    assert cfg.clip_actions == 0 and cfg.reserved == 0
    for t in range(_abi.MAX_TASKS):
        a = cfg.task[t]
        assert a.mode == _abi.ACT_NONE and a.blocks == 0
        assert list(a.pos_scale) == [1.0] * 3 and a.ori_scale == a.force_scale == a.moment_scale == 1.0
        assert list(a.pos_lower) == [-INF] * 3 and list(a.pos_upper) == [INF] * 3 and a.max_pos_lead == INF
        assert list(a.jt_scale) == [1.0] * 8 and list(a.jt_lower) == [-INF] * 8 and list(a.jt_upper) == [INF] * 8
    # every task NONE: nothing to apply
    assert _validate(cfg, _tasks()) == (_abi.INVALID_ARGUMENT, "action: no task has a mode")
    assert _validate(_valid(), _tasks()) == (_abi.OK, "")
    assert _lib().sai2b_default_action(None) == _abi.INVALID_ARGUMENT


def _mft(name, value, index=None):
    def edit(c):
        if index is None:
            setattr(c.task[0], name, value)
        else:
            getattr(c.task[0], name)[index] = value

    return edit


def _jt(name, value, index):
    def edit(c):
        getattr(c.task[1], name)[index] = value

    return edit


def _both(*edits):
    def edit(c):
        for e in edits:
            e(c)

    return edit


REJECTED = [
    (_mft("mode", 4), "task 0: unknown mode"),
    (_mft("mode", -1), "task 0: unknown mode"),
    (_mft("blocks", 16 | 1), "task 0: unknown bits in blocks"),
    (lambda c: setattr(c.task[3], "blocks", 32), "task 3: unknown bits in blocks"),  # also on a task without a mode
    (lambda c: setattr(c.task[1], "blocks", _abi.ACT_POSITION), "task 1: blocks are for a MotionForceTask"),
    (_mft("blocks", 0), "task 0: a MotionForceTask with a mode needs a block"),
    (lambda c: setattr(c.task[2], "mode", _abi.ACT_ABSOLUTE), "task 2: a mode on a task the hierarchy does not have"),
    (_mft("pos_scale", -1e-3, 1), "task 0: pos_scale must be finite and >= 0"),
    (_mft("pos_scale", INF, 2), "task 0: pos_scale must be finite and >= 0"),
    (_mft("ori_scale", math.nan), "task 0: ori_scale must be finite and >= 0"),
    (_mft("force_scale", -1.0), "task 0: force_scale must be finite and >= 0"),
    (_mft("moment_scale", -INF), "task 0: moment_scale must be finite and >= 0"),
    (_jt("jt_scale", -0.5, 6), "task 1: jt_scale must be finite and >= 0"),
    (_jt("jt_scale", math.nan, 0), "task 1: jt_scale must be finite and >= 0"),
    (_both(_mft("pos_lower", 0.5, 0), _mft("pos_upper", 0.5, 0)), "task 0: pos_lower must be < pos_upper"),
    (_both(_mft("pos_lower", 0.6, 2), _mft("pos_upper", 0.5, 2)), "task 0: pos_lower must be < pos_upper"),
    (_mft("pos_upper", math.nan, 1), "task 0: pos_lower must be < pos_upper"),
    (_mft("pos_lower", math.nan, 1), "task 0: pos_lower must be < pos_upper"),
    (_both(_jt("jt_lower", 1.0, 3), _jt("jt_upper", 1.0, 3)), "task 1: jt_lower must be < jt_upper"),
    (_jt("jt_upper", math.nan, 6), "task 1: jt_lower must be < jt_upper"),
    (_mft("max_pos_lead", 0.0), "task 0: max_pos_lead must be > 0"),
    (_mft("max_pos_lead", -1.0), "task 0: max_pos_lead must be > 0"),
    (_mft("max_pos_lead", math.nan), "task 0: max_pos_lead must be > 0"),
    (_both(_mft("mode", 0), lambda c: setattr(c.task[1], "mode", 0)), "action: no task has a mode"),
]


@pytest.mark.parametrize("case", range(len(REJECTED)))
def test_every_rejection_with_its_message(case):
    edit, text = REJECTED[case]
    cfg = _valid()
    edit(cfg)
    rc, msg = _validate(cfg, _tasks())
    assert rc == _abi.INVALID_ARGUMENT and text in msg, msg
    assert text.encode() in _lib().sai2b_last_error(None)


def test_what_is_not_rejected():
    cfg = _valid()
    cfg.task[0].pos_scale[0] = 0.0  # a zero scale freezes a component
    cfg.task[0].max_pos_lead = 1e-3
    cfg.task[0].pos_lower[2], cfg.task[0].pos_upper[2] = -INF, 0.0
    cfg.task[1].jt_scale[7] = math.nan  # beyond the task's 7 rows: ignored
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    assert _validate(None, _tasks())[0] == _abi.INVALID_ARGUMENT
    rc, msg = _validate(_valid(), _tasks(), dof=5)
    assert rc != _abi.OK
    # a build for every robot size answers
    for dof in (4, 6, 8):
        assert _validate(_valid(), _tasks(dof), dof) == (_abi.OK, "")


def test_layout_of_a_full_motion_force_task_and_a_joint_task():
    tasks = _tasks()
    cfg = _default()
    cfg.task[0].mode, cfg.task[0].blocks = _abi.ACT_DELTA_GOAL, 15
    cfg.task[1].mode = _abi.ACT_DELTA_CURRENT
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 0) == (_abi.OK, 0, 3, 19)
    assert _layout(cfg, tasks, _abi.ACT_ORIENTATION, 0) == (_abi.OK, 3, 3, 19)
    assert _layout(cfg, tasks, _abi.ACT_FORCE, 0) == (_abi.OK, 6, 3, 19)
    assert _layout(cfg, tasks, _abi.ACT_MOMENT, 0) == (_abi.OK, 9, 3, 19)
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 1) == (_abi.OK, 12, 7, 19)
    assert _layout(cfg, tasks, 0, 1) == (_abi.OK, 12, 7, 19)  # the block is ignored for a JointTask
    # blocks in flag order whatever is left out
    cfg.task[0].blocks = _abi.ACT_ORIENTATION | _abi.ACT_MOMENT
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 0) == (_abi.OK, -1, 0, 13)
    assert _layout(cfg, tasks, _abi.ACT_ORIENTATION, 0) == (_abi.OK, 0, 3, 13)
    assert _layout(cfg, tasks, _abi.ACT_MOMENT, 0) == (_abi.OK, 3, 3, 13)
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 1) == (_abi.OK, 6, 7, 13)
    # a task without a mode takes no rows
    cfg.task[0].mode = _abi.ACT_NONE
    assert _layout(cfg, tasks, _abi.ACT_ORIENTATION, 0) == (_abi.OK, -1, 0, 7)
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 1) == (_abi.OK, 0, 7, 7)
    # bad arguments
    assert _layout(cfg, tasks, 3, 0)[0] == _abi.INVALID_ARGUMENT and _layout(cfg, tasks, 16, 0)[0] == _abi.INVALID_ARGUMENT
    assert _layout(cfg, tasks, 1, 2)[0] == _abi.INVALID_ARGUMENT and _layout(cfg, tasks, 1, -1)[0] == _abi.INVALID_ARGUMENT


def test_layout_of_two_partial_motion_force_tasks_and_a_joint_task():
    pos_only, ori_only = (np.eye(3), np.zeros((0, 3))), (np.zeros((0, 3)), np.eye(3))
    tasks = [pkg.motion_force_task_config("p", partial=pos_only), pkg.motion_force_task_config("o", link=4, partial=ori_only),
             pkg.joint_task_config("j")]
    cfg = _default()
    cfg.task[0].mode, cfg.task[0].blocks = _abi.ACT_DELTA_GOAL, _abi.ACT_POSITION
    cfg.task[1].mode, cfg.task[1].blocks = _abi.ACT_ABSOLUTE, _abi.ACT_ORIENTATION
    cfg.task[2].mode = _abi.ACT_DELTA_GOAL
    assert _validate(cfg, tasks) == (_abi.OK, "")
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 0) == (_abi.OK, 0, 3, 13)
    assert _layout(cfg, tasks, _abi.ACT_ORIENTATION, 0) == (_abi.OK, -1, 0, 13)
    assert _layout(cfg, tasks, _abi.ACT_ORIENTATION, 1) == (_abi.OK, 3, 3, 13)
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 2) == (_abi.OK, 6, 7, 13)


def test_layout_of_a_partial_joint_task_on_the_8_joint_robot():
    sel = np.zeros((2, 8))
    sel[0, 0], sel[1, 3] = 1.0, 1.0
    tasks = [pkg.joint_task_config("base", selection=sel, robot_dof=8), pkg.motion_force_task_config("m", robot_dof=8, link=7)]
    cfg = _default()
    cfg.task[0].mode = _abi.ACT_DELTA_CURRENT
    cfg.task[1].mode, cfg.task[1].blocks = _abi.ACT_DELTA_CURRENT, _abi.ACT_POSITION | _abi.ACT_FORCE
    cfg.task[0].jt_lower[0], cfg.task[0].jt_upper[0] = -0.4, 0.4
    cfg.task[0].jt_scale[2] = -1.0  # beyond the task's two rows: ignored
    assert _validate(cfg, tasks, dof=8) == (_abi.OK, "")
    assert _layout(cfg, tasks, 0, 0) == (_abi.OK, 0, 2, 8)
    assert _layout(cfg, tasks, _abi.ACT_POSITION, 1) == (_abi.OK, 2, 3, 8)
    assert _layout(cfg, tasks, _abi.ACT_FORCE, 1) == (_abi.OK, 5, 3, 8)
    cfg.task[0].jt_scale[1] = -1.0
    assert _validate(cfg, tasks, dof=8) == (_abi.INVALID_ARGUMENT, "action: task 0: jt_scale must be finite and >= 0")
