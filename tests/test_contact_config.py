"""CPU-only: sai2b_default_contact / sai2b_validate_contact (host-only entry points of the built library, through ctypes):
the defaults, and every rejection that include/sai2b.h lists for the configuration, with its message."""
import ctypes as C

import numpy as np
import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi


def _lib():
    return _abi.load_library()


def _default(link=6, n_points=1, points=None):
    cfg = _abi.ContactConfig()
    p = None if points is None else np.ascontiguousarray(points, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    return _lib().sai2b_default_contact(C.byref(cfg), link, n_points, p), cfg


def _validate(cfg, tasks, dof=7):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_contact(C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def _tasks():
    return [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")]


def test_layout_of_the_mirror():
    assert C.sizeof(_abi.ContactConfig) == 4 + 4 + 4 * 3 * 8 + 8 + 8  # two ints, the points, eps, sensor_task + padding
    assert _abi.ContactConfig.points.offset == 8 and _abi.ContactConfig.friction_velocity_eps.offset == 104
    assert _abi.ContactConfig.sensor_task.offset == 112 and _abi.BUF_CONTACT == 10


def test_defaults():
    rc, cfg = _default(5, 1)
    assert rc == _abi.OK and (cfg.link, cfg.n_points, cfg.sensor_task) == (5, 1, -1)
    assert cfg.friction_velocity_eps == 1e-3 and all(cfg.points[k][a] == 0 for k in range(4) for a in range(3))
    pts = np.arange(12.0).reshape(4, 3) * 0.01
    rc, cfg = _default(6, 4, pts)
    assert rc == _abi.OK and np.array_equal(np.array([list(r) for r in cfg.points]), pts)
    rc, cfg = _default(6, 2, pts)
    assert rc == _abi.OK and list(cfg.points[2]) == [0, 0, 0]  # only n_points rows are read
    for n in (0, 5, -1):
        assert _default(6, n)[0] == _abi.INVALID_ARGUMENT
    assert _validate(_default(6, 4, pts)[1], _tasks()) == (_abi.OK, "")


@pytest.mark.parametrize("edit, message", [
    (lambda c: setattr(c, "link", -1), "contact: link must be in [0, dof)"),
    (lambda c: setattr(c, "link", 7), "contact: link must be in [0, dof)"),
    (lambda c: setattr(c, "n_points", 0), "contact: n_points must be in [1, 4]"),
    (lambda c: setattr(c, "n_points", 5), "contact: n_points must be in [1, 4]"),
    (lambda c: c.points[1].__setitem__(2, float("nan")), "contact: points must be finite"),
    (lambda c: c.points[0].__setitem__(0, float("inf")), "contact: points must be finite"),
    (lambda c: setattr(c, "friction_velocity_eps", 0.0), "contact: friction_velocity_eps must be finite and > 0"),
    (lambda c: setattr(c, "friction_velocity_eps", -1e-3), "contact: friction_velocity_eps must be finite and > 0"),
    (lambda c: setattr(c, "friction_velocity_eps", float("nan")), "contact: friction_velocity_eps must be finite and > 0"),
    (lambda c: setattr(c, "sensor_task", 1), "contact: sensor_task must be -1 or the index of a MotionForceTask"),
    (lambda c: setattr(c, "sensor_task", 2), "contact: sensor_task must be -1 or the index of a MotionForceTask"),
    (lambda c: setattr(c, "sensor_task", -2), "contact: sensor_task must be -1 or the index of a MotionForceTask"),
])
def test_rejections(edit, message):
    rc, cfg = _default(6, 2, np.full((2, 3), 0.01))
    assert rc == _abi.OK
    edit(cfg)
    rc, msg = _validate(cfg, _tasks())
    assert rc == _abi.INVALID_ARGUMENT and msg == message
    assert _lib().sai2b_last_error(None).decode() == message


def test_sensor_task_and_robot_size():
    rc, cfg = _default(3, 1)
    cfg.sensor_task = 0
    assert _validate(cfg, _tasks())[0] == _abi.OK
    # a 4-joint robot: link 3 is its last, link 4 does not exist; a robot size without a build is unsupported
    t4 = [pkg.motion_force_task_config("m", link=3, robot_dof=4), pkg.joint_task_config("j", robot_dof=4)]
    assert _validate(cfg, t4, dof=4)[0] == _abi.OK
    cfg.link = 4
    assert _validate(cfg, t4, dof=4) == (_abi.INVALID_ARGUMENT, "contact: link must be in [0, dof)")
    assert _validate(cfg, t4, dof=5)[0] == _abi.UNSUPPORTED
