"""CPU-only: sai2b_default_hardware / sai2b_validate_hardware / sai2b_sizeof_hardware_config (host-only entry points of the
built library, through ctypes): the defaults, every rejection that include/sai2b.h lists for the configuration, with its
message, and the size of the ctypes mirror. (The rejections of the per-robot rows need a context: tests/test_gpu_hardware.py.)"""
import ctypes as C

import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi


def _lib():
    return _abi.load_library()


def _default():
    cfg = _abi.HardwareConfig()
    return _lib().sai2b_default_hardware(C.byref(cfg)), cfg


def _validate(cfg, tasks, dof=7):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_hardware(C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def _tasks():
    return [pkg.motion_force_task_config("m"), pkg.joint_task_config("j")]


def test_layout_of_the_mirror():
    assert _lib().sai2b_sizeof_hardware_config() == C.sizeof(_abi.HardwareConfig) == 24  # four 4-byte fields and the 8-byte seed
    assert _abi.HardwareConfig.first_robot.offset == 8 and _abi.HardwareConfig.seed.offset == 16
    assert (_abi.BUF_HARDWARE_ACTUATOR, _abi.BUF_HARDWARE_SENSOR, _abi.BUF_TAU_APPLIED, _abi.MAX_ACTUATION_DELAY) == (15, 16, 17, 8)


def test_defaults():
    rc, cfg = _default()
    assert rc == _abi.OK and (cfg.max_delay, cfg.sensor_task, cfg.first_robot, cfg.reserved, cfg.seed) == (0, -1, 0, 0, 0)
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    assert _lib().sai2b_default_hardware(None) == _abi.INVALID_ARGUMENT
    cfg.max_delay, cfg.sensor_task, cfg.first_robot, cfg.seed = 8, 0, 2**32 - 1, 2**64 - 1
    assert _validate(cfg, _tasks()) == (_abi.OK, "")


@pytest.mark.parametrize("edit, message", [
    (lambda c: setattr(c, "max_delay", -1), "hardware: max_delay must be in [0, SAI2B_MAX_ACTUATION_DELAY]"),
    (lambda c: setattr(c, "max_delay", 9), "hardware: max_delay must be in [0, SAI2B_MAX_ACTUATION_DELAY]"),
    (lambda c: setattr(c, "sensor_task", 1), "hardware: sensor_task must be -1 or the index of a MotionForceTask"),
    (lambda c: setattr(c, "sensor_task", 2), "hardware: sensor_task must be -1 or the index of a MotionForceTask"),
    (lambda c: setattr(c, "sensor_task", -2), "hardware: sensor_task must be -1 or the index of a MotionForceTask"),
])
def test_rejections(edit, message):
    rc, cfg = _default()
    assert rc == _abi.OK
    edit(cfg)
    rc, msg = _validate(cfg, _tasks())
    assert rc == _abi.INVALID_ARGUMENT and msg == message
    assert _lib().sai2b_last_error(None).decode() == message


def test_null_config_and_robot_size():
    arr = (_abi.TaskConfig * 2)(*_tasks())
    msg = C.create_string_buffer(256)
    assert _lib().sai2b_validate_hardware(None, arr, 2, 7, msg, 256) == _abi.INVALID_ARGUMENT and msg.value.decode() == "hardware: null config"
    rc, cfg = _default()
    cfg.sensor_task = 0
    t4 = [pkg.motion_force_task_config("m", link=3, robot_dof=4), pkg.joint_task_config("j", robot_dof=4)]
    assert _validate(cfg, t4, dof=4)[0] == _abi.OK
    assert _validate(cfg, t4, dof=5)[0] == _abi.UNSUPPORTED
