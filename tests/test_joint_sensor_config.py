"""The joint sensors' host side without a GPU (include/sai2b.h "joint sensors").

1: the configuration: the default, the ctypes mirror's size, every rejection of sai2b_validate_joint_sensor with its message,
   and a robot size this library has no build for.
2: the entry points are exported, and the Python names of the appended snapshot blocks continue the list.
3: the snapshot layout (tests/cpp/joint_sensor_layout_driver.cpp includes csrc/sai2b_snapshot_layout.h alone, plain g++ per
   joint count). With the feature: joint_sensor_q / _dq / _previous / _filter dof rows each, joint_sensor_history
   (D + 1) 2 dof, joint_sensor_clock 2 (4-byte) in the episode group and joint_sensor_rows 1 + 5 dof in the environment group,
   for 4 / 6 / 7 / 8 joints and D = 0, 3, 8; every block before them keeps its words. Without it: the table of every
   description, with and without each earlier feature, is row for row and fingerprint for fingerprint what the header of the
   commit before gave (tests/golden/snapshot_layout_before_joint_sensor.json, recorded from that header with
   tests/cpp/env_sampler_driver.cpp). A difference is named by the first block one description lacks.
(The validation of host rows needs a context; tests/test_gpu_joint_sensor.py has every rejection and its message.)"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import pytest

import env_sampler_reference as er
import test_snapshot_layout as sl
from sai2_primitives_perso_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "cpp", "joint_sensor_layout_driver.cpp")
GOLDEN = os.path.join(HERE, "golden", "snapshot_layout_before_joint_sensor.json")
HEAD = sl.HEAD + ("hardware", "hardware_depth", "reward", "reset_sampler", "env_sampler", "joint_sensor", "joint_sensor_depth")
NEW = _abi.SNAP_JOINT_SENSOR_BLOCKS

_built = {}


def _lib():
    return _abi.load_library()


def _validate(cfg, dof=7):
    msg = C.create_string_buffer(256)
    return _lib().sai2b_validate_joint_sensor(C.byref(cfg), dof, msg, 256), msg.value.decode()


def test_default_size_and_every_rejection():
    lib = _lib()
    cfg = _abi.JointSensorConfig(max_delay=5, velocity_mode=1, first_robot=3, reserved=9, seed=77)
    assert lib.sai2b_default_joint_sensor(C.byref(cfg)) == _abi.OK
    assert (cfg.max_delay, cfg.velocity_mode, cfg.first_robot, cfg.reserved, cfg.seed) == (0, 0, 0, 0, 0)
    assert lib.sai2b_default_joint_sensor(None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_sizeof_joint_sensor_config() == C.sizeof(_abi.JointSensorConfig) == 24
    for n in (4, 6, 7, 8):
        assert _validate(cfg, n) == (_abi.OK, "")
    for d in (0, 3, _abi.MAX_ACTUATION_DELAY):
        for mode in (0, 1):
            assert _validate(_abi.JointSensorConfig(max_delay=d, velocity_mode=mode, seed=2**64 - 1, first_robot=2**32 - 1))[0] == _abi.OK
    for d in (-1, _abi.MAX_ACTUATION_DELAY + 1):
        assert _validate(_abi.JointSensorConfig(max_delay=d)) == (_abi.INVALID_ARGUMENT, "joint sensor: max_delay must be in [0, SAI2B_MAX_ACTUATION_DELAY]")
    for mode in (-1, 2):
        assert _validate(_abi.JointSensorConfig(velocity_mode=mode)) == (
            _abi.INVALID_ARGUMENT, "joint sensor: velocity_mode must be 0 (tachometer) or 1 (finite difference)")
    rc = lib.sai2b_validate_joint_sensor(None, 7, None, 0)
    assert rc == _abi.INVALID_ARGUMENT and b"null config" in lib.sai2b_last_error(None)
    assert _validate(cfg, 5)[0] == _abi.UNSUPPORTED


def test_exports_and_block_names():
    for name in ("sai2b_default_joint_sensor", "sai2b_validate_joint_sensor", "sai2b_sizeof_joint_sensor_config", "sai2b_set_joint_sensor",
                 "sai2b_clear_joint_sensor", "sai2b_get_joint_sensor", "sai2b_get_joint_sensor_state", "sai2b_get_measured_state"):
        assert name in _abi.EXPORTS and getattr(_lib(), name)
    assert (_abi.BUF_Q_MEASURED, _abi.BUF_DQ_MEASURED, _abi.BUF_JOINT_SENSOR) == (21, 22, 23)
    assert _abi.SNAP_BLOCK_NAMES_ALL[: len(_abi.SNAP_BLOCK_NAMES)] == _abi.SNAP_BLOCK_NAMES and _abi.SNAP_BLOCK_NAMES_ALL[-7:] == NEW
    # null contexts are bad arguments, not crashes
    lib = _lib()
    assert lib.sai2b_set_joint_sensor(None, None, None, 0) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_clear_joint_sensor(None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_joint_sensor(None, None, None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_joint_sensor_state(None, None, None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_measured_state(None, None, None) == _abi.INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- snapshot layout
def _build(tmp_factory, n):
    if n not in _built:
        exe = os.path.join(str(tmp_factory.mktemp(f"jssnap{n}")), "joint_sensor_layout_driver")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DSAI2B_N={n}", "-I", sl.CSRC, DRIVER, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[n] = exe
    return _built[n]


def _args(d, hardware=0, depth=0, reward=0, sampler=0, env=0, js=0, js_depth=0):
    d = dict(d, hardware=hardware, hardware_depth=depth, reward=reward, reset_sampler=sampler, env_sampler=env, joint_sensor=js, joint_sensor_depth=js_depth)
    return [d[k] for k in HEAD] + [t[k] for t in d["tasks"] for k in sl.TASK]


def _table(exe, d, **kw):
    rows, tail = [], None
    for line in sl._run(exe, "table", *_args(d, **kw)).splitlines():
        f = line.split()
        if f[0] == "row":
            rows.append(dict(id=int(f[1]), block=f[2], task=int(f[3]), rows=int(f[4]), elem=int(f[5]), word=int(f[6]), first_row=int(f[7])))
        else:
            tail = dict(words=int(f[1]), rows=int(f[3]), fingerprint=f[5])
    return rows, tail


@pytest.mark.parametrize("n", [4, 6, 7, 8])
@pytest.mark.parametrize("depth", [0, 3, 8])
def test_rows_of_the_new_blocks(tmp_path_factory, n, depth):
    exe = _build(tmp_path_factory, n)
    consts = {k: int(v) for k, v in (line.split() for line in sl._run(exe, "consts").splitlines())}
    assert consts["BLOCKS_ALL"] == 36 and consts["BLOCKS_EVERY"] == 43 == len(_abi.SNAP_BLOCK_NAMES_ALL) and consts["FULL"] == consts["ROOM"] + 7
    d = sl.descriptions(n)["everything"]
    total = er.layout(31, n)[1]
    for other in (dict(), dict(hardware=1, depth=8, reward=1, sampler=1, env=1 + total)):
        rows, tail = _table(exe, d, js=1, js_depth=depth, **other)
        base, base_tail = _table(exe, d, **other)
        new = {r["block"]: r for r in rows if r["block"].startswith("joint_sensor")}
        want = dict(joint_sensor_q=(n, 8), joint_sensor_dq=(n, 8), joint_sensor_previous=(n, 8), joint_sensor_filter=(n, 8),
                    joint_sensor_history=((depth + 1) * 2 * n, 8), joint_sensor_clock=(2, 4), joint_sensor_rows=(1 + 5 * n, 8))
        assert {k: (r["rows"], r["elem"]) for k, r in new.items()} == want and all(r["task"] == -1 for r in new.values())
        assert sorted(r["id"] for r in new.values()) == list(range(36, 43))
        assert [_abi.SNAP_BLOCK_NAMES_ALL[r["id"]] for r in rows] == [r["block"] for r in rows]
        assert len(rows) == len(base) + 7 <= consts["FULL"]
        # words contiguous, in table order; 8-byte blocks ahead of the 4-byte ones; the clock is the last block of all
        word = first = 0
        for r in rows:
            assert (r["word"], r["first_row"]) == (word, first), r
            word, first = word + r["rows"] * r["elem"] // 4, first + r["rows"]
        assert (tail["words"], tail["rows"]) == (word, first)
        elems = [r["elem"] for r in rows]
        assert elems == sorted(elems, reverse=True) and rows[-1]["block"] == "joint_sensor_clock"
        eight = [r["block"] for r in rows if r["elem"] == 8]
        assert eight[-1] == "joint_sensor_rows"
        assert tail["words"] == base_tail["words"] + sum(r["rows"] * r["elem"] // 4 for r in new.values())
        assert tail["fingerprint"] != base_tail["fingerprint"]
        # the rest of the table in its order
        assert [(r["block"], r["task"], r["rows"]) for r in rows if not r["block"].startswith("joint_sensor")] == [(r["block"], r["task"], r["rows"]) for r in base]
    epi, _ = _table(exe, dict(d, what=sl.EPISODE), js=1, js_depth=depth)
    env, _ = _table(exe, sl.descriptions(n)["environment_only"], js=1, js_depth=0)
    assert {r["block"] for r in epi if r["block"].startswith("joint_sensor")} == set(NEW[:-1])
    assert {r["block"] for r in env if r["block"].startswith("joint_sensor")} == {"joint_sensor_rows"}


@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_without_the_joint_sensor_the_layout_is_what_it_was(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    golden = json.load(open(GOLDEN))[str(n)]
    descs = sl.descriptions(n)
    total = er.layout(31, n)[1]
    assert len(golden) == 16 * len(descs)
    for name, d in descs.items():
        for hs, hw in (("", (0, 0)), ("+hw3", (1, 3))):
            for rs, rew in (("", 0), ("+rew", 1)):
                for ss, smp in (("", 0), ("+rs", 1)):
                    for es, env in (("", 0), ("+es", 1 + total)):
                        lines = sl._run(exe, "table", *_args(d, hardware=hw[0], depth=hw[1], reward=rew, sampler=smp, env=env)).splitlines()
                        table = "\n".join(line for line in lines if line.startswith("row "))
                        f = lines[-1].split()
                        got = [len(lines) - 1, int(f[1]), int(f[3]), f[5], hashlib.sha256(table.encode()).hexdigest()[:32]]
                        assert got == golden[name + hs + rs + ss + es], name + hs + rs + ss + es


@pytest.mark.parametrize("n", [4, 7, 8])
def test_fingerprints_and_the_named_difference(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["c3"]
    prints = {depth: _table(exe, d, js=1, js_depth=depth)[1]["fingerprint"] for depth in (0, 3, 8)}
    none = _table(exe, d)[1]["fingerprint"]
    assert len(set(prints.values()) | {none}) == 4

    def diff(d, a, b, **kw):
        return sl._run(exe, "diff", *_args(d, js=a[0], js_depth=a[1], **kw), "--", *_args(d, js=b[0], js_depth=b[1], **kw)).strip()

    assert diff(d, (1, 3), (1, 3)) == "same" and diff(d, (0, 0), (0, 0)) == "same"
    for a, b in (((1, 0), (1, 3)), ((1, 8), (1, 3))):
        assert diff(d, a, b) == "differ block joint_sensor_history", (a, b)
    # a bank made before sai2b_set_joint_sensor: the first block it lacks
    for a, b in (((0, 0), (1, 3)), ((1, 0), (0, 0))):
        assert diff(d, a, b) == "differ block joint_sensor_q", (a, b)
    full = sl.descriptions(n)["everything"]
    total = er.layout(31, n)[1]
    assert diff(full, (1, 2), (0, 0), hardware=1, depth=2, reward=1, sampler=1, env=1 + total) == "differ block joint_sensor_q"
    assert diff(sl.descriptions(n)["environment_only"], (1, 0), (0, 0), env=1 + total) == "differ block joint_sensor_rows"
    # and an earlier feature's difference is still named as its own block with the joint sensor present on both sides
    assert sl._run(exe, "diff", *_args(full, hardware=1, depth=2, js=1), "--", *_args(full, js=1)).strip() == "differ block hw_history"
