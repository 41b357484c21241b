"""The blocks the actuator and sensor models add to a snapshot bank (csrc/sai2b_snapshot_layout.h) on the CPU:
tests/cpp/hardware_layout_driver.cpp includes the header alone and is built with plain g++ per joint count.

1: rows, element sizes and word offsets of the new blocks for D = 0, 3, 8 and 4 / 7 / 8 joints: hw_history (D + 1) dof,
   hw_filter dof + 6, hw_applied dof, hw_clock 2 (4-byte) in the episode group, hw_actuator 1 + 3 dof and hw_sensor 13 in the
   environment group; words contiguous, 8-byte blocks first.
2: hardware = 0: the table of every description of tests/test_snapshot_layout.py is, row for row and fingerprint for
   fingerprint, what the header gave before the feature (tests/golden/snapshot_layout_before_hardware.json, recorded from the
   header of the commit before it with tests/cpp/snapshot_layout_driver.cpp): blobs exported before still import.
3: hardware = 1: every D has a fingerprint of its own, none that of hardware = 0, and the difference between two depths is
   named as hw_history; hardware against none is named as hw_history too (the first block one of them lacks)."""
import json
import os
import subprocess

import pytest

import test_snapshot_layout as sl

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "cpp", "hardware_layout_driver.cpp")
GOLDEN = os.path.join(HERE, "golden", "snapshot_layout_before_hardware.json")
HEAD = sl.HEAD + ("hardware", "hardware_depth")

_built = {}


def _build(tmp_factory, n):
    if n not in _built:
        exe = os.path.join(str(tmp_factory.mktemp(f"hwsnap{n}")), "hardware_layout_driver")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DSAI2B_N={n}", "-I", sl.CSRC, DRIVER, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[n] = exe
    return _built[n]


def _args(d, hardware=0, depth=0):
    d = dict(d, hardware=hardware, hardware_depth=depth)
    return [d[k] for k in HEAD] + [t[k] for t in d["tasks"] for k in sl.TASK]


def _table(exe, d, hardware=0, depth=0):
    rows, tail = [], None
    for line in sl._run(exe, "table", *_args(d, hardware, depth)).splitlines():
        f = line.split()
        if f[0] == "row":
            rows.append(dict(block=f[2], task=int(f[3]), rows=int(f[4]), elem=int(f[5]), word=int(f[6]), first_row=int(f[7])))
        else:
            tail = dict(words=int(f[1]), rows=int(f[3]), fingerprint=f[5])
    return rows, tail


@pytest.mark.parametrize("n", [4, 7, 8])
@pytest.mark.parametrize("depth", [0, 3, 8])
def test_rows_of_the_new_blocks(tmp_path_factory, n, depth):
    exe = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["everything"]
    rows, tail = _table(exe, d, 1, depth)
    base, base_tail = _table(exe, d)
    new = {r["block"]: r for r in rows if r["block"].startswith("hw_")}
    want = dict(hw_history=((depth + 1) * n, 8), hw_filter=(n + 6, 8), hw_applied=(n, 8), hw_clock=(2, 4), hw_actuator=(1 + 3 * n, 8), hw_sensor=(13, 8))
    assert {k: (r["rows"], r["elem"]) for k, r in new.items()} == want and all(r["task"] == -1 for r in new.values())
    assert [r for r in rows if not r["block"].startswith("hw_")] != [] and len(rows) == len(base) + 6
    # words contiguous, in table order; 8-byte blocks ahead of the 4-byte ones
    word = first = 0
    for r in rows:
        assert (r["word"], r["first_row"]) == (word, first), r
        word, first = word + r["rows"] * r["elem"] // 4, first + r["rows"]
    assert (tail["words"], tail["rows"]) == (word, first)
    elems = [r["elem"] for r in rows]
    assert elems == sorted(elems, reverse=True) and rows[-1]["block"] == "hw_clock"
    extra = sum(r["rows"] * r["elem"] // 4 for r in new.values())
    assert tail["words"] == base_tail["words"] + extra
    # an episode-only bank has the four episode blocks, an environment-only one the two row buffers
    epi, _ = _table(exe, dict(d, what=sl.EPISODE), 1, depth)
    env, _ = _table(exe, sl.descriptions(n)["environment_only"], 1, 0)
    assert {r["block"] for r in epi if r["block"].startswith("hw_")} == {"hw_history", "hw_filter", "hw_applied", "hw_clock"}
    assert {r["block"] for r in env if r["block"].startswith("hw_")} == {"hw_actuator", "hw_sensor"}


@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_without_hardware_the_layout_is_what_it_was(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    golden = json.load(open(GOLDEN))[str(n)]
    descs = sl.descriptions(n)
    assert set(descs) == set(golden) and len(descs) == 14
    for name, d in descs.items():
        rows, tail = _table(exe, d)
        got = [[r["block"], r["task"], r["rows"], r["elem"], r["word"], r["first_row"]] for r in rows]
        assert got == golden[name]["rows"], name
        assert (tail["words"], tail["rows"], tail["fingerprint"]) == (golden[name]["words"], golden[name]["total_rows"], golden[name]["fingerprint"]), name


@pytest.mark.parametrize("n", [4, 7, 8])
def test_fingerprints_and_the_named_difference(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["c3"]
    prints = {depth: _table(exe, d, 1, depth)[1]["fingerprint"] for depth in (0, 3, 8)}
    none = _table(exe, d)[1]["fingerprint"]
    assert len(set(prints.values()) | {none}) == 4

    def diff(a, b):
        return sl._run(exe, "diff", *_args(d, *a), "--", *_args(d, *b)).strip()

    assert diff((1, 3), (1, 3)) == "same" and diff((0, 0), (0, 0)) == "same"
    for a, b in (((1, 0), (1, 3)), ((1, 8), (1, 3)), ((0, 0), (1, 3)), ((1, 0), (0, 0))):
        assert diff(a, b) == "differ block hw_history", (a, b)
    # with an environment group behind it the episode block is still the one named
    full = dict(sl.descriptions(n)["everything"])
    out = sl._run(exe, "diff", *_args(full, 1, 2), "--", *_args(full, 0, 0)).strip()
    assert out == "differ block hw_history"
