"""The blocks the reward's accumulators add to a snapshot bank (csrc/sai2b_snapshot_layout.h) on the CPU:
tests/cpp/reward_layout_driver.cpp includes the header alone and is built with plain g++ per joint count, and once more with
-fsanitize=address,undefined and run as the stand-alone program it is.

1: rows, element sizes and word offsets of the two blocks for 4 / 7 / 8 joints: reward_state 3 + dof (8-byte), reward_episode 2
   (4-byte), both in the episode group; words contiguous, 8-byte blocks first.
2: reward = 0: the table of every description of tests/test_snapshot_layout.py, without hardware and with it (D = 3), is, row for
   row and fingerprint for fingerprint, what the header gave before the feature (tests/golden/snapshot_layout_before_reward.json,
   recorded from the header of the commit before it with tests/cpp/hardware_layout_driver.cpp): blobs exported before still
   import. The two drivers from before the field existed compile unchanged under -Wall -Werror.
3: reward = 1: another fingerprint, and the difference is named as reward_state (the first block one of them lacks)."""
import json
import os
import subprocess

import pytest

import test_hardware_snapshot_layout as hl
import test_snapshot_layout as sl

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "cpp", "reward_layout_driver.cpp")
GOLDEN = os.path.join(HERE, "golden", "snapshot_layout_before_reward.json")
HEAD = hl.HEAD + ("reward",)
HARDWARE = {"": (0, 0), "+hw3": (1, 3)}  # suffix of the golden's names -> (hardware, hardware_depth)

_built = {}


def _build(tmp_factory, n, sanitize=False):
    key = (n, sanitize)
    if key not in _built:
        exe = os.path.join(str(tmp_factory.mktemp(f"rewsnap{n}{'s' if sanitize else ''}")), "reward_layout_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DSAI2B_N={n}", "-I", sl.CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[4:4] = [sl.SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[key] = exe
    return _built[key]


def _args(d, hardware=0, depth=0, reward=0):
    d = dict(d, hardware=hardware, hardware_depth=depth, reward=reward)
    return [d[k] for k in HEAD] + [t[k] for t in d["tasks"] for k in sl.TASK]


def _table(exe, d, hardware=0, depth=0, reward=0):
    rows, tail = [], None
    for line in sl._run(exe, "table", *_args(d, hardware, depth, reward)).splitlines():
        f = line.split()
        if f[0] == "row":
            rows.append(dict(block=f[2], task=int(f[3]), rows=int(f[4]), elem=int(f[5]), word=int(f[6]), first_row=int(f[7])))
        else:
            tail = dict(words=int(f[1]), rows=int(f[3]), fingerprint=f[5])
    return rows, tail


@pytest.mark.parametrize("n", [4, 7, 8])
@pytest.mark.parametrize("hardware", [(0, 0), (1, 8)])
def test_rows_of_the_new_blocks(tmp_path_factory, n, hardware):
    exe = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["everything"]
    rows, tail = _table(exe, d, *hardware, reward=1)
    base, base_tail = _table(exe, d, *hardware)
    new = {r["block"]: r for r in rows if r["block"].startswith("reward_")}
    assert {k: (r["rows"], r["elem"], r["task"]) for k, r in new.items()} == dict(reward_state=(3 + n, 8, -1), reward_episode=(2, 4, -1))
    assert [r["block"] for r in rows if not r["block"].startswith("reward_")] == [r["block"] for r in base] and len(rows) == len(base) + 2
    consts = {k: int(v) for k, v in (line.split() for line in sl._run(exe, "consts").splitlines())}
    assert len(rows) <= consts["MAX_TABLE"] and consts["MAX_TABLE"] == 9 + 11 * 4 + 5 + 6 + 2
    # words contiguous, in table order; 8-byte blocks ahead of the 4-byte ones; reward_episode is the last 4-byte block
    word = first = 0
    for r in rows:
        assert (r["word"], r["first_row"]) == (word, first), r
        word, first = word + r["rows"] * r["elem"] // 4, first + r["rows"]
    assert (tail["words"], tail["rows"]) == (word, first)
    elems = [r["elem"] for r in rows]
    assert elems == sorted(elems, reverse=True) and rows[-1]["block"] == "reward_episode"
    assert new["reward_state"]["word"] % 2 == 0
    assert tail["words"] == base_tail["words"] + 2 * (3 + n) + 2
    # the blocks stand with the episode group: behind the hardware's episode blocks (or the status rows), ahead of the environment
    names = [r["block"] for r in rows if r["elem"] == 8]
    k = names.index("reward_state")
    assert names[k - 1] == ("hw_applied" if hardware[0] else "wrench_status") and names[k + 1] == "payload"
    # an episode-only bank has both, an environment-only one neither
    epi, _ = _table(exe, dict(d, what=sl.EPISODE), *hardware, reward=1)
    env, _ = _table(exe, sl.descriptions(n)["environment_only"], *hardware, reward=0)
    assert {r["block"] for r in epi if r["block"].startswith("reward_")} == {"reward_state", "reward_episode"}
    assert not [r for r in env if r["block"].startswith("reward_")]


@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_without_a_reward_the_layout_is_what_it_was(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    golden = json.load(open(GOLDEN))[str(n)]
    descs = sl.descriptions(n)
    assert set(golden) == {name + suffix for name in descs for suffix in HARDWARE} and len(descs) == 14
    for name, d in descs.items():
        for suffix, hw in HARDWARE.items():
            rows, tail = _table(exe, d, *hw)
            got = [[r["block"], r["task"], r["rows"], r["elem"], r["word"], r["first_row"]] for r in rows]
            g = golden[name + suffix]
            assert got == g["rows"], name + suffix
            assert (tail["words"], tail["rows"], tail["fingerprint"]) == (g["words"], g["total_rows"], g["fingerprint"]), name + suffix


@pytest.mark.parametrize("n", [7, 8])
def test_the_drivers_from_before_the_field_compile_unchanged(tmp_path_factory, n):
    old, old_hw = sl._build(tmp_path_factory, n), hl._build(tmp_path_factory, n)
    new = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["everything"]
    assert sl._run(old, "table", *sl._args(d)) == sl._run(new, "table", *_args(d))
    assert sl._run(old_hw, "table", *hl._args(d, 1, 3)) == sl._run(new, "table", *_args(d, 1, 3))


@pytest.mark.parametrize("n", [4, 7, 8])
def test_fingerprint_and_the_named_difference(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    for name in ("c3", "everything"):
        d = sl.descriptions(n)[name]
        for hw in HARDWARE.values():
            assert _table(exe, d, *hw, reward=1)[1]["fingerprint"] != _table(exe, d, *hw)[1]["fingerprint"]

            def diff(a, b):
                return sl._run(exe, "diff", *_args(d, *hw, reward=a), "--", *_args(d, *hw, reward=b)).strip()

            assert diff(1, 1) == "same" and diff(0, 0) == "same"
            assert diff(0, 1) == "differ block reward_state" and diff(1, 0) == "differ block reward_state"


def test_sanitized_driver(tmp_path_factory):
    """the same program under AddressSanitizer and UBSan: the fullest table (every block of the largest robot), the
    differences, bad command lines"""
    exe, plain = _build(tmp_path_factory, 8, sanitize=True), _build(tmp_path_factory, 8)
    d = sl.descriptions(8)
    for name in ("everything", "environment_only", "c4"):
        for reward in (0, 1):
            assert sl._run(exe, "table", *_args(d[name], 1, 8, reward)) == sl._run(plain, "table", *_args(d[name], 1, 8, reward))
    assert sl._run(exe, "diff", *_args(d["everything"], 1, 8, 1), "--", *_args(d["everything"], 1, 8, 0)).strip() == "differ block reward_state"
    assert sl._run(exe, "consts") == sl._run(plain, "consts")
    for bad in (["table"], ["table", 1, 0], ["diff"] + _args(d["c2"]), ["table"] + _args(d["c2"]) + [1, 2, 3]):
        r = subprocess.run([exe] + [str(a) for a in bad], capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
