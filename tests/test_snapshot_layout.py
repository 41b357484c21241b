"""The snapshot banks' row table (csrc/sai2b_snapshot_layout.h) on the CPU: tests/cpp/snapshot_layout_driver.cpp includes the
header alone and is built with plain g++, once per joint count, and once more with -fsanitize=address,undefined and run as the
stand-alone program it is. Checked for hand-written descriptions of C2, C3 with both generator modes, C4, the 8-joint hierarchy
and each optional feature: the rows are the constants of sai2b_params.h, the words are contiguous and do not overlap, the
4-byte blocks are istate, popc_i and the step counter, and the fingerprint changes under every single-field change of the
description and under nothing else."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "snapshot_layout_driver.cpp")
SAN = "-fsanitize=address,undefined"
EPISODE, ENVIRONMENT = 1, 2
JT, MFT = 1, 2  # enum sai2b_task_type; checked against the driver's `consts`

_built = {}


def _build(tmp_factory, n, sanitize=False):
    key = (n, sanitize)
    if key not in _built:
        exe = os.path.join(str(tmp_factory.mktemp(f"snap{n}{'s' if sanitize else ''}")), "snapshot_layout_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DSAI2B_N={n}", "-I", CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[4:4] = [SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[key] = exe
    return _built[key]


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r.stdout


def _consts(exe):
    return {k: int(v) for k, v in (line.split() for line in _run(exe, "consts").splitlines())}


def task(kind, k0=0, otg_mode=0, otg3=0, popc=0, nprec=0):
    return dict(kind=kind, k0=k0, otg_mode=otg_mode, otg3=otg3, popc=popc, nprec=nprec)


def desc(tasks, what=EPISODE, steps=0, contact=0, joint=0, wrench=0, payload=0, plant_payload=0):
    return dict(what=what, steps=steps, contact=contact, joint=joint, wrench=wrench, payload=payload, plant_payload=plant_payload,
                tasks=[dict(t) for t in tasks])


HEAD = ("what", "steps", "contact", "joint", "wrench", "payload", "plant_payload")
TASK = ("kind", "k0", "otg_mode", "otg3", "popc", "nprec")


def _args(d):
    return [d[k] for k in HEAD] + [t[k] for t in d["tasks"] for k in TASK]


def _table(exe, d):
    rows, tail = [], None
    for line in _run(exe, "table", *_args(d)).splitlines():
        f = line.split()
        if f[0] == "row":
            rows.append(dict(block=f[2], task=int(f[3]), rows=int(f[4]), elem=int(f[5]), word=int(f[6]), first_row=int(f[7])))
        else:
            tail = dict(words=int(f[1]), rows=int(f[3]), fingerprint=f[5])
    return rows, tail


def descriptions(n):
    """name -> description, for robots of n joints"""
    everything = dict(steps=1, contact=1, joint=1, wrench=1, payload=1, plant_payload=1)
    out = {
        "c2": desc([task(MFT)]),
        "c3": desc([task(MFT), task(JT, n)]),
        "c3_acc": desc([task(MFT, otg_mode=1), task(JT, n, otg_mode=1)]),
        "c3_jerk": desc([task(MFT, otg_mode=2, otg3=1), task(JT, n, otg_mode=2, otg3=1)]),
        "c4": desc([task(MFT), task(JT, 2), task(JT, n)]),
        "force_popc": desc([task(MFT, popc=1), task(JT, n)]),
        "task_level": desc([task(MFT, nprec=1), task(JT, n, nprec=1)]),
        "steps": desc([task(MFT), task(JT, n)], steps=1),
        "contact": desc([task(MFT), task(JT, n)], what=EPISODE | ENVIRONMENT, contact=1),
        "joint": desc([task(MFT), task(JT, n)], what=EPISODE | ENVIRONMENT, joint=1),
        "wrench": desc([task(MFT), task(JT, n)], what=EPISODE | ENVIRONMENT, wrench=1),
        "payloads": desc([task(MFT), task(JT, n)], what=EPISODE | ENVIRONMENT, payload=1, plant_payload=1),
        "environment_only": desc([], what=ENVIRONMENT, **{k: v for k, v in everything.items() if k != "steps"}),
        "everything": desc([task(MFT, otg_mode=2, otg3=1, popc=1, nprec=1), task(JT, 2, otg_mode=1), task(JT, n, otg_mode=2, otg3=1)],
                           what=EPISODE | ENVIRONMENT, **everything),
    }
    return out


def expected_rows(c, d):
    """{(block, task): (rows, elem bytes)} from the constants of sai2b_params.h alone"""
    n, exp = c["N"], {}
    if d["what"] & EPISODE:
        for blk in ("q", "dq", "tau", "q_pose"):
            exp[(blk, -1)] = (n, 8)
        for t, k in enumerate(d["tasks"]):
            mft = k["kind"] == MFT
            goal = c["MFT_GOAL_ROWS"] if mft else 3 * k["k0"]
            exp[("goals", t)] = exp[("otg_desired", t)] = (goal, 8)
            exp[("state", t)] = (c["MFT_STATE_ROWS"] if mft else k["k0"], 8)
            exp[("otg_state", t)] = (c["OTG_ROWS"], 8)
            if mft:
                exp[("sensed", t)] = (6, 8)
                exp[("istate", t)] = (c["MFT_ISTATE_ROWS"], 4)
            if k["otg3"]:
                exp[("otg3_traj", t)] = (c["OTG_MD"] * c["OTG3_STRIDE"], 8)
            if k["popc"]:
                exp[("popc_f", t)], exp[("popc_i", t)], exp[("popc_q", t)] = (4, 8), (3, 4), (c["POPC_RING"], 8)
            if k["nprec"]:
                exp[("N_prec", t)] = (n * n, 8)
        if d["steps"]:
            exp[("episode_step", -1)] = (1, 4)
        if d["wrench"]:
            exp[("wrench_remaining", -1)], exp[("wrench_status", -1)] = (1, 8), (6 + n, 8)
        if d["contact"]:
            exp[("contact_status", -1)] = (c["CONTACT_STATUS_ROWS"], 8)
        if d["joint"]:
            exp[("joint_status", -1)] = (3 * n, 8)
    if d["what"] & ENVIRONMENT:
        if d["payload"]:
            exp[("payload", -1)] = (c["PAYLOAD_ROWS"], 8)
        if d["plant_payload"]:
            exp[("plant_payload", -1)] = (c["PAYLOAD_ROWS"], 8)
        if d["contact"]:
            exp[("contact", -1)] = (c["CONTACT_ROWS"], 8)
        if d["joint"]:
            exp[("joint_dynamics", -1)] = (6 * n, 8)
        if d["wrench"]:
            exp[("external_wrench", -1)] = (6, 8)
    return exp


@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_tables(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    c = _consts(exe)
    assert (c["N"], c["JOINT_TASK"], c["MOTION_FORCE_TASK"]) == (n, JT, MFT)
    for name, d in descriptions(n).items():
        rows, tail = _table(exe, d)
        assert len(rows) <= c["MAX_TABLE"], name
        got = {(r["block"], r["task"]): (r["rows"], r["elem"]) for r in rows}
        assert len(got) == len(rows), f"{name}: a block appears twice"
        assert got == expected_rows(c, d), name
        # contiguous, non-overlapping, 8-byte blocks on even words; the rows count up alike
        word = row = 0
        for r in rows:
            assert (r["word"], r["first_row"]) == (word, row), (name, r)
            if r["elem"] == 8:
                assert r["word"] % 2 == 0, (name, r)
            word += r["rows"] * r["elem"] // 4
            row += r["rows"]
        assert (tail["words"], tail["rows"]) == (word, row), name
        assert {r["block"] for r in rows if r["elem"] == 4} <= {"istate", "popc_i", "episode_step"}, name
        assert all(r["elem"] == 4 for r in rows if r["block"] in ("istate", "popc_i", "episode_step")), name


def _single_field_changes(d):
    """every description that differs from d in exactly one field"""
    for k in HEAD:
        for v in ((1, 2, 3) if k == "what" else (0, 1)):
            if v != d[k]:
                e = desc(d["tasks"], **{h: d[h] for h in HEAD})
                e[k] = v
                yield f"{k}={v}", e
    for t in range(len(d["tasks"])):
        for k in TASK:
            for v in {"kind": (JT, MFT), "k0": (0, 1, 2, 3), "otg_mode": (0, 1, 2)}.get(k, (0, 1)):
                if v != d["tasks"][t][k]:
                    e = desc(d["tasks"], **{h: d[h] for h in HEAD})
                    e["tasks"][t][k] = v
                    yield f"task{t}.{k}={v}", e
    if len(d["tasks"]) > 1:
        yield "one task fewer", desc(d["tasks"][:-1], **{h: d[h] for h in HEAD})
    if len(d["tasks"]) < 4:
        yield "one task more", desc(d["tasks"] + [task(JT, 1)], **{h: d[h] for h in HEAD})


@pytest.mark.parametrize("n", [7, 8])
def test_fingerprint(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    for name, d in descriptions(n).items():
        base = _table(exe, d)[1]["fingerprint"]
        assert _table(exe, desc(d["tasks"], **{h: d[h] for h in HEAD}))[1]["fingerprint"] == base, f"{name}: not a function of the description"
        assert _run(exe, "diff", *_args(d), "--", *_args(d)).strip() == "same", name
        seen = {base: "the description itself"}
        for what, e in _single_field_changes(d):
            fp = _table(exe, e)[1]["fingerprint"]
            assert fp not in seen, f"{name}: {what} has the fingerprint of {seen[fp]}"
            seen[fp] = what
            out = _run(exe, "diff", *_args(d), "--", *_args(e)).strip()
            assert out.startswith("differ block "), (name, what, out)
    # the joint count is part of it
    other = _build(tmp_path_factory, 6)
    d = descriptions(6)["c2"]
    assert _table(exe, d)[1]["fingerprint"] != _table(other, d)[1]["fingerprint"]


def test_difference_names_the_block(tmp_path_factory):
    exe = _build(tmp_path_factory, 7)
    d = descriptions(7)
    diff = lambda a, b: _run(exe, "diff", *_args(a), "--", *_args(b)).strip()  # noqa: E731
    assert "otg_state of task 0" in diff(d["c3_acc"], d["c3_jerk"]) and "generator mode" in diff(d["c3_acc"], d["c3_jerk"])
    assert "goals of task 1" in diff(d["c3"], d["c2"])
    assert "popc_f of task 0" in diff(d["c3"], d["force_popc"])
    assert "block episode_step" in diff(d["c3"], d["steps"])
    both = desc(d["c3"]["tasks"], what=EPISODE | ENVIRONMENT)
    assert "block contact_status" in diff(both, d["contact"])
    assert "block payload" in diff(both, d["payloads"])


def test_sanitized_driver(tmp_path_factory):
    """the same program under AddressSanitizer and UBSan: the fullest table, every difference, bad command lines"""
    exe = _build(tmp_path_factory, 8, sanitize=True)
    d = descriptions(8)
    plain = _build(tmp_path_factory, 8)
    for name in ("everything", "environment_only", "c4"):
        assert _run(exe, "table", *_args(d[name])) == _run(plain, "table", *_args(d[name]))
    for what, e in _single_field_changes(d["everything"]):
        assert _run(exe, "diff", *_args(d["everything"]), "--", *_args(e)).startswith("differ block "), what
    for bad in (["table"], ["table", 1, 0], ["diff", 1, 0, 0, 0, 0, 0, 0], ["table"] + _args(d["c2"]) + [1, 2, 3]):
        r = subprocess.run([exe] + [str(a) for a in bad], capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
