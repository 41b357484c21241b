"""CPU-only checks of the episode sampler (include/sai2b.h "episode starts"):

1: tests/cpp/reset_sampler_driver.cpp (the shared draw header csrc/sai2b_reset_draw.h under plain g++, and once more under
   -fsanitize=address,undefined as the stand-alone program it is) against tests/reset_sampler_reference.py on 10 000 random
   (counter, rows) inputs: candidate q, goal offsets and joint-goal offsets bit-equal; dq and the goal rotation within 4e-15
   relative (log, sin, cos of two maths libraries; the hardware test's bound for the normals).
2: the host-only entry points through ctypes: defaults, every rejection with its message, the size of the ctypes mirror.
3: the row layout for 4, 6, 7 and 8 joints and mixed goal_tasks, the library against the driver against the restatement; the
   host checks of rows given as a host array (csrc/sai2b_reset_sampler_layout.h through the driver), every message, for mixed
   goal_tasks, also under the sanitizers.
4: the snapshot layout: the new block's position; without the sampler the table and fingerprint of every description are what
   the header gave before the feature (tests/golden/snapshot_layout_before_reset_sampler.json, recorded from the header of the
   commit before it with tests/cpp/reward_layout_driver.cpp).
5: the distribution of 200 000 draws of the shared header through the driver: moments of the uniform candidates, mean and
   covariance of the goal axis within 5 standard errors of isotropy."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import reset_sampler_reference as rr
import sai2_primitives_perso_amd as pkg
import test_reward_snapshot_layout as rl
import test_snapshot_layout as sl
from sai2_primitives_perso_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "cpp", "reset_sampler_driver.cpp")
GOLDEN = os.path.join(HERE, "golden", "snapshot_layout_before_reset_sampler.json")
HEAD = rl.HEAD + ("reset_sampler",)
REL = 4e-15

_built = {}


def _build(tmp_factory, n, sanitize=False):
    key = (n, sanitize)
    if key not in _built:
        exe = os.path.join(str(tmp_factory.mktemp(f"rs{n}{'s' if sanitize else ''}")), "reset_sampler_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSAI2B_N={n}", "-I", sl.CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[4:4] = [sl.SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[key] = exe
    return _built[key]


# ---------------------------------------------------------------------------------------------- 1: the draws
def _records(R, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2**32, (R, 6), dtype=np.uint64).astype(np.uint32)
    c[:, 0] %= 64  # try index / task index
    c[:, 2] %= 2   # call
    c[: R // 8, 1:4] = 0
    c[R // 8 : R // 4, 3] = 0xFFFFFFFF
    v = np.empty((R, 32))
    v[:, 0:4] = rng.uniform(-3, 3, (R, 4))
    v[:, 4:8] = v[:, 0:4] + rng.uniform(0, 3, (R, 4)) * (rng.uniform(size=(R, 4)) < 0.8)  # some lower == upper
    v[:, 8:12] = rng.uniform(0, 2, (R, 4)) * (rng.uniform(size=(R, 4)) < 0.7)  # some sigma == 0
    v[:, 12:15] = rng.uniform(-0.5, 0, (R, 3))
    v[:, 15:18] = rng.uniform(0, 0.5, (R, 3))
    v[:, 18] = rng.uniform(0, np.pi, R)
    w = rng.normal(size=(R, 3))
    v[:, 19:28] = pkg.workloads._expmap(w).reshape(R, 9)
    v[:, 28:32] = rng.uniform(0, 1, (R, 4))
    return c, v


def _reference(c, v):
    n, e, call, robot = (c[:, k].astype(np.int64) for k in range(4))
    out = np.empty((len(c), 24))
    # (every record has its own key: the restatement's pieces are called with the key words instead of one seed)
    key = (c[:, 4].astype(np.uint64), c[:, 5].astype(np.uint64))

    def u4(stream, cl):
        wds = rr.hr.philox4x32_10((n, e, 256 * stream + cl, robot), key)
        return (wds.astype(np.float64) + 0.5) * 2.0**-32

    u = u4(rr.CANDIDATE, call)
    out[:, 0:4] = (v[:, 0:4].T + (v[:, 4:8].T - v[:, 0:4].T) * u).T
    wds = rr.hr.philox4x32_10((np.zeros_like(n), e, 256 * rr.VELOCITY + call, robot), key)
    z = np.stack([*rr.hr.box_muller(wds[0], wds[1]), *rr.hr.box_muller(wds[2], wds[3])])
    sig = v[:, 8:12].T
    out[:, 4:8] = np.where(sig != 0, sig * z, 0.0).T
    g0, g1 = u4(rr.GOAL, 0), u4(rr.GOAL, 1)
    out[:, 8:11] = (v[:, 12:15].T + (v[:, 15:18].T - v[:, 12:15].T) * g0[:3]).T
    _, D = rr.axis_rotation(v[:, 18] * g0[3], g1[0], g1[1])
    out[:, 11:20] = rr.rotate(np.ascontiguousarray(v[:, 19:28].T), D).T
    out[:, 20:24] = (v[:, 28:32].T * (2.0 * u4(rr.GOAL, call) - 1.0)).T
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_draws_of_the_shared_header(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, 7, sanitize)
    c, v = _records(10000, 20261020)
    paths = [str(tmp_path / name) for name in ("c.u32", "v.f64", "o.f64")]
    c.tofile(paths[0]), v.tofile(paths[1])
    r = subprocess.run([exe, "draws"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = np.fromfile(paths[2]).reshape(-1, 24), _reference(c, v)
    for name, cols in (("candidate q", slice(0, 4)), ("goal offset", slice(8, 11)), ("joint goal offset", slice(20, 24))):
        assert np.array_equal(got[:, cols], want[:, cols]), name
    same = v[:, 0:4] == v[:, 4:8]
    assert same.any() and np.array_equal(got[:, 0:4][same], v[:, 0:4][same])  # lower == upper gives lower
    zero = v[:, 8:12] == 0
    assert zero.any() and not got[:, 4:8][zero].any() and not np.signbit(got[:, 4:8][zero]).any()
    for name, cols, floor in (("dq", slice(4, 8), 1e-300), ("goal rotation", slice(11, 20), 1.0)):
        scale = np.maximum(np.abs(want[:, cols]), floor)  # (a rotation's elements are sums of terms of order 1)
        assert (np.abs(got[:, cols] - want[:, cols]) <= REL * scale).all(), name
    assert subprocess.run([exe, "draws", paths[0], paths[0], paths[2]], capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- 2: configuration
def _lib():
    return _abi.load_library()


def _default():
    cfg = _abi.ResetSamplerConfig()
    assert _lib().sai2b_default_reset_sampler(C.byref(cfg)) == _abi.OK
    return cfg


def _tasks(dof=7):
    """[MotionForceTask, JointTask, MotionForceTask, JointTask of 2 rows]"""
    sel = np.zeros((2, dof))
    sel[0, 0] = sel[1, dof - 1] = 1
    return [pkg.motion_force_task_config("m", robot_dof=dof, link=dof - 1), pkg.joint_task_config("j", robot_dof=dof),
            pkg.motion_force_task_config("n", robot_dof=dof, link=dof - 2), pkg.joint_task_config("p", sel, robot_dof=dof)]


def _validate(cfg, tasks, dof=7):
    arr = (_abi.TaskConfig * len(tasks))(*tasks)
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_reset_sampler(None if cfg is None else C.byref(cfg), arr, len(tasks), dof, msg, 256)
    return rc, msg.value.decode()


def test_defaults_and_the_size_of_the_mirror():
    cfg = _default()
    assert (cfg.seed, cfg.first_robot, cfg.max_tries, cfg.goal_tasks, cfg.absolute_position) == (0, 0, 8, 0, 0)
    assert (cfg.ratio_task, cfg.box_task, cfg.use_clearance) == (-1, -1, 0) and _abi.MAX_RESET_TRIES == 64
    assert _lib().sai2b_sizeof_reset_sampler_config() == C.sizeof(_abi.ResetSamplerConfig)
    assert _validate(cfg, _tasks()) == (_abi.OK, "")
    assert "sai2b_reset_robots_sampled" in _abi.EXPORTS and _abi.SNAP_BLOCKS[-1] == "reset_sampler_episode"


REJECTED = [
    (dict(max_tries=0), "max_tries must be in"),
    (dict(max_tries=65), "max_tries must be in"),
    (dict(goal_tasks=1 << 4), "goal_tasks names a task"),
    (dict(goal_tasks=1, absolute_position=2), "absolute_position names a task that is not a MotionForceTask of goal_tasks"),
    (dict(goal_tasks=0, absolute_position=1), "absolute_position names a task that is not a MotionForceTask of goal_tasks"),
    (dict(ratio_task=1), "ratio_task must be -1 or the index of a MotionForceTask"),
    (dict(ratio_task=4), "ratio_task must be -1 or the index of a MotionForceTask"),
    (dict(ratio_task=0, min_ratio=1.5), "min_ratio must be in"),
    (dict(ratio_task=0, min_ratio=float("nan")), "min_ratio must be in"),
    (dict(box_task=3), "box_task must be -1 or the index of a MotionForceTask"),
    (dict(box_task=2, box_lower=(0.0, float("inf"), 0.0)), "the box must be finite"),
    (dict(use_clearance=2), "use_clearance must be 0 or 1"),
    (dict(use_clearance=1, clearance=float("nan")), "clearance must be finite"),
]


@pytest.mark.parametrize("edit, message", REJECTED)
def test_every_rejected_configuration_gives_its_message(edit, message):
    cfg = _default()
    for k, v in edit.items():
        if k.startswith("box_l") or k.startswith("box_u"):
            getattr(cfg, k)[:] = v
        else:
            setattr(cfg, k, v)
    rc, msg = _validate(cfg, _tasks())
    assert rc == _abi.INVALID_ARGUMENT and message in msg
    assert _validate(None, _tasks())[1] == "reset sampler: null config"
    assert _validate(_default(), _tasks(), dof=9)[0] != _abi.OK  # no build for nine joints


# ---------------------------------------------------------------------------------------------- 3: row layout
@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_row_layout(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    tasks = _tasks(n)
    arr = (_abi.TaskConfig * 4)(*tasks)
    kinds = [("mft",), ("jt", n, None), ("mft",), ("jt", 2, None)]
    for goal_tasks in range(16):
        cfg = _default()
        cfg.goal_tasks = goal_tasks
        first, rows, total = C.c_int(), C.c_int(), C.c_int()
        want, want_total = rr.layout(n, kinds, goal_tasks)
        got = {}
        for t in range(4):
            assert _lib().sai2b_reset_sampler_config_layout(C.byref(cfg), arr, 4, n, 4, t, C.byref(first), C.byref(rows), C.byref(total)) == _abi.OK
            if rows.value:
                got[t] = first.value
                assert rows.value == (7 if kinds[t][0] == "mft" else kinds[t][1])
            else:
                assert first.value == -1
        assert got == want and total.value == want_total
        for block in range(4):
            assert _lib().sai2b_reset_sampler_config_layout(C.byref(cfg), arr, 4, n, block, 0, C.byref(first), C.byref(rows), None) == _abi.OK
            assert (first.value, rows.value) == (block * n, n)
        out = sl._run(exe, "rows", goal_tasks, *[x for t in tasks for x in (t.type, t.task_dof)]).split()
        assert int(out[-1]) == want_total and {int(out[i + 1]): int(out[i + 2]) for i in range(0, len(out) - 2, 4)} == want
    # the MotionForceTasks' rows stand ahead of the JointTasks'
    assert rr.layout(n, kinds, 0b1111)[0] == {0: 4 * n, 2: 4 * n + 7, 1: 4 * n + 14, 3: 5 * n + 14}
    assert _lib().sai2b_reset_sampler_config_layout(C.byref(cfg), arr, 4, n, 5, 0, None, None, None) == _abi.INVALID_ARGUMENT


@pytest.mark.parametrize("n, sanitize", [(4, False), (7, False), (8, True)])
def test_host_checks_of_the_rows(tmp_path_factory, tmp_path, n, sanitize):
    """csrc/sai2b_reset_sampler_layout.h: every rejection of rows given as a host array with its message, for every mixture of
    goal_tasks: the theta_max row of each MotionForceTask's block and every row of each JointTask's block are found where the
    layout puts them, and no other goal row is held to a sign"""
    exe = _build(tmp_path_factory, n, sanitize)
    B = 3
    kinds = [("mft",), ("jt", n, None), ("mft",), ("jt", 2, None)]
    types = [x for k in kinds for x in ((_abi.MOTION_FORCE_TASK, 0) if k[0] == "mft" else (_abi.JOINT_TASK, k[1]))]
    path = str(tmp_path / "rows.f64")

    def check(goal_tasks, rows):
        rows.tofile(path)
        return sl._run(exe, "rowcheck", goal_tasks, B, path, *types).strip()

    for goal_tasks in (0, 1, 2, 5, 10, 15):
        first, total = rr.layout(n, kinds, goal_tasks)
        good = rr.default_rows(n, np.full(n, -3.0), np.full(n, 3.0), total, B)
        for t, f in first.items():
            if kinds[t][0] == "mft":
                good[f : f + 3], good[f + 3 : f + 6], good[f + 6] = 0.2, -0.1, np.pi  # a box of either order, the largest angle
            else:
                good[f : f + kinds[t][1]] = 0.0
        assert check(goal_tasks, good) == "ok"

        def bad(row, value, col=1):
            r = good.copy()
            r[row, col] = value
            return check(goal_tasks, r)

        assert "finite" in bad(total - 1, np.nan) and "finite" in bad(0, np.inf)
        assert "q_lower must not exceed q_upper" in bad(0, 2.9) and "q_lower must not exceed q_upper" in bad(2 * n - 1, -2.9)
        assert "dq_sigma must not be negative" in bad(2 * n, -1e-9) and "dq_sigma must not be negative" in bad(3 * n - 1, -1.0)
        assert "q_nominal must lie within" in bad(3 * n, 3.5) and "q_nominal must lie within" in bad(4 * n - 1, -3.5)
        for t, f in first.items():
            if kinds[t][0] == "mft":
                assert "theta_max must be in" in bad(f + 6, np.nextafter(np.pi, 4.0)) and "theta_max must be in" in bad(f + 6, -1e-12)
                assert all(bad(f + k, -5.0) == "ok" for k in range(6))  # the position box is not held to a sign or an order
            else:
                for k in (0, kinds[t][1] - 1):
                    assert "half_width must not be negative" in bad(f + k, -1e-12)
    r = subprocess.run([exe, "rowcheck", "15", str(B), path] + [str(x) for x in types], capture_output=True, text=True)
    assert r.returncode == 0
    r = subprocess.run([exe, "rowcheck", "1", str(B), path] + [str(x) for x in types], capture_output=True, text=True)
    assert r.returncode == 2  # (the file holds the rows of the last mixture: another mixture has another row count)


# ---------------------------------------------------------------------------------------------- 4: snapshot layout
def _args(d, hardware=0, depth=0, reward=0, sampler=0):
    d = dict(d, hardware=hardware, hardware_depth=depth, reward=reward, reset_sampler=sampler)
    return [d[k] for k in HEAD] + [t[k] for t in d["tasks"] for k in sl.TASK]


def _table(exe, d, **kw):
    rows, tail = [], None
    for line in sl._run(exe, "table", *_args(d, **kw)).splitlines():
        f = line.split()
        if f[0] == "row":
            rows.append(dict(block=f[2], task=int(f[3]), rows=int(f[4]), elem=int(f[5]), word=int(f[6]), first_row=int(f[7])))
        else:
            tail = dict(words=int(f[1]), rows=int(f[3]), fingerprint=f[5])
    return rows, tail


@pytest.mark.parametrize("n", [4, 7, 8])
def test_the_new_snapshot_block(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["everything"]
    for hw, rew in ((dict(), 0), (dict(hardware=1, depth=8), 1)):
        rows, tail = _table(exe, d, reward=rew, sampler=1, **hw)
        base, base_tail = _table(exe, d, reward=rew, **hw)
        assert len(rows) == len(base) + 1
        new = rows[-1]
        assert (new["block"], new["rows"], new["elem"], new["task"]) == ("reset_sampler_episode", 1, 4, -1)  # the last 4-byte block
        assert [(r["block"], r["task"], r["rows"], r["word"]) for r in rows[:-1]] == [(r["block"], r["task"], r["rows"], r["word"]) for r in base]
        assert tail["words"] == base_tail["words"] + 1 and tail["fingerprint"] != base_tail["fingerprint"]
        consts = {k: int(v) for k, v in (line.split() for line in sl._run(exe, "consts").splitlines())}
        assert len(rows) <= consts["CAPACITY"] and consts["CAPACITY"] == consts["MAX_TABLE"] + 1 and consts["BLOCKS"] == 34

        def diff(a, b):
            return sl._run(exe, "diff", *_args(d, reward=rew, sampler=a, **hw), "--", *_args(d, reward=rew, sampler=b, **hw)).strip()

        assert diff(1, 1) == "same" and diff(0, 1) == "differ block reset_sampler_episode" == diff(1, 0)
    env, _ = _table(exe, sl.descriptions(n)["environment_only"], sampler=0)
    assert not [r for r in env if r["block"].startswith("reset_sampler")]


@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_without_the_sampler_the_layout_is_what_it_was(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    golden = json.load(open(GOLDEN))[str(n)]
    descs = sl.descriptions(n)
    assert len(golden) == 4 * len(descs)
    for name, d in descs.items():
        for hs, hw in rl.HARDWARE.items():
            for rs, rew in (("", 0), ("+rew", 1)):
                rows, tail = _table(exe, d, hardware=hw[0], depth=hw[1], reward=rew)
                g = golden[name + hs + rs]
                assert [[r["block"], r["task"], r["rows"], r["elem"], r["word"], r["first_row"]] for r in rows] == g["rows"], name + hs + rs
                assert (tail["words"], tail["rows"], tail["fingerprint"]) == (g["words"], g["total_rows"], g["fingerprint"]), name + hs + rs


def test_sanitized_tables(tmp_path_factory):
    exe, plain = _build(tmp_path_factory, 8, sanitize=True), _build(tmp_path_factory, 8)
    d = sl.descriptions(8)
    for name in ("everything", "c4"):
        for s in (0, 1):
            a = _args(d[name], hardware=1, depth=8, reward=1, sampler=s)
            assert sl._run(exe, "table", *a) == sl._run(plain, "table", *a)
    assert sl._run(exe, "rows", 15, 2, 0, 1, 8, 2, 0, 1, 2) == sl._run(plain, "rows", 15, 2, 0, 1, 8, 2, 0, 1, 2)


# ---------------------------------------------------------------------------------------------- 5: distribution
def test_distribution_of_the_draws(tmp_path_factory, tmp_path):
    """200 000 draws of the shared header (csrc/sai2b_reset_draw.h through the driver): moments of the uniform candidates, mean and
    covariance of the goal axis within 5 standard errors of isotropy; the restatement gives the same candidates bit for bit"""
    exe = _build(tmp_path_factory, 7)
    R, seed = 200000, 12345
    c = np.zeros((R, 6), dtype=np.uint32)
    c[:, 1], c[:, 3], c[:, 4], c[:, 5] = np.arange(R) % 7, np.arange(R), seed & 0xFFFFFFFF, seed >> 32
    v = np.zeros((R, 32))
    v[:, 0:4], v[:, 4:8] = [-2.0, 0.5, 1.0, -1e-3], [1.0, 0.75, 1.0, 1e3]
    v[:, 18] = 1.0  # theta = u in (0, 1): sin(theta) > 0, so the antisymmetric part of the rotation points along the axis
    v[:, 19:28] = np.eye(3).reshape(9)
    paths = [str(tmp_path / name) for name in ("c.u32", "v.f64", "o.f64")]
    c.tofile(paths[0]), v.tofile(paths[1])
    r = subprocess.run([exe, "draws"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(paths[2]).reshape(R, 24)
    q, lower, upper = out[:, 0:4].T, v[:, 0:4].T, v[:, 4:8].T
    assert np.array_equal(q, rr.candidate(np.zeros(R, dtype=np.int64), c[:, 1].astype(np.int64), np.arange(R), seed, lower, upper))
    w = upper[:, 0] - lower[:, 0]
    assert (np.abs(q.mean(axis=1) - 0.5 * (lower[:, 0] + upper[:, 0])) <= 5 * w / np.sqrt(12 * R)).all()
    # the variance of a uniform: w^2 / 12, its standard error w^2 sqrt(1 / 180 R) (fourth central moment w^4 / 80)
    assert (np.abs(q.var(axis=1) - w * w / 12) <= 5 * w * w * np.sqrt(1 / (180 * R))).all()
    assert (q >= lower).all() and (q <= upper).all() and np.array_equal(q[2], lower[2])
    D = out[:, 11:20]
    axis = np.stack([D[:, 7] - D[:, 5], D[:, 2] - D[:, 6], D[:, 3] - D[:, 1]])
    axis /= np.linalg.norm(axis, axis=0)
    # isotropy: mean 0 with variance 1/3 per component; E[a_i a_j] = delta_ij / 3 with variances 4/45 (i = j) and 1/15 (i != j)
    assert (np.abs(axis.mean(axis=1)) <= 5 * np.sqrt(1 / (3 * R))).all()
    cov = axis @ axis.T / R
    for i in range(3):
        for j in range(3):
            sd = np.sqrt((4 / 45 if i == j else 1 / 15) / R)
            assert abs(cov[i, j] - (1 / 3 if i == j else 0.0)) <= 5 * sd, (i, j)
    Dm = D.reshape(R, 3, 3)
    assert np.abs(Dm @ np.transpose(Dm, (0, 2, 1)) - np.eye(3)).max() < 1e-14
    # the angle is theta_max u with u uniform: trace = 1 + 2 cos(theta), mean of theta 1/2 within 5 standard errors
    theta = np.arccos(np.clip((np.einsum("rii->r", Dm) - 1) / 2, -1, 1))
    assert abs(theta.mean() - 0.5) <= 5 * np.sqrt(1 / (12 * R)) and theta.max() < 1.0
