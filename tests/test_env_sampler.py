"""CPU-only checks of the environment sampler (include/sai2b.h "environment sampler"):

1: tests/cpp/env_sampler_driver.cpp (the shared draw header csrc/sai2b_env_draw.h under plain g++ -ffp-contract=off, and once
   more under -fsanitize=address,undefined as the stand-alone program it is) against tests/env_sampler_reference.py on 10 000
   random (counter, key, nominal, range) records: every affine and product result and both integer draws bit-equal; log-uniform
   scales (and what is multiplied by them), the tilted normal and the push directions (and the push rows) within 4e-15 relative
   (log, exp, sin, cos of two maths libraries; the bound of tests/test_reset_sampler.py and tests/test_hardware_reference.py).
2: the host-only entry points through ctypes: defaults, the size of the ctypes mirror, every rejection with its message.
3: the sample-row layout for 4, 6, 7 and 8 joints and all 32 group sets: library, driver and restatement agree.
4: the snapshot layout: the two new blocks' positions; without the sampler the table and fingerprint of every description are
   what the header gave before the feature (tests/golden/snapshot_layout_before_env_sampler.json, recorded from the header of
   the commit before it with tests/cpp/reset_sampler_driver.cpp: per description the number of blocks, words, rows, the
   fingerprint and a SHA-256 of the driver's "row" lines).
5: the distribution of 200 000 draws through the driver: mean and variance of a uniform and of a log-uniform scale, the
   frequencies of a delay range [1, 4], mean and covariance of the push direction, each within 5 standard errors."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import env_sampler_reference as er
import test_reset_sampler as trs
import test_reward_snapshot_layout as rl
import test_snapshot_layout as sl
from sai2_primitives_perso_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "cpp", "env_sampler_driver.cpp")
GOLDEN = os.path.join(HERE, "golden", "snapshot_layout_before_env_sampler.json")
HEAD = trs.HEAD + ("env_sampler",)
REL = 4e-15
IN, OUT = 102, 84

_built = {}


def _build(tmp_factory, n, sanitize=False):
    key = (n, sanitize)
    if key not in _built:
        exe = os.path.join(str(tmp_factory.mktemp(f"es{n}{'s' if sanitize else ''}")), "env_sampler_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSAI2B_N={n}", "-I", sl.CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[4:4] = [sl.SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[key] = exe
    return _built[key]


def _draw(exe, tmp_path, c, v):
    paths = [str(tmp_path / name) for name in ("c.u32", "v.f64", "o.f64")]
    np.ascontiguousarray(c, dtype=np.uint32).tofile(paths[0]), np.ascontiguousarray(v, dtype=np.float64).tofile(paths[1])
    r = subprocess.run([exe, "draws"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(paths[2]).reshape(-1, OUT), paths


# ---------------------------------------------------------------------------------------------- 1: the draws
def _records(R, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2**32, (R, 4), dtype=np.uint64).astype(np.uint32)
    c[: R // 8, 0:2] = 0  # counter words 0 ...
    c[R // 8 : R // 4, 0] = 0xFFFFFFFF  # ... and 0xFFFFFFFF
    c[R // 8 : R // 4 : 2, 1] = 0xFFFFFFFF
    v = np.zeros((R, IN))
    for k in range(15):
        log = (rng.uniform(size=R) < 0.3) & (k != 1)
        lo = np.where(log, rng.uniform(0.05, 2.0, R), rng.uniform(0.0, 2.0, R))
        if k == 1:  # contact_height: an offset, either sign
            lo = rng.uniform(-0.1, 0.1, R)
        w = rng.uniform(0.0, 1.5, R) * (rng.uniform(size=R) < 0.8)  # some lower == upper
        v[:, 3 * k], v[:, 3 * k + 1], v[:, 3 * k + 2] = lo, lo + w, log
    v[:, 45:48] = rng.uniform(0, 0.1, (R, 3)) * (rng.uniform(size=(R, 3)) < 0.7)  # some zero halves
    v[:, 48] = rng.uniform(0, np.pi, R) * (rng.uniform(size=R) < 0.8)  # some theta == 0
    v[:, 49:55] = rng.uniform(0, 2.0, (R, 6)) * (rng.uniform(size=(R, 6)) < 0.7)
    v[:, 55] = rng.integers(0, 9, R)
    v[:, 56] = v[:, 55] + rng.integers(0, 9, R) * (rng.uniform(size=R) < 0.8)
    v[:, 56] = np.minimum(v[:, 56], 8)
    v[:, 57] = rng.integers(0, 50, R)
    v[:, 58] = v[:, 57] + rng.integers(0, 200, R) * (rng.uniform(size=R) < 0.8)
    nom = v[:, 59:98]
    nom[:, 0] = rng.uniform(0, 3, R)  # payload: mass, com, inertia
    nom[:, 1:4] = rng.uniform(-0.1, 0.1, (R, 3))
    nom[:, 4:10] = rng.uniform(-0.01, 0.02, (R, 6))
    nom[:, 10:13] = rng.uniform(-1, 1, (R, 3))  # contact: point, unit normal, material
    nrm = rng.normal(size=(R, 3))
    nom[:, 13:16] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    nom[:, 16:19] = rng.uniform(0, 1e4, (R, 3))
    nom[:, 19:23] = rng.uniform(0, 50, (R, 4))  # a joint chunk; torque limits may be +inf
    v[:, 98], v[:, 99] = rng.integers(0, 4, R), rng.integers(0, 2, R)
    inf = (v[:, 98] == 3) & (rng.uniform(size=R) < 0.5)
    nom[inf, 19:23] = np.inf
    nom[:, 23:27] = rng.uniform(0.2, 1.0, (R, 4))  # a hardware chunk
    v[:, 100], v[:, 101] = rng.integers(0, 3, R), rng.integers(0, 2, R)
    nom[:, 27:33] = rng.uniform(-1, 1, (R, 6))  # sensor: bias, noise deviation
    nom[:, 33:39] = rng.uniform(0, 0.5, (R, 6))
    return c, v


def _cfg(v):
    """the records' configuration as the restatement takes it: every entry an array over the records"""
    cfg = {name: (v[:, 3 * k], v[:, 3 * k + 1], v[:, 3 * k + 2]) for k, name in enumerate(er.RANGES)}
    cfg.update(payload_com_half=v[:, 45:48].T, contact_tilt_max=v[:, 48], sensor_bias_half=v[:, 49:55].T,
               delay_lower=v[:, 55].astype(np.int64), delay_upper=v[:, 56].astype(np.int64),
               push_steps_lower=v[:, 57].astype(np.int64), push_steps_upper=v[:, 58].astype(np.int64))
    return cfg


def _reference(c, v):
    cnt, robot = c[:, 0].astype(np.int64), c[:, 1].astype(np.int64)
    key = (c[:, 2].astype(np.uint64), c[:, 3].astype(np.uint64))
    cfg, nom = _cfg(v), v[:, 59:98].T
    out = np.empty((OUT, len(c)))
    out[4:14], out[0:4] = er.payload(cfg, cnt, robot, key, nom[0:10])
    out[14:23], out[23:31] = er.contact(cfg, cnt, robot, key, nom[10:19])
    jp, jj, hp, hj = (v[:, k].astype(np.int64) for k in (98, 99, 100, 101))
    s = np.empty((4, len(c)))
    for p in range(4):  # the chunk of parameter p, call 2 p + j
        sel = jp == p
        r = tuple(x[sel] for x in cfg[er.JOINT_RANGES[p]])
        s[:, sel] = er.draw_range(r, er.uniforms4(cnt[sel], 7, 2 * p + jj[sel], robot[sel], (key[0][sel], key[1][sel])))
    out[31:35], out[35:39] = nom[19:23] * s, s
    for p in range(3):
        sel = hp == p
        r = tuple(x[sel] for x in cfg[er.HW_RANGES[p]])
        s[:, sel] = er.draw_range(r, er.uniforms4(cnt[sel], 8, 1 + 2 * p + hj[sel], robot[sel], (key[0][sel], key[1][sel])))
    rows = nom[23:27] * s
    clip = (hp == 0) & (rows > 1.0)
    out[39:43], out[43:47] = np.where(clip, 1.0, rows), s
    out[47] = (clip * (1 << np.arange(4))[:, None]).sum(axis=0)
    act = np.ones((1 + 3 * 4, len(c)))
    _, out[49:61], hs, _ = er.hardware(cfg, cnt, robot, key, act, nom[27:39], 4)
    out[48], out[61:68] = hs[0], hs[13:20]
    out[68:75], out[75:84] = er.push(cfg, cnt, robot, key)
    return out.T


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_draws_of_the_shared_header(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, 7, sanitize)
    c, v = _records(10000, 20261021)
    got, paths = _draw(exe, tmp_path, c, v)
    want = _reference(c, v)
    log = {name: v[:, 3 * k + 2] != 0 for k, name in enumerate(er.RANGES)}
    tilted = v[:, 48] != 0

    def close(a, b, floor):
        with np.errstate(invalid="ignore"):  # (+inf against +inf: equal)
            return (a == b) | (np.abs(a - b) <= REL * np.maximum(np.abs(b), floor))

    def check(name, cols, loose=None, floor=1e-300):
        """bit-equal where `loose` (per record) is false, within REL where it is true"""
        g, w = got[:, cols], want[:, cols]
        loose = np.zeros(len(g), dtype=bool) if loose is None else loose
        assert np.array_equal(g[~loose], w[~loose]), name
        assert close(g[loose], w[loose], floor).all(), name

    check("payload sample", slice(0, 4), log["payload_mass_scale"])
    check("payload rows", slice(4, 14), log["payload_mass_scale"])
    check("contact point", slice(14, 17))
    assert log["contact_height"].sum() == 0
    check("contact normal", slice(17, 20), tilted, floor=1.0)  # (a rotated unit vector: sums of terms of order 1)
    assert (~tilted).any() and np.array_equal(got[~tilted, 17:20], v[~tilted, 72:75])  # theta == 0 keeps n bit for bit
    for k, name in enumerate(("contact_stiffness_scale", "contact_damping_scale", "contact_friction_scale")):
        check(name, [20 + k, 28 + k], log[name])
    check("height and angle", slice(23, 25))
    check("tilt axis", slice(25, 28), np.ones(len(got), dtype=bool), floor=1.0)
    jp, hp = v[:, 98].astype(int), v[:, 100].astype(int)
    jlog = np.choose(jp, [log[n] for n in er.JOINT_RANGES])
    check("joint chunk", slice(31, 39), jlog)
    inf = np.isinf(v[:, 78:82]).all(axis=1)
    assert inf.any() and np.isinf(got[inf, 31:35]).all() and (got[inf, 31:35] > 0).all()  # +inf stays +inf
    hlog = np.choose(hp, [log[n] for n in er.HW_RANGES])
    check("hardware chunk", slice(39, 47), hlog)
    # the clip decision is a comparison with 1: exact where the scale is, and away from ties elsewhere
    tie = hlog & (np.abs(v[:, 82:86] * want[:, 43:47] - 1.0) < 1e-12).any(axis=1)
    assert np.array_equal(got[~tie, 47], want[~tie, 47]) and (got[:, 39:43][hp == 0] <= 1.0).all() and (want[:, 47] > 0).any()
    check("delay", [48])
    assert ((got[:, 48] >= v[:, 55]) & (got[:, 48] <= v[:, 56])).all() and np.array_equal(got[:, 48], np.round(got[:, 48]))
    check("sensor bias", slice(49, 55))
    check("sensor noise", slice(55, 61), log["sensor_noise_scale"])
    check("sensor sample", slice(61, 68), log["sensor_noise_scale"])
    check("push magnitudes and steps", [75, 79], log["push_force"])
    check("push moment magnitude", [80], log["push_moment"])
    everything = np.ones(len(got), dtype=bool)
    check("push directions", [76, 77, 78, 81, 82, 83], everything, floor=1.0)
    scale = np.maximum(np.abs(want[:, [75, 75, 75, 80, 80, 80]]), 1e-300)
    assert (np.abs(got[:, 68:74] - want[:, 68:74]) <= (2 * REL + 2.3e-16) * scale).all()  # magnitude times direction: both may differ, and a rounding
    check("push steps row", [74])
    # lower == upper gives lower, a zero half gives a zero offset
    same = (v[:, 0] == v[:, 1]) & ~log["payload_mass_scale"]
    assert same.any() and np.array_equal(got[same, 0], v[same, 0])
    zero = v[:, 45] == 0
    assert zero.any() and not got[zero, 1].any()
    assert subprocess.run([exe, "draws", paths[0], paths[0], paths[2]], capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------- 2: configuration
def _lib():
    return _abi.load_library()


def _default():
    cfg = _abi.EnvSamplerConfig()
    assert _lib().sai2b_default_env_sampler(C.byref(cfg)) == _abi.OK
    return cfg


def _validate(cfg, dof=7):
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_env_sampler(None if cfg is None else C.byref(cfg), dof, msg, 256)
    return rc, msg.value.decode()


def test_defaults_and_the_size_of_the_mirror():
    cfg = _default()
    assert (cfg.seed, cfg.first_robot, cfg.groups, cfg.payload_target) == (0, 0, 0, _abi.PAYLOAD_PLANT)
    want = er.default_config()
    for name in _abi.ENV_RANGE_FIELDS:
        r = getattr(cfg, name)
        assert (r.lower, r.upper, r.log_uniform) == want[name], name
    assert set(_abi.ENV_RANGE_FIELDS) == set(er.RANGES)
    assert list(cfg.payload_com_half) == [0.0] * 3 and list(cfg.sensor_bias_half) == [0.0] * 6 and cfg.contact_tilt_max == 0.0
    assert (cfg.delay_lower, cfg.delay_upper, cfg.push_steps_lower, cfg.push_steps_upper) == (0, 0, 0, 0)
    assert _lib().sai2b_sizeof_env_sampler_config() == C.sizeof(_abi.EnvSamplerConfig)
    assert _validate(cfg) == (_abi.OK, "")
    assert "sai2b_randomize_robots" in _abi.EXPORTS and _abi.SNAP_BLOCK_NAMES[-2:] == ("env_sampler_counter", "env_sampler_sample")
    assert _abi.BUF_ENV_SAMPLE == 20


def _range(lower, upper, log=0):
    return _abi.EnvRange(lower, upper, log, 0)


REJECTED = [
    (dict(groups=32), "groups holds a bit that is no group"),
    (dict(payload_target=1), "payload_target must be SAI2B_PAYLOAD_PLANT or SAI2B_PAYLOAD_BOTH"),
    (dict(payload_target=0), "payload_target must be"),
    (dict(payload_mass_scale=_range(2.0, 1.0)), "payload_mass_scale: lower must not exceed upper"),
    (dict(contact_height=_range(0.1, -0.1)), "contact_height: lower must not exceed upper"),
    (dict(gain_scale=_range(1.0, float("inf"))), "gain_scale must be finite"),
    (dict(push_force=_range(float("nan"), 1.0)), "push_force must be finite"),
    (dict(damping_scale=_range(-0.5, 1.0)), "damping_scale: lower must not be negative"),
    (dict(push_moment=_range(-1.0, 1.0)), "push_moment: lower must not be negative"),
    (dict(friction_scale=_range(0.0, 1.0, 1)), "friction_scale: a log-uniform range needs lower > 0"),
    (dict(contact_height=_range(-0.1, 0.1, 1)), "contact_height: a log-uniform range needs lower > 0"),
    (dict(armature_scale=_range(1.0, 2.0, 2)), "armature_scale: log_uniform must be 0 or 1"),
    (dict(lag_scale=_range(0.0, 1.0)), "lag_scale: lower must be > 0"),
    (dict(payload_com_half=(0.0, -1e-9, 0.0)), "payload_com_half must be finite and not negative"),
    (dict(sensor_bias_half=(0.0, 0.0, 0.0, 0.0, 0.0, float("inf"))), "sensor_bias_half must be finite and not negative"),
    (dict(contact_tilt_max=-1e-9), "contact_tilt_max must be in [0, pi]"),
    (dict(contact_tilt_max=float(np.nextafter(np.pi, 4.0))), "contact_tilt_max must be in [0, pi]"),
    (dict(contact_tilt_max=float("nan")), "contact_tilt_max must be in [0, pi]"),
    (dict(delay_lower=-1), "the delay must lie in [0, SAI2B_MAX_ACTUATION_DELAY]"),
    (dict(delay_upper=9), "the delay must lie in [0, SAI2B_MAX_ACTUATION_DELAY]"),
    (dict(delay_lower=3, delay_upper=2), "delay_lower must not exceed delay_upper"),
    (dict(push_steps_lower=-1), "push steps must not be negative"),
    (dict(push_steps_lower=5, push_steps_upper=4), "push_steps_lower must not exceed push_steps_upper"),
]


@pytest.mark.parametrize("edit, message", REJECTED)
def test_every_rejected_configuration_gives_its_message(edit, message):
    cfg = _default()
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(cfg, k)[:] = v
        else:
            setattr(cfg, k, v)
    rc, msg = _validate(cfg)
    assert rc == _abi.INVALID_ARGUMENT and message in msg
    assert _validate(None)[1] == "env sampler: null config"
    assert _validate(_default(), dof=9)[0] != _abi.OK  # no build for nine joints


# ---------------------------------------------------------------------------------------------- 3: sample-row layout
@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_sample_row_layout(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    for groups in range(32):
        cfg = _default()
        cfg.groups = groups
        want, want_total = er.layout(groups, n)
        first, rows, total = C.c_int(), C.c_int(), C.c_int()
        got = {}
        for g in er.GROUPS:
            assert _lib().sai2b_env_sampler_config_layout(C.byref(cfg), n, g, C.byref(first), C.byref(rows), C.byref(total)) == _abi.OK
            if rows.value:
                got[g] = (first.value, rows.value)
            else:
                assert first.value == -1
            assert total.value == want_total
        assert got == want
        out = [line.split() for line in sl._run(exe, "layout", groups).splitlines()]
        assert {int(f[1]): (int(f[2]), int(f[3])) for f in out[:-1]} == want and int(out[-1][1]) == want_total
    assert er.layout(31, n) == ({1: (0, 4), 2: (4, 8), 4: (12, 4 * n), 8: (12 + 4 * n, 8 + 3 * n), 16: (20 + 7 * n, 9)}, 29 + 7 * n)
    for bad in (0, 3, 32):
        assert _lib().sai2b_env_sampler_config_layout(C.byref(cfg), n, bad, None, None, None) == _abi.INVALID_ARGUMENT
    assert _lib().sai2b_env_sampler_config_layout(C.byref(cfg), n, 1, None, None, None) == _abi.OK


# ---------------------------------------------------------------------------------------------- 4: snapshot layout
def _args(d, hardware=0, depth=0, reward=0, sampler=0, env=0):
    d = dict(d, hardware=hardware, hardware_depth=depth, reward=reward, reset_sampler=sampler, env_sampler=env)
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
def test_the_new_snapshot_blocks(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    d = sl.descriptions(n)["everything"]
    total = er.layout(31, n)[1]
    consts = {k: int(v) for k, v in (line.split() for line in sl._run(exe, "consts").splitlines())}
    assert consts["MAX_TABLE"] == 9 + 11 * 4 + 5 + 6 + 2 and consts["ROOM"] == consts["MAX_TABLE"] + 3 and consts["BLOCKS_ALL"] == 36
    for hw, rew, rs in ((dict(), 0, 0), (dict(hardware=1, depth=8), 1, 1)):
        rows, tail = _table(exe, d, reward=rew, sampler=rs, env=1 + total, **hw)
        base, base_tail = _table(exe, d, reward=rew, sampler=rs, **hw)
        assert len(rows) == len(base) + 2 <= consts["ROOM"]
        eight = [r for r in rows if r["elem"] == 8]
        # the sample rows: the last 8-byte block, behind every environment block; the counter: the last 4-byte block, behind
        # the episode sampler's
        assert (eight[-1]["block"], eight[-1]["rows"], eight[-1]["task"]) == ("env_sampler_sample", total, -1)
        assert (rows[-1]["block"], rows[-1]["rows"], rows[-1]["elem"], rows[-1]["task"]) == ("env_sampler_counter", 1, 4, -1)
        if rs:
            assert rows[-2]["block"] == "reset_sampler_episode" and eight[-2]["block"] == "hw_sensor"
        assert [(r["block"], r["task"], r["rows"], r["word"]) for r in eight[:-1]] == [(r["block"], r["task"], r["rows"], r["word"]) for r in base if r["elem"] == 8]
        four = [(r["block"], r["task"], r["rows"], r["word"] - 2 * total) for r in rows if r["elem"] == 4][:-1]
        assert four == [(r["block"], r["task"], r["rows"], r["word"]) for r in base if r["elem"] == 4]
        assert tail["words"] == base_tail["words"] + 2 * total + 1 and tail["fingerprint"] != base_tail["fingerprint"]
        other, other_tail = _table(exe, d, reward=rew, sampler=rs, env=1 + total - 9, **hw)
        assert other_tail["fingerprint"] != tail["fingerprint"] and other_tail["words"] == tail["words"] - 18

        def diff(a, b):
            return sl._run(exe, "diff", *_args(d, reward=rew, sampler=rs, env=a, **hw), "--", *_args(d, reward=rew, sampler=rs, env=b, **hw)).strip()

        assert diff(1 + total, 1 + total) == "same" and diff(0, 1 + total) == "differ block env_sampler_counter" == diff(1 + total, 0)
        assert diff(1 + total, 1 + total - 9) == "differ block env_sampler_sample"
    # each group holds its own block: the counter is episode state, the sample rows environment
    env, _ = _table(exe, sl.descriptions(n)["environment_only"], env=1 + total)
    assert [r["block"] for r in env if r["block"].startswith("env_sampler")] == ["env_sampler_sample"]
    epi, _ = _table(exe, sl.descriptions(n)["c3"], env=1 + total)
    assert [r["block"] for r in epi if r["block"].startswith("env_sampler")] == ["env_sampler_counter"]
    none, _ = _table(exe, d, env=0)
    assert not [r for r in none if r["block"].startswith("env_sampler")]


@pytest.mark.parametrize("n", [4, 6, 7, 8])
def test_without_the_sampler_the_layout_is_what_it_was(tmp_path_factory, n):
    exe = _build(tmp_path_factory, n)
    golden = json.load(open(GOLDEN))[str(n)]
    descs = sl.descriptions(n)
    assert len(golden) == 8 * len(descs)
    for name, d in descs.items():
        for hs, hw in rl.HARDWARE.items():
            for rs, rew in (("", 0), ("+rew", 1)):
                for ss, smp in (("", 0), ("+rs", 1)):
                    lines = sl._run(exe, "table", *_args(d, hardware=hw[0], depth=hw[1], reward=rew, sampler=smp)).splitlines()
                    table = "\n".join(line for line in lines if line.startswith("row "))  # block, task, rows, bytes, word, first row
                    f = lines[-1].split()
                    got = [len(lines) - 1, int(f[1]), int(f[3]), f[5], hashlib.sha256(table.encode()).hexdigest()[:32]]
                    assert got == golden[name + hs + rs + ss], name + hs + rs + ss


def test_sanitized_tables(tmp_path_factory):
    exe, plain = _build(tmp_path_factory, 8, sanitize=True), _build(tmp_path_factory, 8)
    d = sl.descriptions(8)
    for name in ("everything", "c4", "environment_only"):
        for e in (0, 1 + er.layout(31, 8)[1]):
            a = _args(d[name], hardware=1, depth=8, reward=1, sampler=1, env=e)
            assert sl._run(exe, "table", *a) == sl._run(plain, "table", *a)
    assert sl._run(exe, "layout", 31) == sl._run(plain, "layout", 31)


# ---------------------------------------------------------------------------------------------- 5: distribution
def test_distribution_of_the_draws(tmp_path_factory, tmp_path):
    """200 000 draws of the shared header through the driver, each within 5 standard errors of what the law says"""
    exe = _build(tmp_path_factory, 7)
    R, seed = 200000, 24680
    c = np.zeros((R, 4), dtype=np.uint32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = np.arange(R) % 5, np.arange(R), seed & 0xFFFFFFFF, seed >> 32
    v = np.zeros((R, IN))
    for k, name in enumerate(er.RANGES):
        v[:, 3 * k : 3 * k + 3] = er.default_config()[name]
    a, b, la, lb = 0.5, 2.0, 0.1, 10.0
    v[:, 0:3] = [a, b, 0]  # payload mass scale: uniform
    v[:, 6:9] = [la, lb, 1]  # contact stiffness scale: log-uniform
    v[:, 39:42], v[:, 42:45] = [1.0, 1.0, 0], [1.0, 1.0, 0]  # unit pushes: the rows are the directions
    v[:, 55], v[:, 56] = 1, 4
    v[:, 59:98] = 1.0
    out, _ = _draw(exe, tmp_path, c, v)
    s = out[:, 0]
    assert s.min() >= a and s.max() <= b
    w = b - a
    assert abs(s.mean() - 0.5 * (a + b)) <= 5 * w / np.sqrt(12 * R)
    # the variance of a uniform: w^2 / 12, its standard error w^2 sqrt(1 / 180 R) (fourth central moment w^4 / 80)
    assert abs(s.var() - w * w / 12) <= 5 * w * w * np.sqrt(1 / (180 * R))
    g = out[:, 28]
    assert g.min() >= la * (1 - 1e-14) and g.max() <= lb * (1 + 1e-14)
    # log-uniform on [la, lb], L = ln(lb / la): E s^k = (lb^k - la^k) / (k L)
    L = np.log(lb / la)
    m1, m2, m3, m4 = ((lb**k - la**k) / (k * L) for k in (1, 2, 3, 4))
    var = m2 - m1 * m1
    mu4 = m4 - 4 * m1 * m3 + 6 * m1 * m1 * m2 - 3 * m1**4
    assert abs(g.mean() - m1) <= 5 * np.sqrt(var / R)
    assert abs(g.var() - var) <= 5 * np.sqrt((mu4 - var * var) / R)
    # ln s is uniform on [ln la, ln lb]
    assert abs(np.log(g).mean() - 0.5 * np.log(la * lb)) <= 5 * L / np.sqrt(12 * R)
    d = out[:, 48]
    counts = np.array([(d == k).sum() for k in (1, 2, 3, 4)])
    assert counts.sum() == R and (counts > 0).all()
    assert (np.abs(counts / R - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / R)).all()
    for name, cols in (("force", slice(68, 71)), ("moment", slice(71, 74))):
        axis = out[:, cols].T
        assert np.abs(np.linalg.norm(axis, axis=0) - 1).max() < 1e-15 * 4, name
        # isotropy: mean 0 with variance 1/3 per component; E[a_i a_j] = delta_ij / 3 with variances 4/45 (i = j) and 1/15 (i != j)
        assert (np.abs(axis.mean(axis=1)) <= 5 * np.sqrt(1 / (3 * R))).all(), name
        cov = axis @ axis.T / R
        for i in range(3):
            for j in range(3):
                sd = np.sqrt((4 / 45 if i == j else 1 / 15) / R)
                assert abs(cov[i, j] - (1 / 3 if i == j else 0.0)) <= 5 * sd, (name, i, j)
    assert np.array_equal(out[:, 68:71], out[:, 76:79])  # a magnitude of exactly 1: the rows are the direction


# ---------------------------------------------------------------------------------------------- the clearance case of the GPU test
def test_the_clearance_case_keeps_its_candidates_away_from_the_threshold():
    """tests/test_gpu_env_sampler.py resets robots with the clearance criterion over planes the environment sampler has drawn.
    Here, on the CPU oracle's pose: no candidate of any try lies within 1e-9 m of the threshold on the drawn planes (so rounding
    in the device's kinematics or in the tilted normal cannot change who is accepted), and the drawn planes change who is"""
    import contact_cases as cc
    import reset_sampler_reference as rr

    case, env, new, mask = er.clearance_case()
    B, n = new.shape[1], 7
    m = cc.model("panda")
    kin = rr.oracle_kinematics(m, {}, B, (case["link"], case["points"]))
    cfg = dict(seed=er.CLEARANCE_SEED, first_robot=0, goal_tasks=0, absolute_position=0, ratio_task=-1, min_ratio=0.0, box_task=-1,
               box_lower=(0, 0, 0), box_upper=(0, 0, 0), **er.CLEARANCE_RESET)
    rows = rr.default_rows(n, np.array(m.q_lower[:n]), np.array(m.q_upper[:n]), 4 * n, B)
    tries = []
    for plane in (new, case["rows"]):
        ref = rr.ResetSamplerReference(n, B, [("mft",), ("jt", n, None)], cfg, rows, kin, plane)
        tries.append(ref.reset(mask)["tries"])
        assert ref.borderline() == 0 and len(ref.margins) > 1
    assert not np.array_equal(tries[0], tries[1])
    t = tries[0][mask]
    assert (t == 1).any() and (t > 1).any()
    # the drawn planes: height within its range along the nominal normal, tilt below its maximum
    h = np.einsum("ib,ib->b", new[0:3] - case["rows"][0:3], case["rows"][3:6])
    cosine = np.einsum("ib,ib->b", new[3:6], case["rows"][3:6])
    assert (h >= -0.02 - 1e-12).all() and (h <= 0.05 + 1e-12).all() and (cosine >= np.cos(0.4) - 1e-12).all() and np.ptp(h) > 0.03
