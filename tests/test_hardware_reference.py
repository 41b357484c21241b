"""The device random generator (csrc/sai2b_rng.h) and its numpy restatement (tests/hardware_reference.py) on the CPU.
tests/cpp/hardware_driver.cpp includes the header alone and is built with plain g++, and once more with
-fsanitize=address,undefined, each run as the stand-alone program it is.

1: the three known answers of Philox4x32-10 (the zero and the all-ones vector of Random123's kat_vectors and its pi vector),
   exact, from the driver and from the restatement.
2: 10 000 random (counter, key) pairs: the driver's words are bit-equal to the restatement's, and its normals are within
   4e-15 of them (4 ulp of 6.77, the largest normal: two libm implementations of log / sin / cos).
3: the draw as the kernels make it (counter (n, e, 256 stream + call, robot), key from the seed) equals the restatement's
   normals().
4: statistics of the restatement alone, seed 20261020, first_robot 0, episode 0, 4 099 robots x 7 joints x 8 periods =
   N = 229 544 actuator normals: |mean| < 5 / sqrt(N) = 0.0104, |std - 1| < 5 / sqrt(2 N) = 0.0074, and the correlations between
   consecutive periods, neighbouring robots and neighbouring joints each below 0.0104 in magnitude. Because the GPU is held to
   this restatement value by value, the statistics need no GPU test.
5: the stage laws of HardwareReference on hand-made inputs: the ideal rows pass the command through, a pure delay replays the
   command of d periods ago, the lag and the sensor filter follow their recurrences, a reset restarts them."""
import os
import subprocess

import numpy as np
import pytest

import hardware_reference as hr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "hardware_driver.cpp")
SAN = "-fsanitize=address,undefined"

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

_built = {}


def _build(tmp_factory, sanitize):
    if sanitize not in _built:
        exe = os.path.join(str(tmp_factory.mktemp("hwrng" + ("s" if sanitize else ""))), "hardware_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[4:4] = [SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[sanitize] = exe
    return _built[sanitize]


def _words(exe, counters, keys):
    """counters [K][4], keys [K][2] -> (words [K][4] uint64, normals [K][4])"""
    text = "".join("%x %x %x %x %x %x\n" % (*c, *k) for c, k in zip(counters.tolist(), keys.tolist()))
    r = subprocess.run([exe, "words"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(counters)
    return np.array([[int(x, 16) for x in f[:4]] for f in rows], dtype=np.uint64), np.array([[float(x) for x in f[4:]] for f in rows])


@pytest.mark.parametrize("sanitize", [False, True])
def test_known_answers(tmp_path_factory, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    c, k = np.array([a[0] for a in KNOWN], dtype=np.uint64), np.array([a[1] for a in KNOWN], dtype=np.uint64)
    want = np.array([a[2] for a in KNOWN], dtype=np.uint64)
    got, _ = _words(exe, c, k)
    assert np.array_equal(got, want), [[hex(int(x)) for x in row] for row in got]
    assert np.array_equal(hr.philox4x32_10(c.T, k.T).T, want)


@pytest.mark.parametrize("sanitize", [False, True])
def test_driver_equals_the_restatement(tmp_path_factory, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    rng = np.random.default_rng(20261020)
    K = 10000
    c, k = rng.integers(0, 2**32, (K, 4), dtype=np.uint64), rng.integers(0, 2**32, (K, 2), dtype=np.uint64)
    got, z = _words(exe, c, k)
    want = hr.philox4x32_10(c.T, k.T)
    assert np.array_equal(got, want.T)
    zr = np.stack([*hr.box_muller(want[0], want[1]), *hr.box_muller(want[2], want[3])]).T
    err = np.abs(z - zr).max()
    print(f"normals, driver against numpy: {err:.2e}, largest |z| {np.abs(zr).max():.3f}")
    assert err < 4e-15 and np.isfinite(zr).all()


@pytest.mark.parametrize("sanitize", [False, True])
def test_largest_normal(tmp_path_factory, sanitize):
    """the corners of the uniform, which random counters reach only by chance: u = 2^-33 (word 0) gives the largest radius,
    sqrt(-2 ln 2^-33) = 6.764 < 6.77; word 2^32 - 1 gives a finite one too; in the restatement and in the header's box_muller"""
    x0 = np.array([0, 0, 2**32 - 1, 2**32 - 1, 0], dtype=np.uint64)
    x1 = np.array([0, 2**32 - 1, 0, 2**32 - 1, 2**31], dtype=np.uint64)
    z0, z1 = hr.box_muller(x0, x1)
    assert np.isfinite(z0).all() and np.isfinite(z1).all() and 6.76 < np.hypot(z0, z1).max() < 6.77
    text = "".join("%x %x\n" % (a, b) for a, b in zip(x0.tolist(), x1.tolist()))
    r = subprocess.run([_build(tmp_path_factory, sanitize), "box"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([[float(v) for v in line.split()] for line in r.stdout.splitlines()])
    assert got.shape == (5, 2) and np.isfinite(got).all() and np.abs(got - np.stack([z0, z1]).T).max() < 4e-15


def test_kernel_draw_equals_normals(tmp_path_factory):
    exe = _build(tmp_path_factory, False)
    seed = 0x0123456789ABCDEF
    for n, e, stream, robot in ((0, 0, 0, 0), (7, 2, 1, 4098), (123456, 3, 0, 70000)):
        want = hr.normals(np.array([n]), np.array([e]), stream, np.array([robot]), seed, 8)[:, 0]
        got = []
        for call in (0, 1):
            r = subprocess.run([exe, "normals", str(n), str(e), str(stream), str(call), str(robot), str(seed)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            got += [float(x) for x in r.stdout.split()]
        assert np.abs(np.array(got) - want).max() < 4e-15


def test_statistics_of_the_restatement():
    B, dof, periods = 4099, 7, 8
    robot = np.arange(B)
    z = np.stack([hr.normals(np.full(B, n), np.zeros(B, dtype=np.int64), hr.ACTUATOR, robot, 20261020, dof) for n in range(periods)])  # [n][i][b]
    N = z.size
    assert N == 229544

    def corr(a, b):
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])

    mean, std = float(z.mean()), float(z.std())
    c = (corr(z[:-1], z[1:]), corr(z[:, :, :-1], z[:, :, 1:]), corr(z[:, :-1], z[:, 1:]))
    print(f"mean {mean:.4f} std - 1 {std - 1:.4f} correlations: periods {c[0]:.4f} robots {c[1]:.4f} joints {c[2]:.4f}")
    assert abs(mean) < 5 / np.sqrt(N) and abs(std - 1) < 5 / np.sqrt(2 * N)
    assert all(abs(x) < 5 / np.sqrt(N) for x in c)


def test_stage_laws():
    dof, B, D = 4, 6, 3
    rng = np.random.default_rng(5)
    cmds = rng.uniform(-10, 10, (9, dof, B))
    # ideal: the command passes through, bit for bit
    hw = hr.HardwareReference(dof, B, D)
    for c in cmds:
        assert np.array_equal(hw.actuate(c), c)
        assert np.array_equal(hw.sense(c[0] * np.ones((6, B))), c[0] * np.ones((6, B)))
        hw.advance()
    # a pure delay: the command of d periods ago, the first command until d have passed
    act, sen = hr.ideal_rows(dof, B)
    act[0] = np.arange(B) % (D + 1)
    hw = hr.HardwareReference(dof, B, D, act)
    for n, c in enumerate(cmds):
        a = hw.actuate(c)
        hw.advance()
        for b in range(B):
            assert np.array_equal(a[:, b], cmds[max(n - int(act[0, b]), 0)][:, b])
    # lag, gain and the sensor's bias and filter: their recurrences; a reset restarts them
    act[0], act[1 : 1 + dof], act[1 + dof : 1 + 2 * dof] = 0, 0.25, 1.5
    sen[0:6], sen[12] = 2.0, 0.5
    hw = hr.HardwareReference(dof, B, D, act, sen)
    f = g = None
    for n, c in enumerate(cmds[:4]):
        f = c if n == 0 else f + 0.25 * (c - f)
        y = np.ones((6, B)) * n + 2.0
        g = y if n == 0 else g + 0.5 * (y - g)
        assert np.allclose(hw.actuate(c), 1.5 * f, rtol=0, atol=1e-14) and np.allclose(hw.sense(np.ones((6, B)) * n), g, rtol=0, atol=1e-14)
        hw.advance()
    mask = np.arange(B) % 2 == 0
    hw.reset(mask)
    assert np.array_equal(hw.n, np.where(mask, 0, 4)) and np.array_equal(hw.e, mask.astype(int))
    a = hw.actuate(cmds[4])
    assert np.array_equal(a[:, mask], 1.5 * cmds[4][:, mask])
    assert np.allclose(a[:, ~mask], 1.5 * (f + 0.25 * (cmds[4] - f))[:, ~mask], rtol=0, atol=1e-14)
    # noise: the robot index is in the counter, first_robot shifts it
    act[1 + 2 * dof :] = 0.1
    whole = hr.HardwareReference(dof, B, D, act, sen, seed=9).actuate(cmds[0])
    part = hr.HardwareReference(dof, 2, D, act[:, 4:], sen[:, 4:], seed=9, first_robot=4).actuate(cmds[0][:, 4:])
    noise = whole - 1.5 * cmds[0]
    assert np.array_equal(whole[:, 4:], part) and np.abs(noise[:, 0] - noise[:, 1]).min() > 1e-6
