"""The joint sensors' law (csrc/sai2b_joint_sensor_law.h, the code joint_sense_kernel runs per lane) against its numpy restatement
(tests/joint_sensor_reference.py) on the CPU. tests/cpp/joint_sensor_driver.cpp includes the header alone and is built with
plain g++, and once more with -fsanitize=address,undefined, each run as the stand-alone program it is.

1: 10 000 random records, seed 20261020: 4 / 6 / 7 / 8 joints, both velocity modes, m = 0 (a third) and m up to 10^6, D and d
   up to 8 (d row also negative, beyond D and NaN: read as the kernel reads it), every parameter zero for some joints and not
   for others, alpha = 1 for some. Tolerances are the project's for hardware effects: positions 1e-12, velocities 1e-10 (the
   normals of two libm agree to 4e-15; a finite difference divides a position error of 1e-15 by dt >= 1e-4). Where the quantum
   is positive the position is a multiple of it and must be the reference's EXACTLY; records with some x / quantum within 1e-9
   of a half-integer are left out, decided by the reference alone, at most 1e-4 of all (measured with this seed: 0 of 10 000).
   The history slots the reading does not write are untouched, q_pose is the measured q on entry when asked and untouched
   otherwise.
2: ideal rows: bit-equal to the truth whatever m, D, mode = tachometer; a pure delay: bit-equal to the slot of d readings ago.
3: JointSensorReference on hand-made sequences: the delay replays the reading of d periods ago and the first until d have
   passed, the filter and the finite difference follow their recurrences, quantisation rounds half to even, a reset re-seeds
   the selected robots in their next episode, first_robot shifts the noise."""
import os
import subprocess

import numpy as np
import pytest

import joint_sensor_reference as jr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "joint_sensor_driver.cpp")
SAN = "-fsanitize=address,undefined"
INTS, IN, OUT = 8, 235, 184
POS_TOL, VEL_TOL = 1e-12, 1e-10

_built = {}


def _build(tmp_factory, sanitize):
    if sanitize not in _built:
        exe = os.path.join(str(tmp_factory.mktemp("js" + ("s" if sanitize else ""))), "joint_sensor_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[4:4] = [SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[sanitize] = exe
    return _built[sanitize]


def _run(exe, tmp_path, ints, vals):
    a, b, c = (str(tmp_path / n) for n in ("ints.bin", "vals.bin", "out.bin"))
    np.ascontiguousarray(ints, dtype=np.uint32).tofile(a)
    np.ascontiguousarray(vals, dtype=np.float64).tofile(b)
    r = subprocess.run([exe, "readings", a, b, c], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(c, dtype=np.float64).reshape(len(ints), OUT)


def _pack(dof, rec):
    """dict of [..][K] arrays -> (ints [K][8], values [K][IN])"""
    K = rec["q"].shape[1]
    ints = np.zeros((K, INTS), dtype=np.uint32)
    ints[:, 0] = dof
    for k, name in enumerate(("m", "e", "mode", "D", "robot", "k0", "k1")):
        ints[:, 1 + k] = rec[name]
    v = np.zeros((K, IN))
    v[:, 0 : 1 + 5 * dof] = rec["rows"].T
    v[:, 41 : 41 + dof], v[:, 49 : 49 + dof], v[:, 57] = rec["q"].T, rec["dq"].T, rec["dt"]
    v[:, 58 : 58 + dof], v[:, 66 : 66 + dof] = rec["prev"].T, rec["filt"].T
    v[:, 74 : 74 + 9 * 2 * dof] = rec["hist"].transpose(2, 0, 1).reshape(K, -1)
    v[:, 218 : 218 + dof], v[:, 226 : 226 + dof], v[:, 234] = rec["qm"].T, rec["dqm"].T, rec["save_pose"]
    return ints, v


def _unpack(dof, out):
    K = len(out)
    return dict(p=out[:, 0:dof].T, v=out[:, 8 : 8 + dof].T, hist=out[:, 16 : 16 + 9 * 2 * dof].reshape(K, 9, 2 * dof).transpose(1, 2, 0),
                q_meas=out[:, 160 : 160 + dof].T, dq_meas=out[:, 168 : 168 + dof].T, pose=out[:, 176 : 176 + dof].T)


def _records(dof, K, rng, ideal=False, pure_delay=False):
    def some(shape, lo, hi, zero=0.4):
        return np.where(rng.random(shape) < zero, 0.0, rng.uniform(lo, hi, shape))

    rows = jr.ideal_rows(dof, K)
    D = rng.integers(0, 9, K)
    if not ideal:
        rows[0] = np.minimum(rng.integers(0, 9, K), D)
        if not pure_delay:
            odd = rng.random(K)
            rows[0] = np.where(odd < 0.03, np.nan, np.where(odd < 0.06, -2.0, np.where(odd < 0.09, 11.0, rows[0])))
            rows[1 : 1 + dof] = some((dof, K), -0.05, 0.05)
            rows[1 + dof : 1 + 2 * dof] = some((dof, K), 1e-5, 1e-2)
            rows[1 + 2 * dof : 1 + 3 * dof] = some((dof, K), 1e-5, 1e-2)
            rows[1 + 3 * dof : 1 + 4 * dof] = some((dof, K), 1e-4, 1e-1)
            rows[1 + 4 * dof :] = np.where(rng.random((dof, K)) < 0.4, 1.0, rng.uniform(0.05, 1.0, (dof, K)))
    m = np.where(rng.random(K) < 1 / 3, 0, np.where(rng.random(K) < 0.5, rng.integers(1, 12, K), rng.integers(1, 10**6, K)))
    return dict(rows=rows, D=D, m=m, e=rng.integers(0, 1000, K), mode=np.zeros(K, dtype=np.int64) if (ideal or pure_delay) else rng.integers(0, 2, K),
                robot=rng.integers(0, 2**32, K, dtype=np.uint64), k0=rng.integers(0, 2**32, K, dtype=np.uint64), k1=rng.integers(0, 2**32, K, dtype=np.uint64),
                q=rng.uniform(-3, 3, (dof, K)), dq=rng.uniform(-2, 2, (dof, K)), dt=10.0 ** rng.uniform(-4, -2, K),
                prev=rng.uniform(-3, 3, (dof, K)), filt=rng.uniform(-2, 2, (dof, K)), hist=rng.uniform(-3, 3, (9, 2 * dof, K)),
                qm=rng.uniform(-3, 3, (dof, K)), dqm=rng.uniform(-2, 2, (dof, K)), save_pose=(rng.random(K) < 0.5).astype(np.float64))


def _reference(rec):
    hist = rec["hist"].copy()
    ref = jr.reading(rec["rows"], rec["q"], rec["dq"], rec["dt"], rec["m"], rec["e"], rec["mode"], rec["D"], rec["robot"], rec["k0"], rec["k1"],
                     rec["prev"], rec["filt"], hist)
    ref["hist"] = hist
    return ref


@pytest.mark.parametrize("sanitize", [False, True])
def test_driver_equals_the_restatement(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    rng = np.random.default_rng(20261020)
    total = left_out = 0
    worst = dict(p=0.0, v=0.0)
    for dof in (4, 6, 7, 8):
        K = 2500
        rec = _records(dof, K, rng)
        got, ref = _unpack(dof, _run(exe, tmp_path, *_pack(dof, rec))), _reference(rec)
        skip = ref["near_half"].any(axis=0)
        total, left_out = total + K, left_out + int(skip.sum())
        keep = ~skip
        quantised = rec["rows"][1 + 2 * dof : 1 + 3 * dof] > 0.0
        assert quantised.any() and (~quantised).any() and (rec["m"] == 0).any() and (rec["mode"] == 1).any() and (rec["mode"] == 0).any()
        assert np.array_equal(got["p"][quantised & keep], ref["p"][quantised & keep])
        for key, tol in (("p", POS_TOL), ("q_meas", POS_TOL), ("v", VEL_TOL), ("dq_meas", VEL_TOL)):
            err = np.abs(got[key] - ref[key])[:, keep].max()
            kind = "p" if tol == POS_TOL else "v"
            worst[kind] = max(worst[kind], err)
            assert err < tol, (dof, key, err)
        # the history: the slot of this reading holds (p, v) when D > 0, every other slot is as it was
        for b in np.flatnonzero(keep)[:400]:
            D, m = int(rec["D"][b]), int(rec["m"][b])
            h0, h1 = rec["hist"][:, :, b].copy(), got["hist"][:, :, b]
            if D > 0:
                assert np.abs(h1[m % (D + 1), :dof] - ref["p"][:, b]).max() < POS_TOL and np.abs(h1[m % (D + 1), dof:] - ref["v"][:, b]).max() < VEL_TOL
                h0[m % (D + 1)] = h1[m % (D + 1)]
            assert np.array_equal(h0, h1)
        want_pose = np.where(rec["save_pose"] != 0, rec["qm"], 0.0)
        assert np.array_equal(got["pose"], want_pose)
    print(f"records {total}, left out near a tie {left_out}, worst position error {worst['p']:.2e}, worst velocity error {worst['v']:.2e}")
    assert total == 10000 and left_out <= 1e-4 * total


@pytest.mark.parametrize("sanitize", [False, True])
def test_ideal_rows_and_a_pure_delay_are_bit_equal(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    rng = np.random.default_rng(7)
    for dof in (4, 6, 7, 8):
        rec = _records(dof, 500, rng, ideal=True)
        got = _unpack(dof, _run(exe, tmp_path, *_pack(dof, rec)))
        for key, truth in (("p", "q"), ("q_meas", "q"), ("v", "dq"), ("dq_meas", "dq")):
            assert np.array_equal(got[key], rec[truth]), (dof, key)
        rec = _records(dof, 500, rng, pure_delay=True)
        got = _unpack(dof, _run(exe, tmp_path, *_pack(dof, rec)))
        assert np.array_equal(got["p"], rec["q"]) and np.array_equal(got["v"], rec["dq"])
        for b in range(500):
            D, m, d = int(rec["D"][b]), int(rec["m"][b]), int(rec["rows"][0, b])
            past = max(m - d, 0)
            want = np.concatenate([rec["q"][:, b], rec["dq"][:, b]]) if (D == 0 or past == m) else rec["hist"][past % (D + 1), :, b]
            assert np.array_equal(np.concatenate([got["q_meas"][:, b], got["dq_meas"][:, b]]), want), (dof, b)
        assert (rec["rows"][0] > 0).any()


def test_the_reference_on_hand_made_sequences():
    dof, B, D = 4, 6, 3
    rng = np.random.default_rng(5)
    qs, dqs = rng.uniform(-2, 2, (9, dof, B)), rng.uniform(-1, 1, (9, dof, B))
    dt = 1e-3
    # ideal: the truth, bit for bit
    js = jr.JointSensorReference(dof, B, D)
    assert all(np.array_equal(a, b) for a, b in zip(js.seed(qs[0], dqs[0]), (qs[0], dqs[0])))
    for q, dq in zip(qs[1:], dqs[1:]):
        qm, dqm = js.step(q, dq, dt)
        assert np.array_equal(qm, q) and np.array_equal(dqm, dq)
    assert np.array_equal(js.c, np.full(B, 9)) and not js.e.any()
    # a pure delay: the reading of d periods ago, the first until d have passed
    rows = jr.make_rows(dof, B, delay=np.arange(B) % (D + 1))
    js = jr.JointSensorReference(dof, B, D, rows)
    js.seed(qs[0], dqs[0])
    for n in range(1, 9):
        qm, dqm = js.step(qs[n], dqs[n], dt)
        for b in range(B):
            k = max(n - int(rows[0, b]), 0)
            assert np.array_equal(qm[:, b], qs[k][:, b]) and np.array_equal(dqm[:, b], dqs[k][:, b])
    # offset, quantum, finite difference and the filter: their recurrences
    rows = jr.make_rows(dof, B, offset=0.25, quantum=0.01, velocity_alpha=0.5)
    js = jr.JointSensorReference(dof, B, 0, rows, velocity_mode=jr.FINITE_DIFFERENCE)
    p0 = 0.01 * np.rint((qs[0] + 0.25) / 0.01)
    qm, dqm = js.seed(qs[0], dqs[0])
    assert np.array_equal(qm, p0) and np.array_equal(dqm, dqs[0])  # reading 0 has no earlier position: the tachometer's value
    v, prev = dqs[0], p0
    for n in range(1, 5):
        p = 0.01 * np.rint((qs[n] + 0.25) / 0.01)
        v = v + 0.5 * ((p - prev) / dt - v)
        prev = p
        qm, dqm = js.step(qs[n], dqs[n], dt)
        assert np.array_equal(qm, p) and np.array_equal(dqm, v)
    # round half to even
    one = jr.JointSensorReference(4, 1, 0, jr.make_rows(4, 1, quantum=0.5))
    assert np.array_equal(one.seed(np.array([[0.25], [0.75], [-0.25], [1.25]]), np.zeros((4, 1)))[0][:, 0], [0.0, 1.0, -0.0, 1.0])
    assert one.near_half.all()
    # a reset re-seeds the selected robots in their next episode
    mask = np.arange(B) % 2 == 0
    before = js.q_meas.copy()
    qm, _ = js.seed(qs[5], dqs[5], mask, next_episode=True)
    assert np.array_equal(js.c, np.where(mask, 1, 5)) and np.array_equal(js.e, mask.astype(int))
    assert np.array_equal(qm[:, ~mask], before[:, ~mask]) and np.array_equal(qm[:, mask], (0.01 * np.rint((qs[5] + 0.25) / 0.01))[:, mask])
    # noise: the robot index is in the counter, first_robot shifts it; the episode is too
    rows = jr.make_rows(dof, B, noise=0.01, velocity_noise=0.1)
    whole = jr.JointSensorReference(dof, B, 0, rows, seed=9).seed(qs[0], dqs[0])
    part = jr.JointSensorReference(dof, 2, 0, rows[:, 4:], seed=9, first_robot=4).seed(qs[0][:, 4:], dqs[0][:, 4:])
    assert np.array_equal(whole[0][:, 4:], part[0]) and np.array_equal(whole[1][:, 4:], part[1])
    assert np.abs(whole[0] - qs[0]).min() > 0 and np.abs(whole[0] - qs[0]).max() < 0.0677 + 1e-12
    again = jr.JointSensorReference(dof, B, 0, rows, seed=9)
    again.e[:] = 1
    assert np.abs(again.seed(qs[0], dqs[0])[0] - whole[0]).min() > 0
