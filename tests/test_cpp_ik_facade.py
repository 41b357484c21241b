"""The inverse-kinematics members of the C++ facade (include/Sai2PrimitivesBatched.h: setInverseKinematics, clearInverseKinematics,
getInverseKinematics, solveInverseKinematics, getInverseKinematicsCounts on RobotController and BatchedSimulation, mirrored on
ShardedRobotController), compiled with g++ against the C ABI the way tests/test_cpp_collision_facade.py builds its program
(tests/cpp/ik_facade_test.cpp): without a device the members by signature and the exceptions that need no device, each with the
validator's message; on the GPU one solve of 130 Pandas through the members, held to tests/ik_reference.py here, and the members'
own exceptions."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
URDF = os.path.join(ROOT, "tests", "golden", "urdf", "panda_arm.urdf")
B = 130


@pytest.fixture(scope="module")
def ik_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "ik_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ik_facade_test.cpp"),
         "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_ik_members_compile_and_reject_bad_arguments(ik_bin):
    r = subprocess.run([ik_bin, "validate", URDF], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 14


def _case():
    """130 near-seed records for the Panda with its control frame 0.15 m up the end-effector body's z, and the reference's answer"""
    import ik_cases as ic
    from ik_reference import IkReference

    with open(URDF) as f:
        text = f.read()
    lo, hi = ic.limits("panda")
    ref = IkReference(text, "end-effector", (0.0, 0.0, 0.15), None, lo, hi)
    rng = np.random.default_rng(130)
    qt = lo[:, None] + (hi - lo)[:, None] * (0.5 + 0.9 * (rng.random((7, B)) - 0.5))
    seed = np.clip(qt + 0.3 * (2 * rng.random((7, B)) - 1), lo[:, None], hi[:, None])
    goal = ref.goal_rows(qt)
    return ic, ref, goal, np.ascontiguousarray(seed), ref.solve(goal, seed, track_sigma=True)


def test_the_reference_alone_on_the_facade_records():
    ic, ref, goal, seed, out = _case()
    assert (out["flags"] & 1).mean() > 0.95 and ic.separated(out).all()


@pytest.mark.gpu
def test_cpp_ik_solve_against_the_reference_and_exceptions(ik_bin, tmp_path):
    ic, ref, goal, seed, out = _case()
    g, s, o = (str(tmp_path / n) for n in ("goal.bin", "seed.bin", "out.bin"))
    goal.tofile(g), seed.tofile(s)
    r = subprocess.run([ik_bin, "run", URDF, g, s, o], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 15
    got = np.fromfile(o).reshape(7 + 5 + 1, B)
    q, status, flags = got[:7], got[7:12], got[12].astype(np.uint8)
    sep = ic.separated(out)
    assert np.array_equal(flags[sep], out["flags"][sep])
    cv = (flags & 1) != 0
    ep, er = ref.pose_error(goal, np.where(cv, q, seed))
    assert (ep[cv] <= 1e-6).all() and (er[cv] <= 1e-6).all()
    cond = sep & (out["sigma_min"] >= ic.SIGMA_MIN)
    assert cond.sum() > B // 4 and np.abs(q[:, cond] - out["q"][:, cond]).max() <= ic.Q_BOUND
    assert np.array_equal(status[2:4, cond], out["status"][2:4, cond])
