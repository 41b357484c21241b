"""The collision members of the C++ facade (include/Sai2PrimitivesBatched.h: setCollisionGeometry by moving-link index or by URDF
link name, setCollisionEnvironment, clearCollision, queryCollision, collisionCounts, endEpisodes on BatchedSimulation; setCollision,
queryCollision, collisionCounts, endEpisodes, clearCollision on ShardedRobotController), compiled with g++ against the C ABI the way
tests/test_cpp_joint_sensor_facade.py builds its program (tests/cpp/collision_facade_test.cpp): without a device the members by
signature, link-name resolution and the exceptions that need no device; on the GPU a sphere over a floor, the flags and counts, a
geometry that keeps its environment, the members' own exceptions, endEpisodes and clearCollision."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
URDF = os.path.join(ROOT, "tests", "golden", "urdf", "panda_arm.urdf")


@pytest.fixture(scope="module")
def collision_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "collision_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "collision_facade_test.cpp"), "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}",
         "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_collision_members_compile_resolve_link_names_and_reject_bad_arguments(collision_bin):
    r = subprocess.run([collision_bin, "validate", URDF], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 21


@pytest.mark.gpu
def test_cpp_collision_query_environment_end_episodes_and_exceptions(collision_bin):
    r = subprocess.run([collision_bin, "run", URDF], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 21
