"""The masked re-initialisation and the episode reset through the C++ facade (include/Sai2PrimitivesBatched.h:
RobotController::reinitializeTasks(mask) / resetRobots, the tasks' reInitializeTask(mask), the same on
ShardedRobotController), compiled with g++ against the C ABI the way tests/test_cpp_contact_facade.py builds its program
(tests/cpp/subset_reset_test.cpp): the device-free argument checks, and on the GPU 257 robots over two uneven shards with a
mask straddling the shard boundary, bit-equal to one context given the same mask."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def reset_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "subset_reset_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "subset_reset_test.cpp"),
         "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_masked_members_compile_and_reject_wrong_sizes(reset_bin):
    r = subprocess.run([reset_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 9


@pytest.mark.gpu
def test_cpp_sharded_masked_calls_equal_one_context(reset_bin):
    r = subprocess.run([reset_bin, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 15
