"""Snapshot banks through the C++ facade (include/Sai2PrimitivesBatched.h: SnapshotBank, createSnapshotBank on RobotController
and BatchedSimulation), compiled with g++ against the C ABI the way tests/test_cpp_subset_reset.py builds its program
(tests/cpp/snapshot_facade_test.cpp): without a device the members by signature and the C entry points' treatment of NULL; on
the GPU the round trip, the clone and a checkpoint on 130 robots, bit-equal to a twin controller, and std::invalid_argument
for a blob of another hierarchy."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def snapshot_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "snapshot_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "snapshot_facade_test.cpp"),
         "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_snapshot_members_compile_and_reject_null(snapshot_bin):
    r = subprocess.run([snapshot_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 10


@pytest.mark.gpu
def test_cpp_snapshot_round_trip_clone_and_foreign_blob(snapshot_bin):
    r = subprocess.run([snapshot_bin, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 14
