"""The joint-sensor members of the C++ facade (include/Sai2PrimitivesBatched.h: setJointSensor, clearJointSensor,
jointSensorState, measuredState on RobotController, BatchedSimulation and ShardedRobotController), compiled with g++ against the
C ABI the way tests/test_cpp_hardware_facade.py builds its program (tests/cpp/joint_sensor_facade_test.cpp): without a device
the members by signature and what the configuration check rejects; on the GPU a pure delay through 6 periods of integrate()
against the recorded truth, the clocks, a reset, an offset alone through the controller's members, clearJointSensor, and
std::invalid_argument from setJointSensor itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def joint_sensor_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "joint_sensor_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "joint_sensor_facade_test.cpp"), "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}",
         "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_joint_sensor_members_compile_and_reject_bad_configurations(joint_sensor_bin):
    r = subprocess.run([joint_sensor_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 8


@pytest.mark.gpu
def test_cpp_joint_sensor_delay_reset_offset_clear_and_exceptions(joint_sensor_bin):
    r = subprocess.run([joint_sensor_bin, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 20
