"""The hardware members of the C++ facade (include/Sai2PrimitivesBatched.h: BatchedSimulation::setHardware, clearHardware,
getHardwareState), compiled with g++ against the C ABI the way tests/test_cpp_snapshot_facade.py builds its program
(tests/cpp/hardware_facade_test.cpp): without a device the members by signature and the sensor-task conditions; on the GPU
setHardware with a delay, a gain and a sensor task through 6 periods of integrate() against the known delayed command, the
sensor's bias against a twin, clearHardware, and std::invalid_argument from setHardware itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def hardware_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "hardware_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "hardware_facade_test.cpp"), "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}",
         "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_hardware_members_compile_and_reject_bad_sensor_tasks(hardware_bin):
    r = subprocess.run([hardware_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 8


@pytest.mark.gpu
def test_cpp_hardware_six_periods_sensor_clear_and_exceptions(hardware_bin):
    r = subprocess.run([hardware_bin, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 22
