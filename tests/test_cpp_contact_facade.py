"""The contact members of the C++ facade (include/Sai2PrimitivesBatched.h: BatchedSimulation::setContactPlanes, clearContact,
attachForceSensor, getContactState, robotsInContact) compiled with g++ against the C ABI, the way tests/test_cpp_facade.py
builds facade_test.cpp, and their device-free argument checks run (tests/cpp/contact_facade_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def contact_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "contact_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "contact_facade_test.cpp"),
         "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_contact_members_compile_and_reject_bad_arguments(contact_bin):
    r = subprocess.run([contact_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 15
