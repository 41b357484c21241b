"""The environment-sampler members of the C++ facade (include/Sai2PrimitivesBatched.h: setEnvSampler, clearEnvSampler,
randomizeRobots, envSamplerCounts on RobotController and ShardedRobotController), compiled with g++ against the C ABI the way
tests/test_cpp_reset_sampler_facade.py builds its program (tests/cpp/env_sampler_facade_test.cpp): the device-free argument
checks; on the GPU three draws through the members, bit-equal to the C ABI on a twin, two shards bit-equal to the one context,
and the exceptions on a live controller."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")


@pytest.fixture(scope="module")
def sampler_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "env_sampler_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "env_sampler_facade_test.cpp"), "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}",
         "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_env_sampler_members_compile_and_reject_bad_arguments(sampler_bin):
    r = subprocess.run([sampler_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 9


@pytest.mark.gpu
def test_cpp_env_sampler_members_equal_the_c_abi(sampler_bin):
    r = subprocess.run([sampler_bin, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and "FAIL" not in r.stdout and r.stdout.count("ok ") == 21
