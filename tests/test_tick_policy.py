"""CPU-only: what a tick launches (csrc/sai2b_tick_policy.h: eligibility of a hierarchy, the singular mode, the back-off, the
one-launch form, when and how the work list's counts are asked for) with hand-built hierarchies and scripted counts, at
batch sizes no GPU test reaches. tests/cpp/tick_policy_driver.cpp includes the header alone; it is built with plain g++
under the address and undefined-behaviour sanitizers for the 7- and the 6-joint build and run as a program of its own."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "tick_policy_driver.cpp")
SAN = "-fsanitize=address,undefined"


def _build(tmp, n):
    exe = os.path.join(tmp, f"tick_policy_n{n}")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-DSAI2B_N={n}", "-I", CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd[:4] + [SAN, "-fno-sanitize-recover=all"] + cmd[4:], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        print(f"N = {n}: the sanitizer runtime of g++ is missing here, built WITHOUT -fsanitize:\n{r.stderr[-500:]}")
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("n", [7, 6])
def test_tick_policy(tmp_path, n):
    exe = _build(str(tmp_path), n)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    last = r.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok" and int(last[1]) > 300, r.stdout[-1000:]
