"""CPU-only: the FastBlock of the parameter block cannot go stale. fast_block_fill() (csrc/sai2b_fast_block.h) is its one writer
and upload_params() (csrc/sai2b_host.cpp) its one caller; tests/cpp/fast_block_driver.cpp includes the header alone, edits a
parameter block the way the setters edit theirs and, after each edit and fill, holds every value of the block to the field it
copies. Built with plain g++ under the address and undefined-behaviour sanitizers, for the 7- and the 6-joint build, and run as
a program of its own. (What the setters of the C API do to a live context is tests/test_gpu_fast_block.py's.)"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "fast_block_driver.cpp")
SAN = "-fsanitize=address,undefined"


def _build(tmp, n):
    exe = os.path.join(tmp, f"fast_block_n{n}")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-DSAI2B_N={n}", "-I", CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd[:4] + [SAN, "-fno-sanitize-recover=all"] + cmd[4:], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        print(f"N = {n}: the sanitizer runtime of g++ is missing here, built WITHOUT -fsanitize:\n{r.stderr[-500:]}")
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("n", [7, 6])
def test_fast_block_follows_every_change(tmp_path, n):
    exe = _build(str(tmp_path), n)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    last = r.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, r.stdout[-1000:]


def test_one_writer_one_caller():
    """The block is written in fast_block_fill() alone, and that is called from upload_params() alone."""
    writes, calls = [], []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".cpp", ".h", ".hpp", ".hip", ".inc")) or name == "sai2b_dispatch.cpp":
            continue
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())  # (comments may speak of it)
        calls += [(name, m.start()) for m in re.finditer(r"\bfast_block_fill\s*\(", text) if name != "sai2b_fast_block.h"]
        # an assignment through `.fast` from host code (the kernels take the block through a const reference)
        writes += [(name, m.group(0)) for m in re.finditer(r"(h_params|meas|hp)\.fast\b[^;\n]*=", text)]
    assert not writes, writes
    assert {c[0] for c in calls} == {"sai2b_host.cpp"}, calls
    host = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "sai2b_host.cpp")).read())
    body = host[host.index("static int upload_params("):host.index("static int create_impl(")]
    assert len(calls) == body.count("fast_block_fill(") == 2, calls  # the parameters and their measured-state copy
