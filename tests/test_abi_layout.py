"""CPU-only guard of the C ABI layout: the ctypes mirror in _abi.py against include/sai2b.h as the host C compiler lays
it out. A probe generated from the mirror's own field lists prints sizeof and offsetof of every field of
sai2b_robot_model, sai2b_task_config and sai2b_urdf_links, and the struct sizes; each must equal what ctypes computes.
A field inserted into the header but not into the mirror (or the other way round) moves every offset behind it."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from sai2_primitives_perso_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sai2b_robot_model": _abi.RobotModel, "sai2b_task_config": _abi.TaskConfig, "sai2b_urdf_links": _abi.UrdfLinks}
CC = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")

pytestmark = pytest.mark.skipif(CC is None, reason="no host C compiler")


def _mirror():
    """-> {(struct, field): (offset, size)} and {(struct, None): (0, sizeof)} from the ctypes side"""
    out = {}
    for cname, cls in STRUCTS.items():
        out[(cname, None)] = (0, C.sizeof(cls))
        for name, _ in cls._fields_:
            f = getattr(cls, name)
            out[(cname, name)] = (f.offset, f.size)
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "sai2b.h"', "int main(void) {"]
    for cname, cls in STRUCTS.items():
        lines.append(f'\tprintf("{cname} - 0 %zu\\n", sizeof({cname}));')
        for name, _ in cls._fields_:
            lines.append(f'\tprintf("{cname} {name} %zu %zu\\n", offsetof({cname}, {name}), sizeof((({cname}*)0)->{name}));')
    lines += ["\treturn 0;", "}"]
    src, exe = d / "probe.c", d / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([CC, "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, name, off, size = line.split()
        out[(cname, None if name == "-" else name)] = (int(off), int(size))
    return out


def test_every_field_of_the_mirror_sits_where_the_header_puts_it(probe):
    mirror = _mirror()
    assert probe.keys() == mirror.keys()
    bad = [(k, probe[k], mirror[k]) for k in mirror if probe[k] != mirror[k]]
    assert not bad, f"{len(bad)} fields differ (C offset, size) vs (ctypes offset, size), first: {bad[:4]}"

