"""CPU-only check (hipcc cross-compiles) that the baked headline kernels use the structure of the Panda's constants: their
model phase is written out from the nonzero terms (csrc/tools/gen_baked_model.cpp), which shows as fewer double-precision
VALU instructions than the generic functions on compile-time arrays gave.

Static counts of v_*_f64 instructions of tick_fast_kernel<2, true> / <1, true>, with the compile step of
tests/test_fast_kernel_isa.py. Before the written-out model phase they stood at 5 203 / 4 397; letting the compiler drop
the products with the zero literals it already knew (finite-math flags, as an experiment only) reached 422 / 406 fewer
without knowing anything of E and the inertias, so at least 400 fewer is what using the structure must give. Registers
must not rise above the 374 / 504 of before, and scratch stays within the 32 B of tests/test_fast_kernel_isa.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-DSAI2B_N=7", "-include", "sai2b_dof_rename.h"]
# instance: (v_*_f64 instructions, next_free_vgpr) of the generic model phase on PandaBaked's arrays
BEFORE = {"ILi2ELb1E": (5203, 374), "ILi1ELb1E": (4397, 504)}
F64_DROP_MIN = 400
SCRATCH_MAX = 32

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda_model.h")):  # generated headers (build() makes them too)
        subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
    out = str(tmp_path_factory.mktemp("isa") / "kernels_n7.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", "sai2b_kernels.hip", "-o", out],
                   cwd=CSRC, check=True)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_ZN\w*tick_fast_kernel(\w+?)EEvPK\w*):", text, re.M):
        end = text.index(".Lfunc_end", m.end())
        body = [l.strip() for l in text[m.end():end].splitlines()]
        ins = [l for l in body if l and not l.startswith((".", ";")) and not l.endswith(":")]
        desc = text.index(".amdhsa_kernel " + m.group(1) + "\n")
        meta = text[desc:text.index(".end_amdhsa_kernel", desc)]
        found[m.group(2)] = (ins, meta)
    return found


def _field(meta, name):
    return int(re.search(r"\." + name + r"\s+(\d+)", meta).group(1))


@pytest.mark.parametrize("inst", list(BEFORE))
def test_model_phase_uses_the_structure_of_the_constants(kernels, inst):
    ins, meta = kernels[inst]
    f64_before, vgpr_before = BEFORE[inst]
    f64 = sum(1 for l in ins if re.match(r"v_\w*_f64", l))
    valu = sum(1 for l in ins if l.startswith("v_"))
    vgpr, scratch = _field(meta, "amdhsa_next_free_vgpr"), _field(meta, "amdhsa_private_segment_fixed_size")
    print(f"{inst}: {f64} v_*_f64 of {valu} VALU ({f64_before} before), next_free_vgpr {vgpr} ({vgpr_before} before), scratch {scratch} B")
    assert f64 <= f64_before - F64_DROP_MIN, (f64, f64_before)
    assert vgpr <= vgpr_before, (vgpr, vgpr_before)
    assert scratch <= SCRATCH_MAX, scratch
