"""CPU-only check of the gfx950 code of tick_fast_kernel<2, *>'s one-FK form (hipcc cross-compiles, no GPU needed; the
same compilation as tests/test_fast_kernel_isa.py).

The kernel evaluates forward kinematics once: CRBA and gravity run inside the DMA window from the frames the Jacobian
was built from, and M and g are parked in LDS there instead of being recomputed from a second FK behind the control law.
Asserted for <2, true> (Panda constants baked) and <2, false>:
  * at least one ds_write lies between the last global_load_lds and the vmcnt(0) that retires the DMA: M and g are
    written to LDS inside the window;
  * the static count of instructions with `_f64` in their name is at least 350 below the two-FK parent's (one FK is
    about 440 of them; the margin is for FMA-contraction differences);
  * amdhsa_next_free_vgpr is not above the parent's.
The parent's figures, measured by compiling the commit before this change with the same toolchain and flags
(ROCm 7.2 hipcc): `_f64` instructions 5 642 / 5 796, next_free_vgpr 464 / 480 for <2, true> / <2, false>. This form
measured 5 203 / 5 326 and 374 / 392.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-DSAI2B_N=7", "-include", "sai2b_dof_rename.h"]
# FAST = 2 x BAKED: the two-FK parent's `_f64` instruction count and next_free_vgpr
PARENT = {"ILi2ELb1E": (5642, 464), "ILi2ELb0E": (5796, 480)}
F64_MARGIN = 350

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda.h")):  # generated header (build() makes it too)
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


@pytest.mark.parametrize("inst", list(PARENT))
def test_model_results_are_parked_inside_the_window(kernels, inst):
    ins, _ = kernels[inst]
    last = max(i for i, l in enumerate(ins) if l.startswith("global_load_lds"))
    wait = next(i for i in range(last, len(ins)) if re.match(r"s_waitcnt\b.*vmcnt\(0\)", ins[i]))
    parked = [l for l in ins[last:wait] if l.startswith("ds_write")]
    print(f"{inst}: {len(parked)} ds_write in the {wait - last} instructions between the last DMA and its wait")
    assert parked, "no LDS write between the last DMA and the wait that retires it: M and g are not parked in the window"


@pytest.mark.parametrize("inst", list(PARENT))
def test_one_forward_kinematics_fewer(kernels, inst):
    ins, meta = kernels[inst]
    f64, vgpr = PARENT[inst]
    n = sum("_f64" in l for l in ins)
    regs = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
    print(f"{inst}: {n} _f64 instructions (parent {f64}), next_free_vgpr {regs} (parent {vgpr})")
    assert n <= f64 - F64_MARGIN
    assert regs <= vgpr
