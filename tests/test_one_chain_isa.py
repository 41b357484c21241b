"""CPU-only check of the gfx950 code of the two-level fast tick's one-chain form (hipcc cross-compiles, no GPU needed; the
compilation of tests/test_fast_kernel_isa.py, and of sai2b_self.hip the same way).

fast_tick<true> runs one whitened chain (on Mb or M), takes the operational-space factor and the nullspace direction from
one Householder QR of Yx, and recovers the MotionForceTask torques through the chain (csrc/sai2b_chain.h); its parent ran
the chain twice, formed two Gram matrices with a 6 x 6 Cholesky each, searched for the nullspace direction with seven
solves and re-orthogonalised it. Asserted for tick_fast_kernel<2, true | false> and tick_self_kernel<2, true | false>:
  * the static count of instructions with `_f64` in their name is at least 500 below the parent's (one chain plus its
    solves is about 480 of them, the search replaced by QR about another 300; the margin is for contraction differences);
  * amdhsa_next_free_vgpr is not above the parent's.
The parent's figures, measured by compiling the commit before this change with the same toolchain and flags (ROCm 7.2
hipcc), as `_f64` instructions / next_free_vgpr:
    tick_fast_kernel<2, true>  4 514 / 372      tick_fast_kernel<2, false>  5 326 / 392
    tick_self_kernel<2, true> 14 688 / 512      tick_self_kernel<2, false> 15 499 / 512
This form measured 3 969 / 362, 4 756 / 392, 14 142 / 512 and 14 930 / 512; scratch 32 / 32 / 384 / 384 B as the parent's.
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
# (unit, kernel, FAST x BAKED): the parent's `_f64` instruction count and next_free_vgpr
PARENT = {
    ("sai2b_kernels", "tick_fast_kernel", "ILi2ELb1E"): (4514, 372),
    ("sai2b_kernels", "tick_fast_kernel", "ILi2ELb0E"): (5326, 392),
    ("sai2b_self", "tick_self_kernel", "ILi2ELb1E"): (14688, 512),
    ("sai2b_self", "tick_self_kernel", "ILi2ELb0E"): (15499, 512),
}
F64_MARGIN = 500

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda.h")):  # generated header (build() makes it too)
        subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
    tmp = tmp_path_factory.mktemp("isa")
    units = sorted({u for u, _, _ in PARENT})
    outs = {u: str(tmp / (u + "_n7.s")) for u in units}
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", u + ".hip", "-o", outs[u]], cwd=CSRC)
             for u in units]
    assert [p.wait() for p in procs] == [0] * len(units)
    found = {}
    for u in units:
        text = open(outs[u]).read()
        for m in re.finditer(r"^(_ZN\w*?(tick_fast_kernel|tick_self_kernel)(\w+?)EEvPK\w*):", text, re.M):
            end = text.index(".Lfunc_end", m.end())
            body = [l.strip() for l in text[m.end():end].splitlines()]
            ins = [l for l in body if l and not l.startswith((".", ";")) and not l.endswith(":")]
            desc = text.index(".amdhsa_kernel " + m.group(1) + "\n")
            meta = text[desc:text.index(".end_amdhsa_kernel", desc)]
            found[(u, m.group(2), m.group(3))] = (ins, meta)
    return found


@pytest.mark.parametrize("key", list(PARENT), ids=[f"{k[1]}{k[2]}" for k in PARENT])
def test_one_chain_fewer(kernels, key):
    ins, meta = kernels[key]
    f64, vgpr = PARENT[key]
    n = sum("_f64" in l for l in ins)
    regs = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
    print(f"{key[1]}<{key[2]}>: {n} _f64 instructions (parent {f64}), next_free_vgpr {regs} (parent {vgpr}), scratch {scratch} B")
    assert n <= f64 - F64_MARGIN
    assert regs <= vgpr
