"""CPU-only check of the gfx950 code of the four instantiations of sim_kernel<PL, CT> (sai2b_sim.hip compiled with
--cuda-device-only -S, in the manner of tests/test_payload_kernel_isa.py): plant payload x contact.

sim_kernel<NoPayload, NoContact> is what a context runs that has set neither, and must cost what the kernel cost before
either feature existed. The ONE sim_kernel of the commit before payloads (f262aaf), compiled with the same flags (hipcc of
ROCm 7, gfx950, -DSAI2B_N=7), measured VGPR / AGPR / scratch bytes per lane, and code size, none of which may grow:

    256 / 218 / 0, 36 604 bytes of code (one wave per SIMD)

The four instantiations must also differ in code size in the expected order (the bare one smallest, payload + contact
largest): a policy type that compiles to nothing would be noticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-DSAI2B_N=7", "-include", "sai2b_dof_rename.h"]
BASELINE_BEFORE_PAYLOADS = dict(vgpr=256, agpr=218, scratch=0, size=36604)
FORMS = [("NoPayload", "NoContact"), ("Payload", "NoContact"), ("NoPayload", "Contact"), ("Payload", "Contact")]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


def _field(meta, name):
    return int(re.search(r"\." + name + r"\s+(\d+)", meta).group(1))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda.h")):  # generated header (build() makes it too)
        subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
    out = str(tmp_path_factory.mktemp("isa") / "sim_n7.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", "sai2b_sim.hip", "-o", out], cwd=CSRC, check=True)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_ZN\w*sim_kernelINS\w*?_\d+((?:No)?Payload)ENS\w*?_\d+((?:No)?Contact)E\w*):", text, re.M):
        desc = text.index(".amdhsa_kernel " + m.group(1) + "\n")
        meta = text[desc:text.index(".end_amdhsa_kernel", desc)]
        size = int(re.search(r"; codeLenInByte = (\d+)", text[m.end():text.index(".Lfunc_end", m.end()) + 4000]).group(1))
        tail = text[m.end():text.index(".Lfunc_end", m.end()) + 4000]
        found[(m.group(2), m.group(3))] = dict(vgpr=int(re.search(r"; NumVgprs: (\d+)", tail).group(1)),
                                               agpr=int(re.search(r"; NumAgprs: (\d+)", tail).group(1)),
                                               scratch=_field(meta, "amdhsa_private_segment_fixed_size"), size=size)
    return found


def test_all_four_instantiations_exist(kernels):
    for f in FORMS:
        print(f, kernels.get(f))
    assert set(kernels) == set(FORMS)


def test_bare_instantiation_costs_what_the_kernel_cost_before_payloads(kernels):
    k = kernels[("NoPayload", "NoContact")]
    for name, bound in BASELINE_BEFORE_PAYLOADS.items():
        assert k[name] <= bound, (name, k[name], bound)


def test_code_sizes_are_ordered(kernels):
    s = {f: kernels[f]["size"] for f in FORMS}
    bare, both = s[("NoPayload", "NoContact")], s[("Payload", "Contact")]
    assert bare < s[("Payload", "NoContact")] < both and bare < s[("NoPayload", "Contact")] < both, s
