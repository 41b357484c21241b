"""CPU-only check of the gfx950 code of tick_fast_payload_kernel<2>, the headline tick's form for contexts with per-robot
payloads: the same staged input path as tick_fast_kernel<2> (tests/test_fast_kernel_isa.py, whose checks these are), with the
ten payload rows added to the staged image (34 048 + 10 * 64 * 8 = 39 168 bytes).

As measured when this was written (hipcc of ROCm 7, gfx950; VGPR / AGPR / scratch / LDS): the form with the compile-time Panda
(ILi2ELb1E) 256 / 252 / 32 B / 39 168 B, the form that reads the model from the parameter block (ILi2ELb0E) 256 / 256 / 96 B /
39 168 B; the forms without payload 256 / 208 / 32 / 34 048 and 256 / 224 / 32 / 34 048.

Every per-robot input row but q reaches the kernel by global_load_lds (DMA into LDS) at entry, and the model phase
runs while the DMA is in flight. That overlap holds only while the span between the first DMA and the wait that
retires it issues no ordinary global load and no scratch or buffer access: hipcc answers any of them with a
vmcnt(0) that drains the DMA early (a spill in that span is the usual way back). The LDS image must also leave room
for 4 workgroups per CU.
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
INSTANCES = ["ILi2ELb1E", "ILi2ELb0E"]	# FAST = 2 x BAKED; FAST = 1 keeps its inputs in registers
LDS_MAX = 40960	 # 4 single-wavefront workgroups per CU (160 KiB)
SCRATCH_MAX = {"ILi2ELb1E": 32, "ILi2ELb0E": 96}  # bytes per lane as measured, all of it after the window

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
	hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
	if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda.h")):	 # generated header (build() makes it too)
		subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
	out = str(tmp_path_factory.mktemp("isa") / "kernels_n7.s")
	subprocess.run([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", "sai2b_kernels.hip", "-o", out],
				   cwd=CSRC, check=True)
	text = open(out).read()
	found = {}
	for m in re.finditer(r"^(_ZN\w*tick_fast_payload_kernel(\w+?)EEvPK\w*):", text, re.M):
		end = text.index(".Lfunc_end", m.end())
		body = [l.strip() for l in text[m.end():end].splitlines()]
		ins = [l for l in body if l and not l.startswith((".", ";")) and not l.endswith(":")]
		desc = text.index(".amdhsa_kernel " + m.group(1) + "\n")
		meta = text[desc:text.index(".end_amdhsa_kernel", desc)]
		found[m.group(2)] = (ins, meta)
	return found


def _field(meta, name):
	return int(re.search(r"\." + name + r"\s+(\d+)", meta).group(1))


@pytest.mark.parametrize("inst", INSTANCES)
def test_staged_window_is_clean(kernels, inst):
	ins, meta = kernels[inst]
	glds = [i for i, l in enumerate(ins) if l.startswith("global_load_lds")]
	assert glds, "no global_load_lds: the inputs are not staged"
	first, last = glds[0], glds[-1]
	wait = next(i for i in range(last, len(ins)) if re.match(r"s_waitcnt\b.*vmcnt\(0\)", ins[i]))
	bad = [l for l in ins[first:wait]
		   if (l.startswith("global_load") and not l.startswith("global_load_lds")) or l.startswith(("scratch_", "buffer_"))]
	assert not bad, f"{len(bad)} forbidden instructions while the DMA is in flight, first: {bad[:3]}"
	# the image is read only after that wait
	assert not any(l.startswith("ds_read") for l in ins[first:wait])
	# the payload rows are part of the image
	assert _field(meta, "amdhsa_group_segment_fixed_size") == 39168 <= LDS_MAX
	assert _field(meta, "amdhsa_private_segment_fixed_size") <= SCRATCH_MAX[inst]
