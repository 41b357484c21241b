"""CPU-only check of the gfx950 code of tick_self_kernel<2, *> (no GPU needed: hipcc cross-compiles): the headline tick in one
launch, the SVD-free body followed in the same wavefront by the lanes-per-robot generic tick of the robots it declined.

The tail must cost the fast wavefronts nothing. What it can spoil, and what is held here:
  * the DMA window of the fast body (tests/test_fast_kernel_isa.py): from the first global_load_lds to the wait that retires
    the last one no plain global load, no scratch or buffer access, no ds_read. (A tail given the kernel's restrict parameter
    pointer turned every parameter read of the body into a vector load inside the window.)
  * the window's length: at least the two-launch kernel's 2 044 instructions from the first DMA to the wait, minus 5 %;
  * LDS: the pads of the tail alias the input image, 4 workgroups per CU still fit;
  * the private segment: that of tick_group_kernel<16, false> of the same build (the tail is that kernel's code) plus the fast
    body's own 32 B, never the 2 KB of a tail behind a call.
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
INSTANCES = ["ILi2ELb1E", "ILi2ELb0E"]	# FAST = 2 x BAKED
LDS_MAX = 40960	 # 4 single-wavefront workgroups per CU (160 KiB)
PARENT_WINDOW = 2044  # tick_fast_kernel<2, true>: instructions from the first DMA to the wait behind the last
WINDOW_MIN = PARENT_WINDOW - PARENT_WINDOW * 5 // 100
SCRATCH_OVER_GROUP = 32	 # bytes per lane the fast body may add to the group tick's private segment

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


def _kernels(text, pattern):
	"""{template arguments as mangled: (instructions, kernel descriptor)} of the kernels whose symbol matches"""
	found = {}
	for m in re.finditer(pattern, text, re.M):
		end = text.index(".Lfunc_end", m.end())
		body = [l.strip() for l in text[m.end():end].splitlines()]
		ins = [l for l in body if l and not l.startswith((".", ";")) and not l.endswith(":")]
		desc = text.index(".amdhsa_kernel " + m.group(1) + "\n")
		found[m.group(2)] = (ins, text[desc:text.index(".end_amdhsa_kernel", desc)])
	return found


@pytest.fixture(scope="module")
def build(tmp_path_factory):
	hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
	if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda.h")):	 # generated header (build() makes it too)
		subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
	tmp = tmp_path_factory.mktemp("isa")
	text = {}
	for unit in ("sai2b_self", "sai2b_group"):
		out = str(tmp / (unit + "_n7.s"))
		subprocess.run([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", unit + ".hip", "-o", out], cwd=CSRC, check=True)
		text[unit] = open(out).read()
	self_k = _kernels(text["sai2b_self"], r"^(_ZN\w*tick_self_kernel(\w+?)EEvPK\w*):")
	group_k = _kernels(text["sai2b_group"], r"^(_ZN\w*tick_group_kernel(\w+?)EEvPK\w*):")
	return self_k, group_k["ILi16ELb0E"]


def _field(meta, name):
	return int(re.search(r"\." + name + r"\s+(\d+)", meta).group(1))


@pytest.mark.parametrize("inst", INSTANCES)
def test_tail_leaves_the_fast_body_as_it_was(build, inst):
	self_k, (_, group_meta) = build
	ins, meta = self_k[inst]
	glds = [i for i, l in enumerate(ins) if l.startswith("global_load_lds")]
	assert glds, "no global_load_lds: the inputs are not staged"
	first, last = glds[0], glds[-1]
	wait = next(i for i in range(last, len(ins)) if re.match(r"s_waitcnt\b.*vmcnt\(0\)", ins[i]))
	window = ins[first:wait]
	plain = [l for l in window if l.startswith("global_load") and not l.startswith("global_load_lds")]
	spill = [l for l in window if l.startswith(("scratch_", "buffer_"))]
	lds_reads = [l for l in window if l.startswith("ds_read")]
	lds, scratch = _field(meta, "amdhsa_group_segment_fixed_size"), _field(meta, "amdhsa_private_segment_fixed_size")
	group_scratch = _field(group_meta, "amdhsa_private_segment_fixed_size")
	valu = sum(l.startswith("v_") for l in ins)
	print(f"tick_self_kernel<{inst}>: {len(ins)} instructions, {valu} VALU, window first DMA {first} / last DMA {last} / wait {wait} "
		  f"({wait - first} long, at least {WINDOW_MIN} asked), in it {len(plain)} plain global loads, {len(spill)} scratch or buffer "
		  f"accesses, {len(lds_reads)} ds_read; LDS {lds} B, private segment {scratch} B (tick_group_kernel<16, false>: {group_scratch} B), "
		  f"s_load {sum(l.startswith('s_load') for l in ins)}")
	assert not plain, f"{len(plain)} plain global loads while the DMA is in flight, first: {plain[:3]}"
	assert not spill, f"{len(spill)} scratch or buffer accesses while the DMA is in flight, first: {spill[:3]}"
	assert not lds_reads, "the image is read before the wait that retires the DMA"
	assert lds <= LDS_MAX
	assert scratch <= group_scratch + SCRATCH_OVER_GROUP, (scratch, group_scratch)
	assert wait - first >= WINDOW_MIN, (first, last, wait)
