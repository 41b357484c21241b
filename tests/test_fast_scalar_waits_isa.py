"""CPU-only check of the gfx950 code of the headline kernels (FAST = 2): how often a wavefront parks at a wait for a
batch-uniform parameter or for q (no GPU needed: hipcc cross-compiles).

Counted in the text of the kernel, in program order, without following branches:
  scalar round trip  an s_waitcnt on lgkmcnt that has an s_load* issued since the previous wait on that counter
  q wait             an s_waitcnt on vmcnt that has a plain global_load issued since the previous wait on that counter

The body reads its parameters from the FastBlock (csrc/sai2b_params.h), one group per phase, each group as one burst of wide
scalar loads behind one wait; q is loaded seven times over and waited for once.

Figures of the parent commit (the body read DevTask field by field), by this same counter:

  kernel                        scalar round trips   v_writelane + v_readlane
  tick_fast_kernel<2, true>             90                    0
  tick_fast_kernel<2, false>           112                  280
  tick_self_kernel<2, true>             93                  160
  tick_self_kernel<2, false>           110                  651

(PARENT[...] below; the self kernels' totals include the lanes-per-robot tail behind the body, which this change leaves alone.)
This form measured 52 / 0, 72 / 270, 51 / 160 and 71 / 520 (the batch size is asked for a second time behind the window: the
row stride made from the entry's copy was spilled ahead of the window and fetched back six times behind it). On the path the library's defaults take, <2, true> executes
about ten round trips where the parent executed 45 to 50.
Where the law's gains are fetched is chosen per kernel (JtLate<EARLY>, csrc/sai2b_fast.hpp): behind the QR in the BAKED forms,
so that no round trip is left in the law; at the top of the law, one burst per use_vsat branch, in the others.
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
# (file, kernel, instance): FAST = 2 x BAKED of the two-launch and of the self form
KERNELS = [("sai2b_kernels.hip", "tick_fast_kernel", "ILi2ELb1E"), ("sai2b_kernels.hip", "tick_fast_kernel", "ILi2ELb0E"),
           ("sai2b_self.hip", "tick_self_kernel", "ILi2ELb1E"), ("sai2b_self.hip", "tick_self_kernel", "ILi2ELb0E")]
IDS = ["fast-baked", "fast", "self-baked", "self"]
# the parent commit: (scalar round trips, v_writelane + v_readlane), measured with count() below
PARENT = {
    ("tick_fast_kernel", "ILi2ELb1E"): (90, 0),
    ("tick_fast_kernel", "ILi2ELb0E"): (112, 280),
    ("tick_self_kernel", "ILi2ELb1E"): (93, 160),
    ("tick_self_kernel", "ILi2ELb0E"): (110, 651),
}
MIN_DROP = 30

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


def kernel_lines(text, kernel, inst):
    """Instructions and SAI2B marker comments of one kernel, in program order."""
    m = re.search(r"^(_ZN\w*" + kernel + inst + r"EEvPK\w*):", text, re.M)
    assert m, f"{kernel}{inst} not in the assembly"
    body = [l.strip() for l in text[m.end():text.index(".Lfunc_end", m.end())].splitlines()]
    return [l for l in body if l and (l.startswith("; SAI2B_") or not l.startswith((".", ";"))) and not l.endswith(":")]


def count(lines):
    """(positions of the scalar round trips, positions of the q waits) in `lines`."""
    trips, qwaits = [], []
    smem = vmem = False
    for i, l in enumerate(lines):
        if l.startswith("s_load"):
            smem = True
        elif l.startswith("global_load") and not l.startswith("global_load_lds"):
            vmem = True
        elif l.startswith("s_waitcnt"):
            if "lgkmcnt" in l:
                if smem:
                    trips.append(i)
                smem = False
            if "vmcnt" in l:
                if vmem:
                    qwaits.append(i)
                vmem = False
    return trips, qwaits


def lanes(lines):
    return sum(l.startswith(("v_writelane", "v_readlane")) for l in lines)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda.h")):  # generated header (build() makes it too)
        subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
    tmp = tmp_path_factory.mktemp("isa")
    files = sorted({k[0] for k in KERNELS})
    procs = []
    for f in files:  # the two files side by side
        out = str(tmp / (f + ".s"))
        procs.append((f, out, subprocess.Popen([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", f, "-o", out], cwd=CSRC)))
    text = {}
    for f, out, p in procs:
        assert p.wait() == 0, f
        text[f] = open(out).read()
    return text


@pytest.fixture(scope="module", params=KERNELS, ids=IDS)
def kern(request, asm):
    f, kernel, inst = request.param
    lines = kernel_lines(asm[f], kernel, inst)
    trips, qwaits = count(lines)
    print(f"{kernel}{inst}: {len(lines)} instructions, {len(trips)} scalar round trips, {lanes(lines)} lane moves")
    return (kernel, inst), lines, trips, qwaits


def test_q_in_one_round_trip(kern):
    _, lines, trips, qwaits = kern
    first = next(i for i, l in enumerate(lines) if l.startswith("global_load_lds"))
    n = [i for i in qwaits if i < first]
    print("q waits before the first DMA:", len(n))
    assert len(n) == 1, [lines[i] for i in n]


def test_entry_and_dma_do_not_wait_for_row_bases(kern):
    _, lines, trips, _ = kern
    first = next(i for i, l in enumerate(lines) if l.startswith("global_load_lds"))
    # the even-batch branch is the one that moves 16 bytes per lane
    even = [i for i, l in enumerate(lines) if l.startswith("global_load_lds_dwordx4")]
    assert even, "no 16-byte DMA: the even-batch branch is gone"
    entry = [i for i in trips if i < first]
    inside = [i for i in trips if even[0] < i < even[-1]]
    print("scalar round trips: kernel entry to the first DMA", len(entry), "; inside the even-batch DMA", len(inside))
    assert len(entry) <= 4
    assert len(inside) <= 1


def test_joint_task_law_region(kern):
    _, lines, trips, _ = kern
    begin = [i for i, l in enumerate(lines) if l == "; SAI2B_MARK jt_law_begin"]
    end = [i for i, l in enumerate(lines) if l == "; SAI2B_MARK jt_law_end"]
    assert len(begin) == 1 and len(end) == 1 and begin[0] < end[0], (begin, end)
    inside = [i for i in trips if begin[0] < i < end[0]]
    print("scalar round trips in the JointTask law:", len(inside), "over", end[0] - begin[0], "lines")
    # both use_vsat loops lie inside the region: the code of each is there, not moved out of line
    assert sum(l.startswith("v_max_f64") or l.startswith("v_min_f64") for l in lines[begin[0]:end[0]]) >= 14
    assert len(inside) <= 2


def test_static_total_and_lane_moves(kern):
    key, lines, trips, _ = kern
    parent_trips, parent_lanes = PARENT[key]
    print(f"{key}: scalar round trips {len(trips)} (parent {parent_trips}), lane moves {lanes(lines)} (parent {parent_lanes})")
    assert len(trips) <= parent_trips - MIN_DROP
    assert lanes(lines) <= parent_lanes
