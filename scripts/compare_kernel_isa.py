#!/usr/bin/env python3
"""compare_kernel_isa.py <dir A> <dir B>: is the device code of two states of csrc/ the same? Each directory holds
<unit>_n<N>.s for the device translation units of the Makefile and N = 4, 6, 7, 8, made in csrc/ of either state with

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DSAI2B_N=<N> -include sai2b_dof_rename.h --cuda-device-only -S <unit>.hip
  (sai2b_otg.hip and sai2b_env_sampler.hip: with -ffp-contract=off, as the Makefile builds them)

Compared per kernel: the .amdhsa_* descriptor block and the instruction lines (directives and comments dropped, as
tests/test_fast_kernel_isa.py filters them). Exit status 0 when every kernel of every unit is the same."""
import os
import re
import sys

UNITS = ["sai2b_kernels", "sai2b_self", "sai2b_cert", "sai2b_group", "sai2b_otg", "sai2b_sim", "sai2b_observe", "sai2b_action", "sai2b_snapshot", "sai2b_hardware",
         "sai2b_env_sampler", "sai2b_joint_sensor", "sai2b_collision", "sai2b_ik"]


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n", text, re.M):
        name = m.group(1)
        meta = text[m.end():text.index(".end_amdhsa_kernel", m.end())]
        meta = [l.split(";")[0].strip() for l in meta.splitlines() if l.strip()]
        start = re.search(r"^" + re.escape(name) + r":.*$", text, re.M).end()
        end = text.index(".Lfunc_end", start)
        # Local labels (.LBB<function>_<block>, .Lpost_getpc<k> of a long branch) are numbered through the whole file, so they
        # move with the order the kernels are emitted in: renamed per kernel by first appearance, and their definitions kept
        # in the compared stream so that every branch still has to land on the same instruction.
        names = {}
        canon = lambda m: names.setdefault(m.group(0), f".L{len(names)}")
        body = [l.split(";")[0].strip() for l in text[start:end].splitlines()]
        ins = [re.sub(r"\.L\w+", canon, l) for l in body if l and (l.startswith(".L") and l.endswith(":") or not l.startswith(".") and not l.endswith(":"))]
        out[name] = (meta, ins)
    return out


a_dir, b_dir = sys.argv[1], sys.argv[2]
print(f"{'translation unit':<16} {'N':>2} {'kernels':>8} {'same set':>9} {'descriptors':>12} {'instructions':>13}")
bad = 0
for u in UNITS:
    for n in (4, 6, 7, 8):
        # a unit the second state adds (no size of it in the first directory) has nothing to be compared with; one missing
        # file of a unit the first state has is an error (kernels() fails on it)
        if not any(os.path.exists(f"{a_dir}/{u}_n{m}.s") for m in (4, 6, 7, 8)):
            print(f"{u:<16} {n:>2} {len(kernels(f'{b_dir}/{u}_n{n}.s')):>8} {'new unit':>9}")
            continue
        a, b = kernels(f"{a_dir}/{u}_n{n}.s"), kernels(f"{b_dir}/{u}_n{n}.s")
        same_set = set(a) == set(b)
        common = set(a) & set(b)
        dm = [k for k in common if a[k][0] != b[k][0]]
        im = [k for k in common if a[k][1] != b[k][1]]
        print(f"{u:<16} {n:>2} {len(b):>8} {'yes' if same_set else 'NO':>9} {'identical' if not dm else 'DIFFER':>12} {'identical' if not im else 'DIFFER':>13}")
        for k in sorted(set(a) ^ set(b)):
            print("   only in", "parent" if k in a else "PR", k)
        for k in sorted(set(dm) | set(im)):
            print("   differs:", k, len(a[k][1]), "->", len(b[k][1]), "instructions")
        bad += (not same_set) + len(dm) + len(im)
sys.exit(1 if bad else 0)
