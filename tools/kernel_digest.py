#!/usr/bin/env python
"""Digest of every gfx950 kernel of a tree, to prove that a host-side change left the device code alone.

    python tools/kernel_digest.py [TREE] > digests.txt        (TREE: a checkout's root, default this one)

Compiles the device side of each unit alone, with frhip/build.py's flags of THAT tree, and prints one line
`unit  kernel  digest` per kernel symbol, sorted.  Two trees have the same device code when the two outputs are equal.
A kernel's digest covers its instruction lines and its .amdhsa_kernel block.  Comments and the per-function index of local
labels (.LBB7_3 -> .LBB_3) are dropped first: both follow the order of instantiation, which follows the host code.
Data outside a kernel's own text (a constant table in .rodata, a __device__ global) is not covered: a change confined to those goes unseen.
No GPU is needed.
"""
import hashlib
import os
import re
import runpy
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+_(\d+)")


def _clean(line):
    return LOCAL_LABEL.sub(r".L\1_\2", line.split(";", 1)[0].strip())


def kernel_digests(asm):
    """{kernel symbol: digest} of one unit's device assembly"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel", asm, flags=re.S | re.M):
        start = asm.index("\n%s:" % m.group(1))                             # the symbol's own label, in column 0
        body = asm[start:asm.index("\n.Lfunc_end", start)]
        lines = [_clean(line) for line in (body + "\n" + m.group(0)).splitlines()]
        out[m.group(1)] = hashlib.sha256("\n".join(line for line in lines if line).encode()).hexdigest()[:20]
    return out


def unit_digests(tree):
    """[(unit, kernel, digest)] of every unit that the tree's build.py compiles"""
    b = runpy.run_path(os.path.join(tree, "face-recognition-pytorch_amd", "frhip", "build.py"))

    def one(src):
        cmd = [b["HIPCC"]] + b["FLAGS"] + ["--cuda-device-only", "-S", os.path.join(b["CSRC"], src), "-o", "-"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stderr.decode(errors="replace")))
        return [(src, k, d) for k, d in kernel_digests(r.stdout.decode()).items()]

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return sorted(row for rows in pool.map(one, b["SOURCES"]) for row in rows)


if __name__ == "__main__":
    tree = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = unit_digests(os.path.abspath(tree))
    for row in rows:
        print("%s  %s  %s" % row)
    print("%d kernels in %d units" % (len(rows), len({r[0] for r in rows})), file=sys.stderr)
