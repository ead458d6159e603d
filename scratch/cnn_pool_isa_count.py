"""Instruction counts per basic block of the 16-pixel forms of pool_pair_kernel (csrc/cnn_pool.hip), from the compiler's
listing: the breakdown quoted in profiles/r25_cnn_pool.txt.  Blocks of more than 60 instructions are printed with their
counts of vector, scalar, LDS-read, LDS-write, global-load and scratch instructions; the largest block with LDS reads and table
loads is one layer of a unit.

    python scratch/cnn_pool_isa_count.py        (runs hipcc -S on csrc/cnn_pool.hip with build.py's flags)
"""
import collections
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scale-mixtures-of-neural-network-gaussian-processes_amd")
FORMS = (("IfLi0ELi16E", "fp32 ReLU, 16 pixels per lane"), ("IdLi0ELi16E", "fp64 ReLU, 16 pixels per lane"))


def kind(op):
    for prefix, name in (("ds_read", "lds_read"), ("ds_write", "lds_write"), ("global_load", "global_load"),
                         ("scratch", "scratch"), ("s_", "scalar")):
        if op.startswith(prefix):
            return name
    return "vector"


def main():
    sys.path.insert(0, PKG)
    import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "cnn_pool.s")
        flags = [f for f in build.FLAGS if f != "-fPIC"]
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-S", "--cuda-device-only", "-o", out,
                                                                                  os.path.join(PKG, "csrc", "cnn_pool.hip")],
                       check=True, stderr=subprocess.DEVNULL)
        lines = open(out).read().split("\n")
    for tag, name in FORMS:
        start = next(i for i, l in enumerate(lines) if "pool_pair_kernel" + tag in l and l.startswith("_ZN") and ":" in l)
        blocks, cur = [], ["entry", []]
        for l in lines[start + 1:]:
            t = l.strip()
            if t.startswith("s_endpgm"):
                break
            if t.split(";")[0].strip().endswith(":"):
                blocks.append(cur)
                cur = [t.split(":")[0], []]
            elif t and not t.startswith((";", ".")):
                cur[1].append(t.split()[0])
        blocks.append(cur)
        print("%s: %d instructions" % (name, sum(len(b[1]) for b in blocks)))
        for label, ops in blocks:
            if len(ops) > 60:
                print("  %-10s %5d  %s" % (label, len(ops), dict(collections.Counter(kind(o) for o in ops))))


if __name__ == "__main__":
    main()
