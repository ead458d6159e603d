"""Code-shape table of every kernel that runs the MFMA tile engine, from `hipcc -S --cuda-device-only` listings made with
build.py's flags (no GPU needed):

    python scratch/r10/isa_table.py LISTING.s [LISTING.s ...]

Per kernel with MFMAs: NumVgprs, ScratchSize, Occupancy, and for its steady-state loop (the innermost loop with the most
MFMAs) the MFMA count and the longest run of consecutive MFMAs that accumulate into the same registers (other instructions
between two MFMAs do not end a run; the loop's back edge is followed once).
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def kernels(path):
    name, body = None, []
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
            elif name is not None:
                body.append(line)
                if re.match(r"^; Occupancy: ", line):      # (the resource comments follow .Lfunc_end)
                    yield name, body
                    name = None


def longest_run(dsts):
    best, run = (1 if dsts else 0), 1
    seq = dsts + dsts[:1]                      # once around the back edge
    for a, b in zip(seq, seq[1:]):
        run = run + 1 if a == b else 1
        best = max(best, run)
    return min(best, len(dsts))


def analyse(body):
    meta = {}
    for line in body:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", line)
        if m:
            meta[m.group(1)] = int(m.group(2))
    # innermost loops: from an "Inner Loop Header" label to the first backward branch to it
    best = []
    i = 0
    while i < len(body):
        m = re.match(r"^(\.LBB\d+_\d+):", body[i])
        if m and "Inner Loop Header" in body[i] + (body[i + 1] if i + 1 < len(body) else ""):   # (nested: on the next line)
            j = i + 1
            while j < len(body) and not re.search(r"s_cbranch\w*\s+%s\b" % re.escape(m.group(1)), body[j]):
                j += 1
            dsts = [re.search(r"v_mfma\w+\s+([av]\[\d+:\d+\])", ln).group(1) for ln in body[i:j] if "v_mfma" in ln]
            if len(dsts) > len(best):
                best = dsts
            i = j
        i += 1
    total = sum("v_mfma" in ln for ln in body)
    if not best:   # K loop unrolled or not an innermost loop (it holds a branch): every MFMA of the kernel, in listing order
        best = [re.search(r"v_mfma\w+\s+([av]\[\d+:\d+\])", ln).group(1) for ln in body if "v_mfma" in ln]
    return meta, total, best


def main():
    rows = []
    for path in sys.argv[1:]:
        for name, body in kernels(path):
            meta, total, loop = analyse(body)
            if total:
                rows.append((name, meta, len(loop), longest_run(loop)))
    names = demangle([r[0] for r in rows])
    print("%-8s %-8s %-9s %-10s %-8s %s" % ("NumVgprs", "Scratch", "Occupancy", "loop MFMAs", "max run", "kernel"))
    for name, meta, nloop, run in rows:
        short = re.sub(r"\(anonymous namespace\)::", "", names[name])
        short = re.sub(r"\(.*", "", re.sub(r"^void ", "", short))
        print("%-8d %-8d %-9d %-10d %-8d %s" % (meta.get("NumVgprs", -1), meta.get("ScratchSize", -1), meta.get("Occupancy", -1), nloop, run, short))


if __name__ == "__main__":
    main()
