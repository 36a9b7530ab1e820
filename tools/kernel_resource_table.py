"""Register, scratch and code-size table of two builds of kernels.hip, conv_any.hip and edge_split.hip, from the
compiler's assembly:
  tools/kernel_resource_table.py PARENT_DIR NEW_DIR > profiles/layer_kernels_resources.txt
Each directory holds kernels.s and conv_any.s, and edge_split.s where the build has that file (a unit only NEW_DIR has
is listed with its own figures), made with
  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S p3achygo_amd/csrc/X.hip -o DIR/X.s
One row per kernel: VGPRs (with AGPRs), SGPRs, ScratchSize, spilled VGPRs + SGPRs, code bytes, parent -> new; then the
scratch instructions of every k_init by loop depth.  Needs no GPU."""
import collections
import os
import re
import subprocess
import sys

COLS = ("vgpr", "sgpr", "scratch", "spills", "code")


def kernels(path):
    asm = open(path).read()
    spills = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S):
        spills[m.group(1)] = sum(int(v) for v in re.findall(r"\.[sv]gpr_spill_count: (\d+)", m.group(2)))
    out = {}
    for m in re.finditer(r"^(_ZN2p3\w+):\s", asm, re.M):
        name, end = m.group(1), asm.index(".Lfunc_end", m.start())
        meta = asm[end:end + 4000]
        if name not in spills or "; ScratchSize" not in meta:
            continue
        get = lambda pat: int(re.search(pat, meta).group(1))
        depth, ops = 0, collections.Counter()
        for line in asm[m.start():end].split("\n"):
            d = re.search(r"^\.LBB.*Depth=(\d+)", line.strip())
            if line.strip().startswith(".LBB"):
                depth = int(d.group(1)) if d else 0
            if "scratch_" in line:
                ops[depth] += 1
        out[name] = dict(vgpr=get(r"; TotalNumVgprs: (\d+)"), sgpr=get(r"; TotalNumSgprs: (\d+)"), scratch=get(r"; ScratchSize: (\d+)"),
                         spills=spills[name], code=get(r"; codeLenInByte = (\d+)"), ops=dict(sorted(ops.items())))
    return out


def main(parent, new):
    for unit in ("kernels.s", "conv_any.s", "edge_split.s"):
        if unit == "edge_split.s" and not os.path.exists(os.path.join(new, unit)):
            continue
        b = kernels(os.path.join(new, unit))
        a = kernels(os.path.join(parent, unit)) if os.path.exists(os.path.join(parent, unit)) else b   # new unit: its own figures
        assert set(a) == set(b), sorted(set(a) ^ set(b))
        names = subprocess.run(["c++filt"] + list(a), capture_output=True, text=True, check=True).stdout.split("\n")
        short = {n: re.sub(r"\(.*", "", d).replace("void ", "").replace("p3::", "") for n, d in zip(a, names)}
        print("== %s: %d kernels; parent -> new; '=' marks a row equal in every column" % (unit, len(a)))
        print("%-66s %-10s %-10s %-10s %-8s %-14s" % (("kernel",) + COLS))
        for n in sorted(a, key=short.get):
            same = all(a[n][c] == b[n][c] for c in COLS)
            cells = ["%d" % a[n][c] if a[n][c] == b[n][c] else "%d->%d" % (a[n][c], b[n][c]) for c in COLS]
            print("%-66s %-10s %-10s %-10s %-8s %-14s %s" % ((short[n],) + tuple(cells) + ("=" if same else "",)))
        for n in sorted(a, key=short.get):
            if "k_init" in short[n]:
                print("scratch instructions by loop depth, %s: parent %s, new %s" % (short[n], a[n]["ops"], b[n]["ops"]))
        print()


if __name__ == "__main__":
    main(*sys.argv[1:3])
