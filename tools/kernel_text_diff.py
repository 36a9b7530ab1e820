#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  CPU only.

    tools/kernel_text_diff.py OLD [OLD ...] NEW [--rename REGEX=REPL ...] [--show N]

OLD and NEW are AMDGPU assembly files (.s), or .hip files, which are compiled with
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S
Several OLD files pool their kernels, so that two files can be held against the one that replaces them.
Kernels are paired by symbol.  --rename rewrites symbols (of both files, re.sub) before pairing, so that an experimental
instantiation can be held against the kernel it should equal, e.g. a 64-token instantiation of a split kernel:
    --rename '15k_tfm_qkv_split(ILi\\d+ELi\\d+E)Li4E=9k_tfm_qkv\\1'
For every kernel one line: `same` or `differs` for its instruction text after comments, whitespace, assembler
directives and symbol names are taken out and local labels are numbered in order of appearance, then the VGPR / AGPR /
SGPR / LDS / scratch figures of the code object's metadata on both sides.  The text is only compared, never looked into.
Exit status 1 if any text or figure differs or a kernel has no partner."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = ["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
FIGURES = [("vgpr", "vgpr_count"), ("agpr", "agpr_count"), ("sgpr", "sgpr_count"),
           ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size")]


def assembly(path, tmp):
    if not path.endswith(".hip"):
        return open(path).read()
    out = os.path.join(tmp, "%d_%s.s" % (len(os.listdir(tmp)), os.path.basename(path)))
    r = subprocess.run(HIPCC + [path, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s does not compile:\n%s" % (path, r.stderr[-3000:]))
    return open(out).read()


def kernels(asm):
    """{symbol: (normalised text lines, {figure: value})}"""
    meta = {}
    notes = asm[asm.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - (?=\.)", notes)[1:]:
        entry = entry.split("\namdhsa.")[0]
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M).group(1)
        meta[name] = {short: int(re.search(r"^\s*\.%s:\s+(\d+)" % key, entry, re.M).group(1)) for short, key in FIGURES}
    res = {}
    for sym, fig in meta.items():
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), asm, re.S | re.M)
        if not m:
            sys.exit("no text for kernel %s" % sym)
        labels, lines = {}, []
        for line in m.group(1).split("\n.section")[0].split("\n\t.section")[0].splitlines():
            line = " ".join(line.split(";")[0].split())
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue                                    # comment, blank or directive
            line = re.sub(r"\b_Z\w+", "SYM", line)
            line = re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), "L%d" % len(labels)), line)
            lines.append(line)
        res[sym] = (lines, fig)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old", nargs="+")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N differing lines of a kernel")
    args = ap.parse_args()

    def renamed(ks):
        out = {}
        for sym, v in ks.items():
            for r in args.rename:
                pat, _, repl = r.partition("=")
                sym = re.sub(pat, repl, sym)
            out[sym] = v
        return out

    with tempfile.TemporaryDirectory() as tmp:
        old = {}
        for path in args.old:
            ks = renamed(kernels(assembly(path, tmp)))
            if set(ks) & set(old):
                sys.exit("%s: kernels already seen in an earlier OLD: %s" % (path, ", ".join(sorted(set(ks) & set(old)))))
            old.update(ks)
        new = renamed(kernels(assembly(args.new, tmp)))
    same = differs = figures = 0
    for sym in sorted(set(old) & set(new)):
        (to, fo), (tn, fn) = old[sym], new[sym]
        equal = to == tn
        same, differs = same + equal, differs + (not equal)
        figures += fo != fn
        fig = " ".join("%s %d" % (k, fo[k]) if fo[k] == fn[k] else "%s %d -> %d" % (k, fo[k], fn[k]) for k, _ in FIGURES)
        print("%-7s %s  %s%s" % ("same" if equal else "differs", sym, fig, "" if fo == fn else "  FIGURES DIFFER"))
        if not equal and args.show:
            for d in [d for d in difflib.unified_diff(to, tn, "old", "new", n=0, lineterm="") if d[:2] not in ("--", "++")][:args.show]:
                print("    " + d)
    alone = sorted(set(old) ^ set(new))
    for sym in alone:
        print("only in %s: %s" % ("old" if sym in old else "new", sym))
    print("%d kernels compared: %d same, %d differ; figures differ in %d; %d without a partner"
          % (same + differs, same, differs, figures, len(alone)))
    return 1 if differs or figures or alone else 0


if __name__ == "__main__":
    sys.exit(main())
