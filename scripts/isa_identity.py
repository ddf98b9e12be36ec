#!/usr/bin/env python3
"""Do two trees compile csrc/qtomo.hip to the same gfx950 device code?  (no GPU needed)

Usage: python scripts/isa_identity.py <tree-a> <tree-b> [extra compiler flags]
       (a tree is a checkout of this repository, e.g. `git worktree add /tmp/parent HEAD~1`; a path that ends in .s is
       taken as assembly that is already there: hipcc -S --cuda-device-only)

Compiles quantpy_amd/csrc/qtomo.hip of both trees with the flags of quantpy_amd/build.py plus -S --cuda-device-only,
cuts each assembly file into functions (symbol label .. .Lfunc_end) and kernel descriptors (.amdhsa_kernel ..
.end_amdhsa_kernel), drops comments and the function index of local labels (.LBB12_3 -> .LBBN_3: it moves when
definitions move), and prints the symbols that only one tree has, those whose text differs, and whether the function symbols stand
in the same order (`order: same`, or the first position where the two sequences differ).  Everything else in the
file -- the __hip_cuid_* symbol, the metadata block -- is ignored.  Exit status 1 if either list is non-empty.
It compares text and nothing else: a refactor that is meant to leave every kernel alone is checked by this, not by a
timing."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("qt_build", os.path.join(_HERE, "..", "quantpy_amd", "build.py"))
qt_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(qt_build)

_LOCAL = re.compile(r"\.L(BB|tmp|func_begin|func_end|post_getpc)\d+")
_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_DESC = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")


def start_compile(tree, out, extra):
    """The device-only compile of build_library()'s command line, as a running process (or None for a .s path)."""
    if tree.endswith(".s"):
        return None
    src = os.path.join(tree, "quantpy_amd", "csrc", "qtomo.hip")
    cmd = [qt_build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *qt_build.FLAGS, *extra,
           "-S", "--cuda-device-only", "-o", out, src]
    return subprocess.Popen(cmd)


def functions(path):
    """{symbol: [normalised lines]} of every function, and under 'symbol (descriptor)' of every kernel descriptor."""
    out, name, body, desc = {}, None, [], None
    with open(path) as fh:
        for raw in fh:
            line = _LOCAL.sub(lambda m: ".L" + m.group(1) + "N", raw.split(";", 1)[0].rstrip())
            if not line.strip():
                continue
            if desc is not None:  # (the descriptor of a kernel stands between its last instruction and .Lfunc_end)
                if line.strip() == ".end_amdhsa_kernel":
                    desc = None
                else:
                    out[desc].append(line)
                continue
            d = _DESC.match(line)
            if d:
                desc = d.group(1) + " (descriptor)"
                out[desc] = []
                continue
            m = _LABEL.match(line)
            if m:  # a data symbol never reaches .Lfunc_end: the next label discards it
                name, body = m.group(1), []
            elif name is not None and line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            elif name is not None:
                body.append(line)
    return out


def order_line(fa, fb):
    """The sequence of function symbols of the two files: the same, or the first position where it differs."""
    sa, sb = ([s for s in f if not s.endswith(" (descriptor)")] for f in (fa, fb))
    if sa == sb:
        return "order: same"
    k = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
    return f"order: differs at position {k}: a has {sa[k] if k < len(sa) else None}, b has {sb[k] if k < len(sb) else None}"


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    trees, extra = argv[1:3], argv[3:]
    with tempfile.TemporaryDirectory() as tmp:
        asm = [t if t.endswith(".s") else os.path.join(tmp, "ab"[i] + ".s") for i, t in enumerate(trees)]
        procs = [start_compile(t, a, extra) for t, a in zip(trees, asm)]
        for t, p in zip(trees, procs):
            if p is not None and p.wait() != 0:
                print(f"compile failed: {t}")
                return 2
        fa, fb = (functions(a) for a in asm)
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    differ = sorted(s for s in set(fa) & set(fb) if fa[s] != fb[s])
    print(f"flags: {' '.join(qt_build.FLAGS + extra)}")
    for tag, f in (("a", fa), ("b", fb)):
        kernels = sum(1 for s in f if s.endswith(" (descriptor)"))
        print(f"{tag}: {len(f) - kernels} functions, {kernels} kernel descriptors, {sum(map(len, f.values()))} lines")
    for tag, names in (("only in a", only_a), ("only in b", only_b)):
        print(f"{tag}: {len(names)}")
        for s in names:
            print(f"  {s}")
    print(f"differ: {len(differ)}")
    for s in differ:
        print(f"  {s}: {len(fa[s])} lines in a, {len(fb[s])} in b")
    print(order_line(fa, fb))
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
