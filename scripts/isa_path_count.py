#!/usr/bin/env python3
"""Static instruction counts of one kernel in the gfx950 assembly of csrc/qtomo.hip, by class: for the whole kernel, per
basic block, and summed over a named list of blocks (the straight-line path one is working on).  No GPU needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-sched-strategy=max-ilp -S --cuda-device-only \\
          -o /tmp/qtomo.s quantpy_amd/csrc/qtomo.hip
    python scripts/isa_path_count.py /tmp/qtomo.s 'k_mle_start<3, false>' [--blocks] [--sum .LBB70_3,.LBB70_7,entry]

The kernel is named by a substring of its mangled or of its demangled name (c++filt).  The classes are those of
scripts/isa_mix.py, by generic mnemonic prefix, plus "spill_restore": a lane read of a register that the same kernel
fills lane by lane (how the compiler parks scalar registers in a vector register) -- it is taken out of valu_other.
A block is named by its label; the instructions in front of the first label are the block "entry"."""
import argparse
import collections
import re
import subprocess

CLASSES = ["valu_f64", "valu_other", "valu_dpp", "spill_restore", "salu", "waitcnt", "lds", "vmem", "scratch", "mfma",
           "accvgpr", "other"]


def classify(op, text, spill_regs):
    if op.startswith("v_readlane") and text.split(",")[1].strip() in spill_regs:
        return "spill_restore"
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("v_accvgpr"):
        return "accvgpr"
    if op.startswith("v_") and "f64" in op:
        return "valu_f64"
    if op.endswith("_dpp") or "dpp" in text:
        return "valu_dpp"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_"):
        return "salu"
    return "other"


def kernel_lines(lines, pat):
    """(mangled name, the lines of its body)"""
    heads = [(i, m.group(1)) for i, ln in enumerate(lines) if (m := re.match(r"^(_Z\w+):", ln))]
    names = [n for _, n in heads]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    for (i, name), d in zip(heads, dem):
        if pat in name or pat in d:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            return name, d, lines[i + 1:end]
    raise SystemExit(f"no kernel matches {pat!r}")


def count(body):
    insts, block = [], "entry"  # (block, op, text)
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.startswith((".", "//")) and not t.endswith(":"):
            continue
        if t.endswith(":"):
            block = t[:-1]
            continue
        insts.append((block, t.split()[0], t))
    spill_regs = {t.split()[1].rstrip(",") for _, op, t in insts if op.startswith("v_writelane")}
    per = collections.OrderedDict()
    for block, op, t in insts:
        per.setdefault(block, collections.Counter())[classify(op, t, spill_regs)] += 1
    return per


def row(name, c):
    return f"{name:16s} {sum(c.values()):6d}  " + " ".join(f"{c.get(k, 0):6d}" for k in CLASSES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--blocks", action="store_true", help="one line per basic block")
    ap.add_argument("--sum", default="", help="comma-separated block labels: one line with their total")
    a = ap.parse_args()
    with open(a.asm) as fh:
        name, dem, body = kernel_lines(fh.read().split("\n"), a.kernel)
    per = count(body)
    print(re.sub(r"\(.*", "", dem))
    print(f"{'block':16s} {'total':>6s}  " + " ".join(f"{k[:6]:>6s}" for k in CLASSES))
    if a.blocks:
        for b, c in per.items():
            print(row(b, c))
    if a.sum:
        want = [b for b in a.sum.split(",") if b]
        missing = [b for b in want if b not in per]
        if missing:
            raise SystemExit(f"no such block: {missing}")
        print(row("sum(named)", sum((per[b] for b in want), collections.Counter())))
    print(row("kernel", sum(per.values(), collections.Counter())))


if __name__ == "__main__":
    main()
