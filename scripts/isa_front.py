#!/usr/bin/env python3
"""The front of a kernel in the gfx950 assembly of csrc/qtomo.hip: how far the entry is from the last load of the
prologue's batch, and what stands in between.  No GPU needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 <flags of quantpy_amd/build.py> -S --cuda-device-only \\
          -o /tmp/qtomo.s quantpy_amd/csrc/qtomo.hip
    python scripts/isa_front.py /tmp/qtomo.s 'k_mle_fused_hw<3, false>' ['k_mle_bfgs<3, false>:2' ...]

Per kernel (named as for scripts/isa_path_count.py; `:N` = the prologue ends at the N-th s_barrier, default 1 --
k_mle_bfgs votes at a barrier of its own first):
  preload      .amdhsa_user_sgpr_kernarg_preload_length of its descriptor (dwords of arguments in SGPRs at wave launch)
  to last load instructions in assembly order from the entry to the last global_load in front of that barrier, the load
               included.  With preloading the kernel starts with a compatibility prologue for firmware that does not
               preload (s_load of the same arguments, a wait, a branch, padding to 256 bytes); it is not counted.
  kernarg waits  s_waitcnt lgkmcnt(0) in that stretch with an s_load outstanding
  s_load         scalar loads issued in that stretch
  loads          global_load instructions in that stretch, and the vmcnt of the first s_waitcnt vmcnt behind them
The count is in assembly order: a branch in the stretch is counted with both of its sides."""
import re
import sys

from isa_path_count import kernel_lines


def instructions(body):
    out = []
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith((".", "//")):
            continue
        out.append(t)
    return out


def front(text, lines, spec):
    pat, _, nb = spec.partition(":")
    nb = int(nb) if nb else 1
    name, dem, body = kernel_lines(lines, pat)
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
    pm = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", m.group(1)) if m else None
    preload = int(pm.group(1)) if pm else 0
    ins = instructions(body)
    start = 0
    if preload:  # the compatibility prologue ends with its padding: the code proper starts behind the last s_nop of the run
        k = next(i for i, t in enumerate(ins) if t.startswith("s_branch"))
        start = k + 1
        while ins[start].startswith(("s_nop", "s_code_end")):
            start += 1
    seen, end = 0, len(ins)
    for i in range(start, len(ins)):
        if ins[i].startswith("s_barrier"):
            seen += 1
            if seen == nb:
                end = i
                break
    loads = [i for i in range(start, end) if ins[i].startswith("global_load")]
    last = loads[-1]
    pending, waits, sloads = 0, 0, 0
    for t in ins[start:last + 1]:
        if t.startswith("s_load"):
            pending += 1
            sloads += 1
        elif t.startswith("s_waitcnt") and "lgkmcnt(0)" in t:
            waits += 1 if pending else 0
            pending = 0
    vm = next((re.search(r"vmcnt\((\d+)\)", t).group(1) for t in ins[last + 1:] if t.startswith("s_waitcnt") and "vmcnt" in t), "-")
    short = re.sub(r"\(.*", "", dem).replace("void qt::", "")
    return f"{short:34s} {preload:7d} {last + 1 - start:12d} {waits:13d} {sloads:6d} {len(loads):5d}   vmcnt({vm})"


def main():
    with open(sys.argv[1]) as fh:
        text = fh.read()
    lines = text.split("\n")
    print(f"{'kernel':34s} {'preload':>7s} {'to last load':>12s} {'kernarg waits':>13s} {'s_load':>6s} {'loads':>5s}   first wait behind")
    for spec in sys.argv[2:]:
        print(front(text, lines, spec))


if __name__ == "__main__":
    main()
