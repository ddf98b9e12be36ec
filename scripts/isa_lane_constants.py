#!/usr/bin/env python3
"""The front and the first evaluation of the n = 3 specialised MLE kernels in the gfx950 assembly of csrc/qtomo.hip of two
trees: what stands in the shadow of the counts' loads, and what the integer front of load_freq, the dropped second store
of the Bloch element and the ballots for the first gradient norm took out.  A sibling of scripts/isa_front.py; no GPU
needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 <flags of quantpy_amd/build.py> -S --cuda-device-only -o parent.s ...
    python scripts/isa_lane_constants.py parent.s tree.s > profiles/lane_constants_isa.txt

Per kernel and assembly, instruction counts by the classes of scripts/isa_path_count.py in four stretches, each found
by anchors in assembly order (a branch inside a stretch is counted with both of its sides):
  shadow      from the s_barrier of make_ctx to the first s_waitcnt vmcnt behind it (the first wait a counts load needs)
  front       from that barrier to the first ds_write_b128 behind the wait: the step, load_freq and lin_invert (the
              start-point code behind them is the first to write a 16-byte matrix element)
  evaluation  the first evaluation of a trial: from the last ds_write_b128 in front of its stage n (the matrix bloch_of
              reads) to the first global store behind it (the result)
  stage n     inside it: from the last ds_write_b64 in front of the four reciprocals of stage_n_log<.., DEFER> (the end
              of forward stage 2) to the last ds_write_b64 behind them (rb[])
The first evaluation is recognised by its stage n: the first four v_rcp_f64 behind the front that stand within 160
instructions of each other with no v_log / second group between them (a deferred evaluation takes no logarithm).

On the first evaluation, two conditions (checked for the kernels named in CHECKED, reported for the others) and one
figure:
  entry reads   ds_read_b32 whose destination is taken apart as a stage-n entry (v_bfe_u32 .., 8, 8 within 30
                instructions) inside the evaluation: reported only -- the row descriptors that would remove them were
                measured slower on the headline and are not built
  bloch store   ds_read_b64 vX .. ds_write_b64 .., vX within 8 instructions in front of stage n (bloch_of's read-back
                stored again): none
  v_max_f64     on an operand that a DPP move has just delivered (the gmax butterfly), between the evaluation's stage n
                and its first global store: none
Exit status 1 if a checked kernel of the second assembly misses one."""
import collections
import re
import sys

from isa_path_count import classify, kernel_lines

KERNELS = ["k_mle_fused_hw<3, false>", "k_mle_fused<3, false>", "k_mle_start<3, false>"]
CHECKED = KERNELS
SHOWN = ["valu_f64", "valu_other", "valu_dpp", "salu", "waitcnt", "lds", "vmem"]


def instructions(body):
    out = []
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith((".", "//")):
            continue
        out.append(t)
    return out


def op(t):
    return t.split()[0]


def stretches(ins):
    """{name: (first, last + 1)} by the anchors of the module docstring."""
    bar = next(i for i, t in enumerate(ins) if op(t) == "s_barrier")
    wait = next(i for i in range(bar, len(ins)) if op(ins[i]) == "s_waitcnt" and "vmcnt" in ins[i])
    front_end = next(i for i in range(wait, len(ins)) if op(ins[i]) == "ds_write_b128")
    rcp = [i for i in range(front_end, len(ins)) if op(ins[i]) == "v_rcp_f64_e32" or op(ins[i]) == "v_rcp_f64"]
    group = None
    for k in range(len(rcp) - 3):
        g = rcp[k:k + 4]
        alone = (k == 0 or g[0] - rcp[k - 1] > 160) and (k + 4 == len(rcp) or rcp[k + 4] - g[3] > 40)
        if g[3] - g[0] <= 160 and alone:
            group = g
            break
    if group is None:
        raise SystemExit("no deferred stage n found")
    n0 = max(i for i in range(group[0]) if op(ins[i]) == "ds_write_b64")
    n1 = max(i for i in range(group[3], group[3] + 60) if op(ins[i]) == "ds_write_b64") + 1
    e0 = max(i for i in range(n0) if op(ins[i]) == "ds_write_b128")
    e1 = next(i for i in range(n1, len(ins)) if op(ins[i]).startswith("global_store")) + 1
    return collections.OrderedDict(shadow=(bar + 1, wait), front=(bar + 1, front_end), evaluation=(e0, e1),
                                   stage_n=(n0 + 1, n1))


def counts(ins, lo, hi):
    c = collections.Counter()
    for t in ins[lo:hi]:
        c[classify(op(t), t, set())] += 1
    return c


def entry_reads(ins, lo, hi):
    n = 0
    for i in range(lo, hi):
        if op(ins[i]) != "ds_read_b32":
            continue
        dst = ins[i].split()[1].rstrip(",")
        pat = re.compile(r"v_bfe_u32 \S+ " + re.escape(dst) + r", 8, 8")
        n += any(pat.search(t) for t in ins[i + 1:i + 31])
    return n


def bloch_stores(ins, lo, hi):
    n = 0
    for i in range(lo, hi):
        if op(ins[i]) != "ds_read_b64":
            continue
        dst = ins[i].split()[1].rstrip(",")
        n += any(op(t) == "ds_write_b64" and t.split(",", 1)[1].strip().split()[0] == dst for t in ins[i + 1:i + 9])
    return n


def report(path, kernel):
    with open(path) as fh:
        name, dem, body = kernel_lines(fh.read().split("\n"), kernel)
    ins = instructions(body)
    st = stretches(ins)
    rows = [(k, hi - lo, counts(ins, lo, hi)) for k, (lo, hi) in st.items()]
    (e0, e1), (n0, n1) = st["evaluation"], st["stage_n"]
    cond = dict(entry_reads=entry_reads(ins, e0, e1), bloch_store=bloch_stores(ins, e0, n0),
                v_max_f64=sum(op(ins[i]).startswith("v_max_f64") and any(op(t) == "v_mov_b32_dpp" for t in ins[i - 2:i])
                              for i in range(n1, e1)))
    return len(ins), rows, cond


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    bad = False
    for kernel in KERNELS:
        print(kernel)
        print(f"  {'':8s} {'stretch':11s} {'total':>6s}  " + " ".join(f"{k[:7]:>7s}" for k in SHOWN))
        conds = []
        for tag, path in zip(("parent", "tree"), sys.argv[1:3]):
            total, rows, cond = report(path, kernel)
            for name, n, c in rows:
                print(f"  {tag:8s} {name:11s} {n:6d}  " + " ".join(f"{c.get(k, 0):7d}" for k in SHOWN))
            print(f"  {tag:8s} {'kernel':11s} {total:6d}")
            conds.append(cond)
        for k in conds[0]:
            verdict = "" if kernel not in CHECKED or k == "entry_reads" else ("  ok" if conds[1][k] == 0 else "  MISSED")
            bad |= verdict.endswith("MISSED")
            print(f"  first evaluation, {k:11s}: parent {conds[0][k]}, tree {conds[1][k]}{verdict}")
        print()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
