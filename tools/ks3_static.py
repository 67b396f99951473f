#!/usr/bin/env python3
"""Static instruction counts of one steady row step of kS3 from `hipcc -S` output
(docs/PERFORMANCE.md, rounds 8 and 9: the per-row-step tables).

  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/hip/fused3.hip -o fused3.s
  tools/ks3_static.py fused3.s [kernel-substring ...]

A steady group is a loop body (one label .. backward branch to it) with 42
scheduling barriers (6 steps x (6 stage barriers + 1 step barrier)).  Counted:
the opcodes of steps 1-5 of the group (between the step barriers), per step.
"""
import re
import sys
from collections import Counter


def kernels(lines):
    out, name, start = {}, None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_ZN\S*kS3\S*):", ln)
        if m:
            name, start = m.group(1), i
        if name and re.match(r"^\s*s_endpgm", ln):
            out.setdefault(name, (start, i))
    # extend each kernel to the next kernel's start (several s_endpgm per kernel)
    names = sorted(out, key=lambda k: out[k][0])
    res = {}
    for j, k in enumerate(names):
        end = out[names[j + 1]][0] if j + 1 < len(names) else len(lines)
        res[k] = (out[k][0], end)
    return res


def classify(op):
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
        return "readlane"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def steady_loops(lines, a, b):
    """(label line, branch line) of the innermost loops with 42 scheduling barriers."""
    labels = {}
    cand = []
    for i in range(a, b):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            labels[m.group(1)] = i
        m = re.match(r"^\s*s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in labels:
            la = labels[m.group(1)]
            if sum(1 for x in lines[la:i] if "sched_barrier" in x) == 42:
                cand.append((la, i))
    return [c for c in cand if not any(o != c and o[0] >= c[0] and o[1] <= c[1] for o in cand)]


def count_steps(lines, la, lb):
    chunks, cur = [], Counter()
    fine = Counter()
    for ln in lines[la:lb]:
        if "sched_barrier" in ln:
            chunks.append((cur, fine))
            cur, fine = Counter(), Counter()
            continue
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        cur[classify(op)] += 1
        fine[op] += 1
    # chunks 0..41: step j = chunks 7j .. 7j+6 ; steps 1-5
    tot, ftot = Counter(), Counter()
    for ch, f in chunks[7:42]:
        tot.update(ch)
        ftot.update(f)
    return {k: v / 5.0 for k, v in tot.items()}, {k: v / 5.0 for k, v in ftot.items()}


def main():
    lines = open(sys.argv[1]).read().splitlines()
    want = sys.argv[2:]
    for name, (a, b) in kernels(lines).items():
        if want and not any(w in name for w in want):
            continue
        for la, lb in steady_loops(lines, a, b):
            c, f = count_steps(lines, la, lb)
            allc = sum(c.values())
            dpp = sum(v for k, v in f.items() if "dpp" in k)
            f64 = {k: v for k, v in f.items() if k in ("v_add_f64", "v_mul_f64", "v_fma_f64")}
            print(f"{name} loop@{la + 1}: all {allc:.1f} VALU {c.get('VALU', 0):.1f} SALU {c.get('SALU', 0):.1f} "
                  f"VMEM {c.get('VMEM', 0):.1f} readlane {c.get('readlane', 0):.1f} s_nop {c.get('s_nop', 0):.1f} "
                  f"s_waitcnt {c.get('s_waitcnt', 0):.1f} LDS {c.get('LDS', 0):.1f} | dpp {dpp:.1f} "
                  + " ".join(f"{k} {v:.1f}" for k, v in sorted(f64.items())))


if __name__ == "__main__":
    main()
