#!/usr/bin/env python3
"""Which product became the fma addend: per kS3 kernel, the sequence of (tag of the v_mul's vector source, tag of the
following v_fmac's vector source) for every v_mul_f64 whose result a v_fmac_f64 accumulates into.
Tags: L = derived from a DPP move through v_add only (a lateral difference), M = the direct result of a v_mul,
- = anything else.  fused3.hip compiles with fast contraction, and which of two products is rounded decides the last
bit: two builds whose sequences agree contract alike (docs/PERFORMANCE.md, round 9).
usage: tools/ks3_fma_forms.py A.s [B.s]  (`hipcc ... --cuda-device-only -S` outputs; two files: compare per kernel)"""
import re
import sys

import os

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks3_static as ic  # noqa: E402


def regs(tok):
    tok = tok.strip().lstrip("-").strip("|")
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return [int(m.group(1))] if m else []


def forms(lines, a, b):
    tag = {}       # vgpr -> tag
    pend = {}      # dest low vgpr -> tag of the mul's vector source
    out = []
    for ln in lines[a:b]:
        s = ln.strip()
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        op = parts[0]
        if not op.startswith("v_") and not op.startswith(("global_load", "ds_read", "flat_load")):
            continue
        ops = [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []
        # strip trailing modifiers from last operand
        if ops:
            ops[-1] = ops[-1].split()[0]
        if not ops:
            continue
        dst = regs(ops[0])
        srcs = ops[1:]
        vt = [tag.get(r, "-") for t in srcs for r in regs(t)[:1]]
        if "dpp" in op:
            for r in dst:
                tag[r] = "L"
            continue
        if op == "v_add_f64":
            t = "L" if "L" in vt else "-"
            for r in dst:
                tag[r] = t
            pend.pop(dst[0], None) if dst else None
            continue
        if op == "v_mul_f64":
            vs = [t for t in srcs if regs(t)]
            st = tag.get(regs(vs[0])[0], "-") if len(vs) == 1 else "vv"
            for r in dst:
                tag[r] = "M"
            if dst:
                pend[dst[0]] = st
            continue
        if op.startswith("v_fmac_f64"):
            vs = [t for t in srcs if regs(t)]
            if dst and dst[0] in pend and len(vs) == 1:
                out.append(pend.pop(dst[0]) + tag.get(regs(vs[0])[0], "-"))
            for r in dst:
                tag[r] = "-"
            continue
        for r in dst:
            tag[r] = "-"
            pend.pop(r, None)
    return out


def per_kernel(path):
    lines = open(path).read().splitlines()
    return {k[30:44]: forms(lines, a, b) for k, (a, b) in ic.kernels(lines).items()}


A = per_kernel(sys.argv[1])
if len(sys.argv) == 2:
    for k, f in A.items():
        print(k, len(f), {x: f.count(x) for x in sorted(set(f))})
else:
    B = per_kernel(sys.argv[2])
    for k in A:
        fa, fb = A[k], B.get(k, [])
        ca = {x: fa.count(x) for x in sorted(set(fa))}
        cb = {x: fb.count(x) for x in sorted(set(fb))}
        print(k, "same order" if fa == fb else "DIFFERENT", len(fa), len(fb), ca, cb if ca != cb else "")
