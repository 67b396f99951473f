#!/usr/bin/env python3
"""The p-update p_i = zc·z + β·p of the lane-tested kinds of kS3 (band and mixed items: z comes out of a select): per
kernel, in program order, which product was rounded — r: zc·z rounded, β·p fused into it; f: the other way round.
A site is a v_fma_f64 / v_fmac_f64 with a scalar factor whose addend is a v_mul_f64 with a scalar factor, one of the
two vector factors last written by v_cndmask.  (A register that held a select result earlier can tag a uniform site:
check the listing at the printed line before believing an f.)
usage: tools/ks3_pnext_forms.py FILE.s [-v]   (`hipcc ... --cuda-device-only -S csrc/hip/fused3.hip`)"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks3_static as ic  # noqa: E402


def regs(tok):
    tok = tok.strip().lstrip("-").strip("|")
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return [int(m.group(1))] if m else []


def scalar(tok):
    return bool(re.match(r"-?s\[\d+:\d+\]", tok.strip()))


def sites(lines, a, b):
    tag, mul, seq = {}, {}, []  # vgpr -> "C" after a select; low vgpr of a scalar·vector product -> its vector's tag
    for i in range(a, b):
        s = lines[i].strip()
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        op = parts[0]
        if not (op.startswith("v_") or op.startswith(("global_load", "ds_read", "flat_load"))):
            continue
        ops = [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []
        if not ops:
            continue
        ops[-1] = ops[-1].split()[0] if ops[-1] else ops[-1]
        dst, srcs = regs(ops[0]), ops[1:]
        if op.startswith("v_cndmask"):
            for r in dst:
                tag[r] = "C"
                mul.pop(r, None)
            continue
        if op.startswith("v_mul_f64"):
            vs = [t for t in srcs if regs(t)]
            one = any(scalar(t) for t in srcs) and len(vs) == 1
            c = tag.get(regs(vs[0])[0], "-") if one else None
            for r in dst:
                tag[r] = "-"
                mul.pop(r, None)
            if one and dst:
                mul[dst[0]] = c
            continue
        if op.startswith(("v_fmac_f64", "v_fma_f64")):
            if op.startswith("v_fmac"):
                add, fs = (dst[0] if dst else None), srcs
            else:
                add, fs = (regs(srcs[2])[0] if len(srcs) > 2 and regs(srcs[2]) else None), srcs[:2]
            vs = [t for t in fs if regs(t)]
            if add in mul and any(scalar(t) for t in fs) and len(vs) == 1:
                cm, cf = mul[add], tag.get(regs(vs[0])[0], "-")
                if cm == "C" or cf == "C":
                    seq.append(("r" if cm == "C" else "f", i + 1))
        for r in dst:
            tag[r] = "-"
            mul.pop(r, None)
    return seq


def main():
    lines = open(sys.argv[1]).read().splitlines()
    for name, (a, b) in ic.kernels(lines).items():
        seq = sites(lines, a, b)
        st = "".join(x for x, _ in seq)
        print(name[30:44], len(seq), "sites: r", st.count("r"), "f", st.count("f"),
              [ln for x, ln in seq if x == "f"] if "f" in st else "")
        if "-v" in sys.argv:
            print("  ", st)


if __name__ == "__main__":
    main()
