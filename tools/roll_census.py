#!/usr/bin/env python3
"""Static instruction census of creff_roll_kernel's five role loops (consumer kh 0 / kh 1, producers KV / Q / AUX) from a hipcc -S listing:
for every depth-2 loop (the iteration loop of a role) the instructions between consecutive s_barrier, by class.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -S --cuda-device-only ar-seg_amd/csrc/creff_roll.hip -o /tmp/creff_roll.s
    python tools/roll_census.py /tmp/creff_roll.s creff_roll_kernelILi1E
"""
import collections
import re
import sys

sys.path.insert(0, __import__("os").path.dirname(__file__))
from isa_census import classify  # noqa: E402


def main():
    lines = open(sys.argv[1]).read().split("\n")
    key = sys.argv[2]
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and ":" in l.split(";")[0])
    end = next(i for i in range(start + 1, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    body = lines[start:end]
    # loop headers at depth 2
    heads = [i for i, l in enumerate(body) if "Inner Loop Header: Depth=2" in l]
    for h in heads:
        # label is on the previous line(s)
        j = h
        while not body[j].startswith(".LBB"):
            j -= 1
        label = body[j].split(":")[0]
        # the loop ends at the last branch back to the label
        last = max(i for i, l in enumerate(body) if re.search(r"s_cbranch\w*\s+" + re.escape(label) + r"\b|s_branch\s+" + re.escape(label) + r"\b", l))
        segs, cur = [], collections.Counter()
        for l in body[j:last + 1]:
            t = l.strip()
            if not t or t.startswith((";", ".")) or t.endswith(":"):
                continue
            op = t.split()[0]
            if op == "s_barrier":
                segs.append(cur)
                cur = collections.Counter()
                continue
            cls, cost = classify(op, t)
            cur[cls] += 1
            cur["_cycles"] += cost
        segs.append(cur)
        print(f"loop {label}: {len(segs) - 1} barriers")
        for k, sg in enumerate(segs):
            valu = sum(v for c, v in sg.items() if c.startswith("valu"))
            print(f"   seg {k}: valu {valu:4d}  mfma {sg['mfma']:3d}  ds_read {sg['ds_read']:3d}  ds_write {sg['ds_write']:3d}  vmem {sg['vmem_load'] + sg['vmem_store']:3d}  "
                  f"salu {sg['salu']:3d}  issue~{sg['_cycles']:.0f}   " + " ".join(f"{c[5:]}={v}" for c, v in sorted(sg.items()) if c.startswith("valu_")))


if __name__ == "__main__":
    main()
