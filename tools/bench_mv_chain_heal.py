#!/usr/bin/env python3
"""What healing the flagged pixels of a chain costs per frame, next to the chain step it follows and to the keyframe anchor it resembles.  One
process, forms alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max: the protocol of
tools/bench_block_motion_anchor.py.

Content: scene 1 of tests/mv_chain_heal_oracle.py scaled up -- NV12 frames cut from one noise canvas, panned by (3, -2) per frame, +-2 of noise
on every sample of the current frame.  The state healed is frame 6 of a GOP: merged = 4 * 6 * (3, -2) and link = 0x60 on unflagged pixels; a
share of the blocks of the grid (0 %, about 5 %, 100 %) is flagged whole, link = 0x61, merged = 4 * 5 * (3, -2): the zero motion the chain
substitutes for an intra block, one frame behind.  Cases: 720x960 and 1024x2048, blocks of 16 and of 8, r = 1, 2, 3.  Forms per case:
  heal/<share>/<r>          arseg_mv_chain_heal_fwd with intra = 0: on noisy content no block is accepted, so merged and link stay as they are
                            and every call does the same work -- the whole of decide, and apply reading the decisions
  restore                   copying merged and link back from pristine copies (what the next form needs before every call)
  restore+heal/<share>/<r>  the copies, then the entry with intra = 20: accepted blocks are rewritten by apply
  read_link                 torch.count_nonzero over the link plane: one byte per pixel read -- a yardstick, not the code under test
  push                      MotionChain.push of grid records for frame 6 (the step the heal follows) -- a yardstick
  anchor/<r>                arseg_block_motion_anchor_fwd at the same (B, r) on the same planes -- a yardstick
Every form with "/graph" is the same call captured once in a HIP graph and replayed: the device's time without the host's enqueue time.
One JSON line on stdout, the same written to --out (default profiles/mv_chain_heal.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from arseg_amd import _lib, ingest, ops
from bench_block_motion_pyr import graphed
from bench_mv_brecords import alternate

PAN, AT, GOP = (3, -2), 6, 12
LAM, INTRA = 2, 20
SHARES = (("0", 0.0), ("5", 0.05), ("100", 1.0))


def planes(H, W, dev):
    g = np.random.Generator(np.random.PCG64(13))
    m = 3 * AT + 4
    cv = g.integers(0, 256, (H + 2 * m, W + 2 * m), dtype=np.uint8)
    key = cv[m:m + H, m:m + W]
    cur = cv[m + PAN[1] * AT:m + PAN[1] * AT + H, m + PAN[0] * AT:m + PAN[0] * AT + W]
    cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in (cur, key))


def state(H, W, B, share, dev):
    """(merged_f, link_f, blocks flagged) with ``share`` of the grid's blocks flagged whole."""
    g = np.random.Generator(np.random.PCG64(17))
    by, bx = -(-H // B), -(-W // B)
    pick = g.random((by, bx)) < share
    fl = np.repeat(np.repeat(pick, B, axis=0), B, axis=1)[:H, :W]
    merged = np.empty((H, W, 2), dtype=np.int16)
    merged[...] = (4 * AT * PAN[0], 4 * AT * PAN[1])
    merged[fl] = (4 * (AT - 1) * PAN[0], 4 * (AT - 1) * PAN[1])
    link = np.where(fl, 0x61, 0x60).astype(np.uint8)
    return torch.from_numpy(merged).to(dev), torch.from_numpy(link).to(dev), int(pick.sum())


def grid_records(H, W, B, dev):
    by, bx = -(-H // B), -(-W // B)
    r = np.zeros((by, bx, 8), dtype=np.int16)
    r[..., 0], r[..., 1] = (np.arange(bx) * B)[None, :], (np.arange(by) * B)[:, None]
    r[..., 2], r[..., 3] = np.minimum(B, W - r[..., 0]), np.minimum(B, H - r[..., 1])
    r[..., 4], r[..., 5] = 4 * PAN[0], 4 * PAN[1]
    return torch.from_numpy(r.reshape(-1, 8)).to(dev)


def case_cost(H, W, B, radii, shares, kept_only, repeats, window, dev):
    cur, key = planes(H, W, dev)
    n = -(-H // B) * -(-W // B)
    rec = grid_records(H, W, B, dev)
    chain = ingest.MotionChain(H, W, gop=GOP, max_ref=16, device=dev, track_links=True)
    for _ in range(AT - 1):
        chain.push(rec)

    def push():
        chain.f = chain.last = AT - 1
        return chain.push(rec)

    forms, info, keep = {"push": push}, {}, []
    forms["push/graph"] = graphed(push)
    states = {name: state(H, W, B, share, dev) for name, share in SHARES if name in shares}
    link0 = next(iter(states.values()))[1]
    forms["read_link"] = lambda: torch.count_nonzero(link0)
    forms["read_link/graph"] = graphed(forms["read_link"])
    for r in radii:
        out, st = torch.zeros((n, 8), dtype=torch.int16, device=dev), torch.zeros(_lib.BMA_NSTATS, dtype=torch.int64, device=dev)
        keep.append((out, st))
        forms[f"anchor/{r}"] = lambda r=r, out=out, st=st: ops.block_motion_anchor(cur, key, rec, chain.merged[AT - 1], AT, B, r, LAM, INTRA, out=out, sad=False, stats=st)
        forms[f"anchor/{r}/graph"] = graphed(forms[f"anchor/{r}"])
    for name in states:
        merged0, link0s, flagged_blocks = states[name]
        merged, link = merged0.clone(), link0s.clone()
        dec, st, row = torch.zeros((n, 8), dtype=torch.int16, device=dev), torch.zeros(_lib.HEAL_NSTATS, dtype=torch.int64, device=dev), torch.zeros(
            _lib.LINK_NSTATS, dtype=torch.int64, device=dev)
        keep.append((merged0, link0s, merged, link, dec, st, row))

        def restore(merged=merged, link=link, merged0=merged0, link0s=link0s):
            merged.copy_(merged0)
            link.copy_(link0s)

        if name == "100" and not kept_only:
            forms["restore"] = restore
            forms["restore/graph"] = graphed(restore)
        for r in radii:
            heal = lambda intra, r=r, merged=merged, link=link, dec=dec, st=st, row=row: ops.mv_chain_heal(
                cur, key, merged, link, B, r, LAM, intra, decisions=dec, sad=False, stats=st, link_stats_row=row)
            restore()
            st.zero_()
            heal(INTRA)
            healed = st.tolist()
            restore()
            st.zero_()
            heal(0)
            kept = st.tolist()
            assert torch.equal(merged, merged0) and torch.equal(link, link0s), "intra = 0 on noisy content must leave the state as it was"
            info[f"{name}/{r}"] = {"blocks": n, "blocks_flagged": flagged_blocks, "stats_intra_20": healed, "stats_intra_0": kept}
            forms[f"heal/{name}/{r}"] = lambda heal=heal: heal(0)
            forms[f"heal/{name}/{r}/graph"] = graphed(forms[f"heal/{name}/{r}"])
            if name != "0" and not kept_only:
                both = lambda heal=heal, restore=restore: (restore(), heal(INTRA))
                forms[f"restore+heal/{name}/{r}"] = both
                forms[f"restore+heal/{name}/{r}/graph"] = graphed(both)
    res = alternate(forms, repeats, window)
    res = {k: {key_.replace("per_gop", "per_frame"): v for key_, v in r.items()} for k, r in res.items()}
    print(f"{H}x{W} B {B}: " + ", ".join(f"{k} {r['us_per_frame_median']:.1f} us ({r['us_per_frame_min']:.1f}-{r['us_per_frame_max']:.1f})" for k, r in res.items()),
          file=sys.stderr)
    return {"frame": [H, W], "block": B, "blocks": n, "states": info, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--cases", default="720x960,1024x2048", help="HxW, each at blocks of 16 and of 8")
    ap.add_argument("--blocks", default="16,8")
    ap.add_argument("--radii", default="1,2,3")
    ap.add_argument("--shares", default="0,5,100", help="the shares of flagged blocks to time, of 0, 5 and 100 (per cent)")
    ap.add_argument("--kept-only", action="store_true", help="leave the restore and restore+heal forms out (for a kernel trace of one state)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mv_chain_heal.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_chain_heal.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    radii = [int(v) for v in a.radii.split(",")]
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "pan": list(PAN), "frame_healed": AT, "lam": LAM,
           "intra_of_restore+heal": INTRA, "cases": []}
    for c in a.cases.split(","):
        H, W = (int(v) for v in c.lower().split("x"))
        for B in (int(v) for v in a.blocks.split(",")):
            res["cases"].append(case_cost(H, W, B, radii, a.shares.split(","), a.kept_only, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
