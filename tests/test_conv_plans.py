"""The conv launch plans, host side (CPU only: nothing here launches).

The library states what each arseg_conv_desc.tile_cfg is once, in csrc/conv_plans.h; this module is the second, independent statement of the
numbering (TABLE32 / TABLE16, written from the tile_cfg comments of include/arseg_hip.h) and holds the pure queries and the tuners' candidate
sequences to a record of what they answered before the table existed (golden/conv_plans_record.json).

``python tests/test_conv_plans.py`` writes that record from the tree it runs in; it holds recorded results only.  The committed record was
written that way in a checkout of commit 2e0af0d, the last one before the table.  There the three candidate generators of ops/conv.py were
closures inside ``_conv2d16``, ``_conv2d16_up2`` and ``_conv_wino``; for the recording their bodies were copied, unchanged, into module-level
functions of the names used below (nothing else in that checkout was touched), and running this module's ``__main__`` on the present tree
reproduces the file byte for byte.  The query grid is every
tile_cfg from -1 to one past the fp32 engine's last id x the three maths x upsample2x 0 / 1 x split_k 0 / 1 / 2 / 4 on the descriptors of
DESCS; per point the status of arseg_conv_out_hw and the bytes of arseg_conv2d_workspace_bytes and arseg_conv2d16_workspace_bytes, per
(descriptor, math, upsample2x) the bytes of arseg_conv2d_find_workspace_bytes, per descriptor the output size."""
import ctypes
import functools
import itertools
import json
import os
import sys

import pytest

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans_record.json")
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
F32, F16X3, F16 = 0, 1, 2
ENGINE32, ENGINE16 = 0, 1
NONE, AUTO, TILE, TILE_WIDE, PATCH, STEM, UP2_C64 = range(7)

# id -> (kind, bm, bn, bk, nbuf); 0 = chosen per shape.  From the tile_cfg comment of struct arseg_conv_desc.
TABLE32 = {0: (AUTO, 0, 0, 32, 1),
           1: (TILE, 128, 128, 32, 2), 2: (TILE, 128, 64, 32, 2), 3: (TILE, 64, 64, 32, 2), 4: (TILE, 64, 128, 32, 2),
           5: (TILE, 128, 128, 32, 1), 6: (TILE, 128, 64, 32, 1), 7: (TILE, 64, 64, 32, 1), 8: (TILE, 64, 128, 32, 1),
           9: (TILE, 128, 128, 64, 1), 10: (TILE, 128, 64, 64, 1), 11: (TILE, 64, 64, 64, 1), 12: (TILE, 64, 128, 64, 1),
           13: (PATCH, 128, 64, 32, 2), 14: (PATCH, 128, 128, 32, 2), 15: (PATCH, 256, 64, 32, 2), 16: (PATCH, 256, 128, 32, 2),
           17: (TILE_WIDE, 256, 128, 32, 1), 18: (TILE_WIDE, 128, 256, 32, 1), 19: (TILE_WIDE, 256, 256, 32, 1),
           20: (PATCH, 256, 64, 32, 2), 21: (PATCH, 256, 64, 32, 2), 22: (PATCH, 128, 64, 32, 2),
           23: (UP2_C64, 128, 64, 32, 2)}
# From the arseg_conv2d16_fwd comment: bn = channel tile, bk = K step in halves, bm = pixel tile (128 for the GEMM tiles).
TABLE16 = {0: (AUTO, 128, 0, 0, 2),
           1: (TILE, 128, 64, 32, 2), 2: (TILE, 128, 128, 32, 2), 3: (TILE, 128, 64, 64, 2), 4: (TILE, 128, 128, 64, 2),
           5: (PATCH, 128, 64, 64, 2), 6: (PATCH, 128, 128, 64, 2), 7: (PATCH, 256, 64, 64, 2), 8: (PATCH, 256, 128, 64, 2),
           9: (STEM, 256, 64, 16, 1),
           10: (PATCH, 256, 64, 64, 2), 11: (PATCH, 256, 64, 64, 2), 12: (PATCH, 256, 128, 64, 2), 13: (PATCH, 128, 64, 64, 2)}
FUSES32, FUSES16 = (13, 14, 15, 16, 20, 21, 22, 23), (5, 6, 7, 8, 10, 11, 12, 13)          # the plans that apply upsample2x themselves
NO_SPLIT32, NO_SPLIT16 = FUSES32, (5, 6, 7, 8, 9, 10, 11, 12, 13)                           # ... and those without split-K
FORCED_TW32, FORCED_TW16 = {20: 32, 21: 16, 22: 16}, {10: 32, 11: 16, 12: 32, 13: 16}      # the squarer pixel tiles

#        N, H,  W,   Cin, Cout, k, stride, pad, dil, batch
DESCS = {
    "c64_w16": (1, 12, 16, 64, 64, 3, 1, 1, 1, 0), "c64_w24": (1, 12, 24, 64, 64, 3, 1, 1, 1, 0), "c64_w40": (1, 12, 40, 64, 64, 3, 1, 1, 1, 0),
    "c64_w50": (1, 12, 50, 64, 64, 3, 1, 1, 1, 0), "c64_w100": (2, 12, 100, 64, 64, 3, 1, 1, 1, 0),
    "c128_w24": (1, 12, 24, 64, 128, 3, 1, 1, 1, 0), "c128_w100": (2, 12, 100, 64, 128, 3, 1, 1, 1, 0),
    "dil2_w40": (1, 12, 40, 64, 64, 3, 1, 2, 2, 0), "dil2_w50": (1, 12, 50, 64, 128, 3, 1, 2, 2, 0),
    "odd_h": (1, 13, 50, 64, 64, 3, 1, 1, 1, 0),
    "1x1_96_19": (1, 12, 50, 96, 19, 1, 1, 0, 1, 0),
    "stem": (1, 20, 40, 8, 64, 7, 2, 3, 1, 0), "stem_cin4": (1, 20, 40, 4, 64, 7, 2, 3, 1, 0),
    "deep_8x8": (1, 8, 8, 512, 512, 3, 1, 1, 1, 0),           # automatic split-K
    "m64": (1, 4, 16, 64, 128, 1, 1, 0, 1, 0),                # M <= 64: no 128-pixel tile in the automatic plan
    "batch36": (1, 40, 1, 64, 128, 1, 1, 0, 1, 36),           # the Winograd route's batched GEMM
}
CFGS, MATHS, UPS, SPLITS = range(-1, 25), (F32, F16X3, F16), (0, 1), (0, 1, 2, 4)
CAND_GRID = {"conv": [(mth, kt, co, m, p) for mth in (F32, F16X3) for kt in (2, 18, 36, 144) for co in (19, 64, 128, 256) for m in (64, 4096)
                      for p in (False, True)],
             "conv16": [(kt, co) for kt in (1, 4, 9, 72) for co in (19, 64, 128)],
             "conv16_up2": [(co,) for co in (32, 64, 128)],
             "wino_gemm": [(mth, co) for mth in MATHS for co in (32, 64, 128, 256)]}


def lib():
    from arseg_amd import _lib

    return _lib.load()


def desc(name, tile_cfg=0, math=F32, up2=0, split_k=0):
    from arseg_amd import _lib

    N, H, W, Cin, Cout, k, stride, pad, dil, batch = DESCS[name]
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.in_ld, d.Cout, d.out_ld, d.res_ld = N, H, W, Cin, Cin, Cout, (Cout + 7) // 8 * 8, (Cout + 7) // 8 * 8
    d.R, d.S, d.stride, d.pad, d.dil = k, k, stride, pad, dil
    d.tile_cfg, d.math, d.upsample2x, d.split_k = tile_cfg, math, up2, split_k
    if batch:
        d.batch, d.in_batch_stride, d.w_batch_stride, d.out_batch_stride = batch, N * H * W * Cin, Cout * Cin, N * H * W * Cout
    return d


def points():
    return itertools.product(MATHS, UPS, CFGS, SPLITS)


def old_queries(name):
    """{"hw": [Ho, Wo] of the accepted points (one size) or None, "find": [bytes per (math, up2)], "rows": [[status, ws32, ws16] per point]}"""
    L = lib()
    rows, sizes, find = [], set(), []
    for mth, up2, cfg, sk in points():
        d, ho, wo = desc(name, cfg, mth, up2, sk), ctypes.c_int(-1), ctypes.c_int(-1)
        st = L.arseg_conv_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo))
        if st == OK:
            sizes.add((ho.value, wo.value))
        rows.append([st, L.arseg_conv2d_workspace_bytes(ctypes.byref(d)), L.arseg_conv2d16_workspace_bytes(ctypes.byref(d))])
    for mth, up2 in itertools.product(MATHS, UPS):
        find.append(L.arseg_conv2d_find_workspace_bytes(ctypes.byref(desc(name, 0, mth, up2))))
    assert len(sizes) <= 1, sizes
    return {"hw": list(sizes.pop()) if sizes else None, "find": find, "rows": rows}


def candidate_sequences():
    from arseg_amd import ops
    from arseg_amd.ops import _plans, conv

    out = {"conv": [], "conv16": [list(map(list, conv._conv16_candidates(*a))) for a in CAND_GRID["conv16"]],
           "conv16_up2": [list(map(list, conv._conv16_up2_candidates(*a))) for a in CAND_GRID["conv16_up2"]],
           "wino_gemm": [list(conv._wino_gemm_candidates(*a)) for a in CAND_GRID["wino_gemm"]]}
    prev = ops.set_conv_math("f32")
    try:
        for mth, kt, co, m, p in CAND_GRID["conv"]:
            ops.set_conv_math({F32: "f32", F16X3: "f16x3"}[mth])
            out["conv"].append(list(map(list, _plans._conv_candidates(kt, co, m, p))))
    finally:
        ops.set_conv_math(prev)
    return out


@functools.lru_cache(maxsize=None)
def record():
    with open(RECORD) as f:
        return json.load(f)


def query(engine, d):
    from arseg_amd import _lib

    info = _lib.ConvPlanInfo()
    return lib().arseg_conv_plan_query(engine, ctypes.byref(d), ctypes.byref(info)), info


@pytest.mark.parametrize("name", list(DESCS))
def test_old_queries_answer_as_recorded(name):
    got, want = old_queries(name), record()["queries"][name]
    assert got["hw"] == want["hw"] and got["find"] == want["find"]
    bad = [(p, g, w) for p, g, w in zip(points(), got["rows"], want["rows"]) if g != w]
    assert not bad and len(got["rows"]) == len(want["rows"]), bad[:5]


def test_candidate_sequences_are_as_recorded():
    got, want = candidate_sequences(), record()["candidates"]
    for kind, args in CAND_GRID.items():
        assert len(got[kind]) == len(want[kind]) == len(args)
        for a, g, w in zip(args, got[kind], want[kind]):
            assert g == w, (kind, a)          # content and order: the tuner lets the first of equals win


@pytest.mark.parametrize("name", list(DESCS))
def test_query_agrees_with_the_old_queries(name):
    """Status and output size of the fp32 engine; workspace bytes of both engines wherever the query accepts the launch."""
    L = lib()
    n16 = 0
    for mth, up2, cfg, sk in points():
        d, ho, wo = desc(name, cfg, mth, up2, sk), ctypes.c_int(-1), ctypes.c_int(-1)
        st, info = query(ENGINE32, d)
        assert st == L.arseg_conv_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)), (mth, up2, cfg, sk)
        if st == OK:
            assert (info.Ho, info.Wo) == (ho.value, wo.value)
            assert info.workspace_bytes == L.arseg_conv2d_workspace_bytes(ctypes.byref(d))
            assert (info.workspace_bytes > 0) == (info.nsplit > 1)
            assert bool(info.patch_tw) == (info.kind == PATCH) and info.patch_tw * info.patch_th == (info.bm if info.kind == PATCH else 0)
        st16, info16 = query(ENGINE16, d)
        assert st16 in (OK, EINVAL, EUNSUPPORTED)
        if st16 == OK:
            n16 += 1
            assert (info16.Ho, info16.Wo) == tuple(record()["queries"][name]["hw"])
            assert info16.workspace_bytes == L.arseg_conv2d16_workspace_bytes(ctypes.byref(d)), (mth, up2, cfg, sk)
    assert n16 or name in ("stem_cin4", "batch36")          # (Cin % 8 and batched mode: not the 16-bit engine's)


@pytest.mark.parametrize("engine, table, fuses, no_split", [(ENGINE32, TABLE32, FUSES32, NO_SPLIT32), (ENGINE16, TABLE16, FUSES16, NO_SPLIT16)])
def test_every_id_is_what_the_header_says(engine, table, fuses, no_split):
    from arseg_amd import _lib

    for cfg in range(-2, len(table) + 3):
        row = _lib.conv_plan_row(engine, cfg)
        want = table.get(cfg, (NONE, 0, 0, 0, 0))
        assert (row.kind, row.bm, row.bn, row.bk, row.nbuf) == want, cfg
        assert bool(row.fuses_upsample) == (cfg in fuses) and bool(row.split_k_allowed) == (cfg in table and cfg not in no_split), cfg
        # ... and on a shape every plan kind has an id for, the accepted launch reports the row (the auto plans: a tile of the table)
        for name in ("c64_w100", "stem"):
            st, info = query(engine, desc(name, cfg, F16X3, 1 if cfg == 23 and engine == ENGINE32 else 0))
            if st == OK:
                got = (info.kind, info.bm, info.bn, info.bk, info.nbuf)
                assert got == want if want[0] != AUTO else got in [(AUTO,) + r[1:] for r in table.values() if r[0] == TILE], (cfg, name)


@pytest.mark.parametrize("engine, forced", [(ENGINE32, FORCED_TW32), (ENGINE16, FORCED_TW16)])
def test_patch_tile_width_follows_the_map(engine, forced):
    """64 / 32 / 16 wide tiles from map widths 48 and 24; a squarer tile is refused where the by-width tile is already that narrow."""
    table = TABLE32 if engine == ENGINE32 else TABLE16
    for name, by_width in (("c64_w16", 16), ("c64_w24", 32), ("c64_w40", 32), ("c64_w50", 64), ("c64_w100", 64)):
        for cfg in (c for c, r in table.items() if r[0] == PATCH):
            st, info = query(engine, desc(name, cfg, F16X3))
            tw = forced.get(cfg, by_width)
            if cfg in forced and by_width <= tw:
                assert st == EUNSUPPORTED, (name, cfg)
            else:
                assert st == OK and (info.patch_tw, info.patch_th) == (tw, table[cfg][1] // tw), (name, cfg)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec = {"queries": {name: old_queries(name) for name in DESCS}, "candidates": candidate_sequences()}
    with open(RECORD, "w") as f:
        f.write('{"queries": {\n')
        f.write(",\n".join(f'{json.dumps(name)}: {json.dumps(q, separators=(",", ":"))}' for name, q in rec["queries"].items()))
        f.write('},\n"candidates": {\n')
        f.write(",\n".join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in rec["candidates"].items()))
        f.write("}}\n")
    print(f"wrote {RECORD}: {os.path.getsize(RECORD)} bytes")
