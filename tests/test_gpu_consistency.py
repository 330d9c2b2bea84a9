"""GPU checks of the temporal consistency (csrc/consistency.hip, arseg_segment_consistency_fwd / arseg_labels_consistency_fwd;
arseg_amd.egress.consistency): the label plane against the EXISTING evaluator tail (ops.argmax_confusion, zero differing pixels), the change
plane and the statistics against the numpy oracle fed those labels (tests/consistency_oracle.py).  Every output is an integer: every
comparison is exact."""
import numpy as np
import pytest
import torch

import consistency_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0xA5
NS = oracle.TC_NSTATS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs(dev):
    """case -> its seeded input on the device plus the tail's pred and the oracle's answer for it, computed once per module and not modified:
    dict(logits, ref, mv, pred (numpy int64), change, stats (numpy))."""
    from arseg_amd import ops

    cache = {}

    def get(case):
        if case[0] not in cache:
            b = oracle.build(case)
            logits = torch.from_numpy(b["logits"]).to(dev)
            pred = ops.argmax_confusion(logits, None, case[6], case[7], align_corners=case[8])[0].cpu().numpy().astype(np.int64)
            change, stats, _ = oracle.consistency(pred, b["ref"], b["mv"], case[3])
            cache[case[0]] = {"logits": logits, "ref": torch.from_numpy(b["ref"]).to(dev), "mv": torch.from_numpy(b["mv"]).to(dev),
                              "ref_np": b["ref"], "mv_np": b["mv"], "pred": pred, "change": change, "stats": stats}
        return cache[case[0]]
    return get


def _same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


def _backed(N, H, W, pad, dev, fill):
    """(backing device buffer [N+1,H,W+pad] of GUARD bytes, its view [:N,:,:W] filled with ``fill``)."""
    buf = np.full((N + 1, H, W + pad), GUARD, dtype=np.uint8)
    buf[:N, :, :W] = fill
    t = torch.from_numpy(buf).to(dev)
    return t, t[:N, :, :W]


def _guards_intact(backing, N, W):
    b = backing.cpu().numpy()
    return bool((b[:N, :, W:] == GUARD).all() and (b[N:] == GUARD).all())


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_labels_change_and_stats_on_every_route(dev, inputs, case):
    """One launch writes labels8, change8 and stats on every route, with 12, 19 and 32 classes, against shared and per-frame reference
    planes: labels8 == the tail's pred with no differing pixel; change8 and stats == the oracle fed those labels."""
    from arseg_amd import egress

    name, _, N, n_cls, h, w, H, W, align, shared = case
    i = inputs(case)
    assert tuple(i["ref"].shape) == ((1 if shared else N), H, W)
    change, labels, stats = egress.consistency(i["logits"], i["ref"], i["mv"], H, W, change_out=True, labels_out=True, align_corners=align)
    assert change.dtype == torch.uint8 and tuple(change.shape) == (N, H, W) and labels.dtype == torch.uint8 and tuple(stats.shape) == (N, NS)
    diff = int((labels.cpu().numpy().astype(np.int64) != i["pred"]).sum())
    got = stats.cpu().numpy()
    print(f"\n{name}: {diff} differing labels of {i['pred'].size}; compared / outside / void per frame {got[:, :3].tolist()}")
    assert diff == 0
    assert _same(change, i["change"])
    assert np.array_equal(got, i["stats"])


@pytest.mark.parametrize("case", [oracle.CASES[0], oracle.CASES[1], oracle.CASES[4]], ids=lambda c: c[0])
def test_one_class(dev, inputs, case):
    """n_cls == 1 on the three routes: every label is 0; a pixel agrees wherever its target is in the frame and not void, and never differs."""
    from arseg_amd import egress

    _, seed, N, _, h, w, H, W, align, _ = case
    i = inputs(case)
    g = np.random.Generator(np.random.PCG64(seed + 50))
    logits = torch.from_numpy(g.standard_normal((N, 1, h, w)).astype(np.float32)).to(dev)
    ref_np = np.where(i["ref_np"] == 255, 255, 0).astype(np.uint8)
    change, labels, stats = egress.consistency(logits, torch.from_numpy(ref_np).to(dev), i["mv"], H, W, change_out=True, labels_out=True,
                                               align_corners=align)
    want_c, want_s, _ = oracle.consistency(np.zeros((N, H, W), dtype=np.int64), ref_np, i["mv_np"], 1)
    assert bool((labels == 0).all()) and _same(change, want_c) and _same(stats, want_s)
    s = stats.cpu().numpy()
    assert not (want_c == 255).any() and (s[:, 0] > 0).all() and (s[:, 3] == s[:, 0]).all() and (s[:, 67] == s[:, 0]).all() and (s[:, 2] > 0).all()


@pytest.mark.parametrize("case", [oracle.CASES[1], oracle.CASES[2]], ids=lambda c: c[0])
def test_shared_against_per_frame_reference_planes(dev, inputs, case):
    """A shared plane ([1,H,W], and [H,W]) gives what N copies of it give as a per-frame stack, and a stack of different planes differs."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, shared = case
    assert shared
    i = inputs(case)
    stack = i["ref"].expand(N, H, W).contiguous()
    for ref in (i["ref"][0], stack):
        change, _, stats = egress.consistency(i["logits"], ref, i["mv"], H, W, change_out=True, align_corners=align)
        assert _same(change, i["change"]) and _same(stats, i["stats"])
    rolled = stack.clone()
    rolled[1] = torch.roll(stack[1], shifts=(1, 2), dims=(0, 1))
    change, _, stats = egress.consistency(i["logits"], rolled, i["mv"], H, W, change_out=True, align_corners=align)
    want_c, want_s, _ = oracle.consistency(i["pred"], rolled.cpu().numpy(), i["mv_np"], n_cls)
    assert _same(change, want_c) and _same(stats, want_s) and not np.array_equal(want_c[1], i["change"][1])
    assert np.array_equal(want_c[0], i["change"][0])


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_int16_corners_all_outside_and_all_void(dev, inputs, case):
    """Vectors at the corners of int16 (and one short of them) planted over the seeded field; a frame whose every vector points off the
    frame (nothing is read from the reference); a reference of 255s (compared == 0)."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, shared = case
    i = inputs(case)
    mv = i["mv_np"].copy()
    corners = np.array([-32768, 32767, -32767, 32766, -32766, 0], dtype=np.int16)
    g = np.random.Generator(np.random.PCG64(case[1] + 7))
    mask = g.random((N, H, W)) < 0.3
    planted = g.choice(corners, (N, H, W, 2))
    planted[..., 0] = np.where(planted[..., 0] == 0, 32767, planted[..., 0])          # at least one component at a corner
    mv[mask] = planted[mask]
    change, _, stats = egress.consistency(i["logits"], i["ref"], torch.from_numpy(mv).to(dev), H, W, change_out=True, align_corners=align)
    want_c, want_s, _ = oracle.consistency(i["pred"], i["ref_np"], mv, n_cls)
    assert _same(change, want_c) and _same(stats, want_s) and (want_s[:, 1] >= mask.sum(axis=(1, 2))).all()

    out = np.empty_like(mv)
    out[..., 0], out[..., 1] = 4 * W, -4 * H
    out[0, :, :, 1] = 0                                                                # frame 0 leaves through the right edge alone
    change, _, stats = egress.consistency(i["logits"], i["ref"], torch.from_numpy(out).to(dev), H, W, change_out=True, align_corners=align)
    s = stats.cpu().numpy()
    assert bool((change == 128).all()) and (s[:, 1] == H * W).all() and not s[:, 0].any() and not s[:, 2:].any()

    void = torch.full_like(i["ref"], 255)
    change, _, stats = egress.consistency(i["logits"], void, i["mv"], H, W, change_out=True, align_corners=align)
    want_c, want_s, _ = oracle.consistency(i["pred"], np.full_like(i["ref_np"], 255), i["mv_np"], n_cls)
    s = stats.cpu().numpy()
    assert bool((change == 128).all()) and np.array_equal(s, want_s) and not s[:, 0].any() and not s[:, 3:].any()
    assert (s[:, 2] > 0).all() and (s[:, 1] + s[:, 2] == H * W).all()


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_lut_changes_labels_out_only(dev, inputs, case):
    """With a LUT labels8 equals egress.labels8 (and lut[pred]); the reference stays in train ids, so change8 and stats do not move."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    lut = np.random.Generator(np.random.PCG64(2)).integers(0, 256, n_cls, dtype=np.uint8)
    change, labels, stats = egress.consistency(i["logits"], i["ref"], i["mv"], H, W, change_out=True, labels_out=True, lut=lut, align_corners=align)
    assert torch.equal(labels, egress.labels8(i["logits"], H, W, lut=lut, align_corners=align))
    assert _same(labels, lut[i["pred"]])
    assert _same(change, i["change"]) and _same(stats, i["stats"])


@pytest.mark.parametrize("pitch", ["odd", "aligned"])
@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_pitched_planes_and_a_frame_slice(dev, inputs, case, pitch):
    """labels8, change8 and the reference in [1:3] slices of pitched buffers (an odd pitch, and a 4-byte aligned one): the planes equal
    the dense call's frames 1..2, frame 0 and the guard bytes after every row and after the last image stay as they were; the statistics
    rows belong to the slice."""
    from arseg_amd import egress

    _, _, _, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    N = 3
    logits = torch.cat([i["logits"]] * 2)[:N].contiguous()
    mv = torch.cat([i["mv"]] * 2)[:N].contiguous()
    ref_np = np.concatenate([np.broadcast_to(i["ref_np"], (i["logits"].shape[0], H, W))] * 2)[:N]
    pad = 3 if pitch == "odd" else ((-W) % 4 or 4)                                # every W here is even
    assert (W + pad) % 2 == 1 if pitch == "odd" else (W + pad) % 4 == 0
    dense_c, dense_l, dense_s = egress.consistency(logits, torch.from_numpy(np.ascontiguousarray(ref_np)).to(dev), mv, H, W, change_out=True,
                                                   labels_out=True, align_corners=align)
    cb, cv = _backed(N, H, W, pad, dev, 7)
    lb, lv = _backed(N, H, W, pad + (2 if pitch == "odd" else 4), dev, 9)         # the label plane has its own pitch, of the same kind
    rb, rv = _backed(N, H, W, pad + (4 if pitch == "odd" else 8), dev, ref_np)
    stats = torch.zeros((N, NS), dtype=torch.int64, device=dev)
    egress.consistency(logits[1:3].contiguous(), rv[1:3], mv[1:3], H, W, change_out=cv[1:3], labels_out=lv[1:3], stats=stats[1:3], align_corners=align)
    assert torch.equal(cv[1:3], dense_c[1:3]) and torch.equal(lv[1:3], dense_l[1:3])
    assert bool((cv[0] == 7).all()) and bool((lv[0] == 9).all())
    assert _guards_intact(cb, N, W) and _guards_intact(lb, N, W) and _guards_intact(rb, N, W)
    assert torch.equal(stats[1:3], dense_s[1:3]) and bool((stats[0] == 0).all())
    pc, ps = egress.consistency_of_planes(lv[1:3], rv[1:3], mv[1:3], n_cls, change_out=True)          # a pitched source plane
    assert torch.equal(pc, dense_c[1:3]) and torch.equal(ps, dense_s[1:3])


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_statistics(dev, inputs, case):
    """stats alone == stats with planes; two launches into one buffer give exactly twice one launch; two runs are bit-equal."""
    from arseg_amd import egress, ops

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    ref = i["ref"]
    change, labels, stats = egress.consistency(i["logits"], ref, i["mv"], H, W, change_out=True, labels_out=True, align_corners=align)
    assert _same(stats, i["stats"])
    alone = torch.zeros((N, NS), dtype=torch.int64, device=dev)
    ops.segment_consistency(i["logits"], ref, i["mv"], H, W, align_corners=align, stats=alone)
    assert torch.equal(alone, stats)
    ops.segment_consistency(i["logits"], ref, i["mv"], H, W, align_corners=align, stats=alone)
    assert torch.equal(alone, 2 * stats)
    change2, labels2, stats2 = egress.consistency(i["logits"], ref, i["mv"], H, W, change_out=True, labels_out=True, align_corners=align)
    assert torch.equal(change2, change) and torch.equal(labels2, labels) and torch.equal(stats2, stats)
    only_c, none_l, none_s = egress.consistency(i["logits"], ref, i["mv"], H, W, change_out=True, stats=None, align_corners=align)
    assert none_l is None and none_s is None and torch.equal(only_c, change)
    with pytest.raises(ValueError):
        egress.consistency(i["logits"], ref, i["mv"], H, W, stats=None, align_corners=align)


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_plane_form(dev, inputs, case):
    """Fed the fused form's own labels the plane form gives identical change8 and stats; a source with 255s counts those pixels as void
    (where their target is in the frame); stats alone == stats with the plane."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    change, labels, stats = egress.consistency(i["logits"], i["ref"], i["mv"], H, W, change_out=True, labels_out=True, align_corners=align)
    pc, ps = egress.consistency_of_planes(labels, i["ref"], i["mv"], n_cls, change_out=True)
    assert torch.equal(pc, change) and torch.equal(ps, stats)
    src = i["pred"].copy()
    holes = np.random.Generator(np.random.PCG64(case[1] + 9)).random(src.shape) < 0.15
    src[holes] = 255
    src[0, H // 2, :] = n_cls                                                       # the smallest void value
    pc, ps = egress.consistency_of_planes(torch.from_numpy(src.astype(np.uint8)).to(dev), i["ref"], i["mv"], n_cls, change_out=True)
    want_c, want_s, _ = oracle.consistency(src, i["ref_np"], i["mv_np"], n_cls)
    assert _same(pc, want_c) and _same(ps, want_s) and (want_s[:, 2] > i["stats"][:, 2]).all()
    none_c, alone = egress.consistency_of_planes(torch.from_numpy(src.astype(np.uint8)).to(dev), i["ref"], i["mv"], n_cls)
    assert none_c is None and torch.equal(alone, ps)


def test_consistency_in_one_graph(dev, inputs):
    """egress.consistency(..., change_out=, labels_out=, stats=) captured once; the logits and mv_q are refilled in place; each of two replays
    equals the eager result for its own inputs (the statistics buffer is zeroed before a replay: it is accumulated into)."""
    from arseg_amd import egress

    case = oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    logits, mv = i["logits"].clone(), i["mv"].clone()
    change = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    labels = torch.zeros_like(change)
    stats = torch.zeros((N, NS), dtype=torch.int64, device=dev)
    egress.consistency(logits, i["ref"], mv, H, W, change_out=change, labels_out=labels, stats=stats, align_corners=align)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        egress.consistency(logits, i["ref"], mv, H, W, change_out=change, labels_out=labels, stats=stats, align_corners=align)
    for s in (seed + 60, seed + 61):
        fresh = oracle.build((case[0], s) + case[2:])
        f_logits, f_mv = torch.from_numpy(fresh["logits"]).to(dev), torch.from_numpy(fresh["mv"]).to(dev)
        logits.copy_(f_logits)
        mv.copy_(f_mv)
        change.zero_()
        labels.zero_()
        stats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_c, want_l, want_s = egress.consistency(f_logits, i["ref"], f_mv, H, W, change_out=True, labels_out=True, align_corners=align)
        assert torch.equal(change, want_c) and torch.equal(labels, want_l) and torch.equal(stats, want_s)
        o_c, o_s, _ = oracle.consistency(labels.cpu().numpy(), i["ref_np"], fresh["mv"], n_cls)
        assert _same(change, o_c) and _same(stats, o_s)


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_alter_res_batch_consistency(dev, manifest, kind):
    """The small PSPNet (fp32) and BiSeNet (bf16, fused x8 tail) of tests/test_gpu_models.py, the motion from an ingest.MotionChain, the
    keyframe's plane from egress.labels8(forward_keyframe(...)): alter_res_batch_consistency's labels equal alter_res_batch_render's, and
    its change8 and statistics equal the oracle fed those labels."""
    import test_gpu_ingest_formats as tf          # its _nets wraps test_gpu_models' _psp / _bise (+ bf16 storage)
    from arseg_amd import egress, ingest, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, kind)
    H, W, gop = ((64, 96) if kind == "psp" else (128, 256)) + (4,)
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    chain = ingest.MotionChain(H, W, gop=gop, device=dev)
    recs = [torch.from_numpy(np.ascontiguousarray(r, dtype=np.int16)).to(dev) for r in synth.make_record_chain(31, H, W, gop - 1)]
    mvs = chain.push_gop(recs)[1:]
    with torch.no_grad():
        key_logits, feat_k = hr.forward_keyframe(frames[0:1])
        key_labels = egress.labels8(key_logits.float(), H, W)
        refs = [feat_k[0]] * (gop - 1)
        labels_r, _ = ev.alter_res_batch_render(lr, refs, frames[1:gop], mvs, 0.5)
        change, labels, stats = ev.alter_res_batch_consistency(lr, refs, frames[1:gop], mvs, key_labels, 0.5)
    assert tuple(key_labels.shape) == (1, H, W) and int((labels != labels_r).sum()) == 0
    n_cls = key_logits.shape[1]
    want_c, want_s, _ = oracle.consistency(labels.cpu().numpy(), key_labels.cpu().numpy(), mvs.cpu().numpy(), n_cls)
    table = egress.tc_table(stats, n_cls)
    print(f"\n{kind}: compared / outside / void {want_s[:, :3].tolist()}, agreement {table['agreement'].tolist()}, TC {table['tc_miou'].tolist()}")
    assert _same(change, want_c) and _same(stats, want_s) and bool((mvs != 0).any())
    for got, want in zip(zip(table["agreement"], table["tc_miou"], table["compared_share"]), oracle.tc_rows(want_s, n_cls)):
        assert all((np.isnan(g) and np.isnan(x)) or abs(g - x) <= 1e-12 for g, x in zip(got, want))


def test_full_size_x8_grid_arithmetic(dev):
    """One 1024x2048 frame, 19 classes, x8 run route: the labels against the tail, change8 and the statistics against the oracle fed the
    tail's pred.  The reference is the pred itself displaced, with a void rectangle; the field is block constant, partly pointing back,
    partly wrong, partly off the frame."""
    from arseg_amd import egress, ops

    H, W, n_cls, bs = 1024, 2048, 19, 64
    g = np.random.Generator(np.random.PCG64(271))
    logits = torch.from_numpy(oracle.make_logits(g, 1, n_cls, H // 8, W // 8)).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=False)[0]
    ref = torch.roll(pred, shifts=(3, -5), dims=(1, 2)).to(torch.uint8)
    ref[0, 300:420, 900:1300] = 255
    blocks = np.tile(np.array([-20, 12], dtype=np.int16), (H // bs, W // bs, 1))          # points back: round(-20 / 4) = -5, 12 / 4 = 3
    blocks[g.random((H // bs, W // bs)) < 0.2] = (-22, 14)                                # -5.5 -> -6, 3.5 -> 4: wrong by one pixel each way
    blocks[0, :] = (0, -4 * bs - 2)                                                       # the top block row leaves the frame
    blocks[:, -1] = (32767, -32768)
    mv = np.repeat(np.repeat(blocks, bs, axis=0), bs, axis=1)[None]
    change, labels, stats = egress.consistency(logits, ref, torch.from_numpy(np.ascontiguousarray(mv)).to(dev), H, W, change_out=True,
                                               labels_out=True, align_corners=False)
    assert int((labels.int() != pred).sum()) == 0
    want_c, want_s, _ = oracle.consistency(pred.cpu().numpy(), ref.cpu().numpy(), mv, n_cls)
    assert _same(change, want_c) and _same(stats, want_s)
    s = want_s[0]
    assert s[:3].sum() == H * W and s[0] > 0.5 * H * W and s[1] > 0 and s[2] > 0 and 0 < s[67:99].sum() < s[0]
