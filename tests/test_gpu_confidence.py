"""GPU checks of the segmentation confidence (csrc/confidence.hip, arseg_segment_confidence_fwd; arseg_amd.egress.confidence): the codes
against the float64 oracle under its comparison rule (tests/confidence_oracle.py), the label plane against the EXISTING evaluator tail
(ops.argmax_confusion, zero differing pixels), the statistics against the planes the same launch wrote, exactly."""
import numpy as np
import pytest
import torch

import confidence_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _existing(logits, H, W, align):
    from arseg_amd import ops

    return ops.argmax_confusion(logits, None, H, W, align_corners=align)[0]


def _want_stats(conf, pred, low, n_cls):
    """int64 [N, CONF_NSTATS] from a confidence plane and the tail's pred, both numpy."""
    from arseg_amd import _lib

    N = conf.shape[0]
    out = np.zeros((N, _lib.CONF_NSTATS), dtype=np.int64)
    for n in range(N):
        out[n, 0] = conf[n].astype(np.int64).sum()
        out[n, 1] = int((conf[n].astype(np.int64) < low).sum())
        out[n, 2:2 + n_cls] = np.bincount(pred[n].reshape(-1), minlength=n_cls)
    return out


def _backed(N, H, W, pad, dev, fill):
    """(backing device buffer [N+1,H,W+pad] of GUARD bytes, its view [:N,:,:W] filled with ``fill``)."""
    buf = np.full((N + 1, H, W + pad), GUARD, dtype=np.uint8)
    buf[:N, :, :W] = fill
    t = torch.from_numpy(buf).to(dev)
    return t, t[:N, :, :W]


def _guards_intact(backing, N, W):
    b = backing.cpu().numpy()
    return bool((b[:N, :, W:] == GUARD).all() and (b[N:] == GUARD).all())


@pytest.fixture(scope="module")
def references():
    """(case name, kind) -> exact 255 c of the oracle, computed once per module."""
    cache = {}

    def get(case, kind):
        key = (case[0], kind)
        if key not in cache:
            cache[key] = oracle.exact(oracle.case_logits(case), case[6], case[7], case[8], kind)
        return cache[key]
    return get


@pytest.mark.parametrize("kind", oracle.KINDS)
@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_codes_labels_and_stats_on_every_route(dev, references, case, kind):
    """One launch writes conf8, labels8 and stats: the codes hold the comparison rule against the oracle, labels8 == the tail's pred with no
    differing pixel, and the statistics equal what the two planes say, exactly."""
    from arseg_amd import egress

    name, _, N, n_cls, h, w, H, W, align = case
    logits = torch.from_numpy(oracle.case_logits(case)).to(dev)
    pred = _existing(logits, H, W, align)
    conf, labels, stats = egress.confidence(logits, H, W, kind=kind, low=128, labels_out=True, stats=True, align_corners=align)
    assert conf.dtype == torch.uint8 and tuple(conf.shape) == (N, H, W) and labels.dtype == torch.uint8 and tuple(stats.shape) == (N, 34)
    diff = int((labels.int() != pred).sum())
    print(f"\n{name}: {diff} differing labels of {pred.numel()}")
    assert diff == 0
    oracle.check(conf.cpu().numpy(), references(case, kind), f"{name} {kind}")
    assert np.array_equal(stats.cpu().numpy(), _want_stats(conf.cpu().numpy(), pred.cpu().numpy(), 128, n_cls))


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_one_class(dev, case):
    """n_cls == 1: top-1 and margin are both 255 everywhere, every label is 0, the whole frame counts into class 0."""
    from arseg_amd import egress

    _, seed, N, _, h, w, H, W, align = case
    logits = torch.from_numpy(oracle.make_logits(seed + 50, N, 1, h, w)).to(dev)
    for kind in oracle.KINDS:
        conf, labels, stats = egress.confidence(logits, H, W, kind=kind, low=255, labels_out=True, stats=True, align_corners=align)
        assert bool((conf == 255).all()) and bool((labels == 0).all())
        s = stats.cpu().numpy()
        assert (s[:, 0] == 255 * H * W).all() and (s[:, 1] == 0).all() and (s[:, 2] == H * W).all() and (s[:, 3:] == 0).all()


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_labels_through_a_lut(dev, case):
    """With a LUT labels8 equals egress.labels8 (and lut[pred]); the statistics stay unmapped."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align = case
    logits = torch.from_numpy(oracle.case_logits(case)).to(dev)
    lut = np.random.Generator(np.random.PCG64(2)).integers(0, 256, n_cls, dtype=np.uint8)
    conf, labels, stats = egress.confidence(logits, H, W, labels_out=True, lut=lut, stats=True, align_corners=align)
    pred = _existing(logits, H, W, align)
    assert torch.equal(labels, egress.labels8(logits, H, W, lut=lut, align_corners=align))
    assert torch.equal(labels, torch.from_numpy(lut).to(dev)[pred.long()])
    assert np.array_equal(stats.cpu().numpy()[:, 2:2 + n_cls], _want_stats(conf.cpu().numpy(), pred.cpu().numpy(), 128, n_cls)[:, 2:2 + n_cls])


@pytest.mark.parametrize("kind", oracle.KINDS)
@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_ties_nans_and_infinities(dev, case, kind):
    """Planted exact ties (the code is continuous across them, the label is the first maximum), a NaN logit, a +inf logit and an all -inf
    pixel: q = 0 wherever the contract's c is NaN, the rule everywhere else, labels == the tail's.  On the same-size route the three planted
    pixels are exactly the zeros the plants cause, and a two-way tie of the maximum gives margin 0."""
    from arseg_amd import egress

    name, _, N, n_cls, h, w, H, W, align = case
    x = oracle.case_logits(case)
    where = oracle.plant_specials(x)
    logits = torch.from_numpy(x).to(dev)
    conf, labels, _ = egress.confidence(logits, H, W, kind=kind, labels_out=True, align_corners=align)
    assert int((labels.int() != _existing(logits, H, W, align)).sum()) == 0
    want = oracle.exact(x, H, W, align, kind)
    q = conf.cpu().numpy()
    assert np.isnan(want).any() and (q[np.isnan(want)] == 0).all()
    oracle.check(q, want, f"{name} {kind} with plants")
    if name == "same":
        assert int(np.isnan(want).sum()) == len(where)
        for n, yy, xx in where:
            assert q[n, yy, xx] == 0
        clean = egress.confidence(torch.from_numpy(oracle.case_logits(case)).to(dev), H, W, kind=kind, align_corners=align)[0].cpu().numpy()
        untouched = np.ones_like(q, dtype=bool)
        untouched[:, 4, :] = False
        untouched[:, 6, 2::3] = False
        for n, yy, xx in where:
            untouched[n, yy, xx] = False
        assert np.array_equal(q[untouched], clean[untouched])          # the neighbours are unaffected
        if kind == "margin":
            assert (q[:, 4, :] == 0).all()


@pytest.mark.parametrize("pitch", ["odd", "aligned"])
@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_pitched_planes_and_a_frame_slice(dev, case, pitch):
    """conf8 and labels8 into a [1:3] slice of pitched buffers (an odd pitch, and a 4-byte aligned one): the planes equal the dense call's
    frames 1..2, frame 0 and the guard bytes after every row and after the last image stay as they were; the statistics rows belong to the
    slice."""
    from arseg_amd import egress

    _, _, _, n_cls, h, w, H, W, align = case
    N = 3
    x = np.concatenate([oracle.case_logits(case)] * 2)[:N]
    logits = torch.from_numpy(x).to(dev)
    pad = 3 if pitch == "odd" else ((-W) % 4 or 4)                                # every W here is even
    assert (W + pad) % 2 == 1 if pitch == "odd" else (W + pad) % 4 == 0
    dense_c, dense_l, dense_s = egress.confidence(logits, H, W, kind="margin", labels_out=True, stats=True, align_corners=align)
    cb, cv = _backed(N, H, W, pad, dev, 7)
    lb, lv = _backed(N, H, W, pad + (2 if pitch == "odd" else 4), dev, 9)         # the label plane has its own pitch, of the same kind
    stats = torch.zeros((N, 34), dtype=torch.int64, device=dev)
    egress.confidence(logits[1:3].contiguous(), H, W, kind="margin", out=cv[1:3], labels_out=lv[1:3], stats=stats[1:3], align_corners=align)
    assert torch.equal(cv[1:3], dense_c[1:3]) and torch.equal(lv[1:3], dense_l[1:3])
    assert bool((cv[0] == 7).all()) and bool((lv[0] == 9).all())
    assert _guards_intact(cb, N, W) and _guards_intact(lb, N, W)
    assert torch.equal(stats[1:3], dense_s[1:3]) and bool((stats[0] == 0).all())


@pytest.mark.parametrize("low", [0, 1, 128, 256])
@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_statistics(dev, case, low):
    """Row n == (sum of conf8[n], count(conf8[n] < low), bincount(pred[n])) exactly; stats alone == stats with planes; two launches into one
    buffer give exactly twice one launch; two runs are bit-equal."""
    from arseg_amd import egress, ops

    _, _, N, n_cls, h, w, H, W, align = case
    logits = torch.from_numpy(oracle.case_logits(case)).to(dev)
    pred = _existing(logits, H, W, align).cpu().numpy()
    conf, _, stats = egress.confidence(logits, H, W, low=low, labels_out=True, stats=True, align_corners=align)
    want = _want_stats(conf.cpu().numpy(), pred, low, n_cls)
    assert np.array_equal(stats.cpu().numpy(), want)
    if low == 0:
        assert (want[:, 1] == 0).all()
    if low == 256:
        assert (want[:, 1] == H * W).all()
    alone = torch.zeros((N, 34), dtype=torch.int64, device=dev)
    ops.segment_confidence(logits, H, W, low=low, align_corners=align, stats=alone)
    assert torch.equal(alone, stats)
    ops.segment_confidence(logits, H, W, low=low, align_corners=align, stats=alone)
    assert torch.equal(alone, 2 * stats)
    conf2, _, stats2 = egress.confidence(logits, H, W, low=low, labels_out=True, stats=True, align_corners=align)
    assert torch.equal(conf2, conf) and torch.equal(stats2, stats)


def test_confidence_in_one_graph(dev):
    """egress.confidence(..., out=, labels_out=, stats=) captured once; the logits are refilled in place; each of two replays equals the
    eager result for its own logits (the statistics buffer is zeroed before a replay: it is accumulated into)."""
    from arseg_amd import egress

    case = oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align = case
    static = torch.from_numpy(oracle.case_logits(case)).to(dev)
    conf = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    labels = torch.zeros_like(conf)
    stats = torch.zeros((N, 34), dtype=torch.int64, device=dev)
    egress.confidence(static, H, W, out=conf, labels_out=labels, stats=stats, align_corners=align)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        egress.confidence(static, H, W, out=conf, labels_out=labels, stats=stats, align_corners=align)
    for s in (seed + 60, seed + 61):
        fresh = torch.from_numpy(oracle.make_logits(s, N, n_cls, h, w)).to(dev)
        static.copy_(fresh)
        conf.zero_()
        labels.zero_()
        stats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_c, want_l, want_s = egress.confidence(fresh, H, W, labels_out=True, stats=True, align_corners=align)
        assert torch.equal(conf, want_c) and torch.equal(labels, want_l) and torch.equal(stats, want_s)
        assert int((labels.int() != _existing(fresh, H, W, align)).sum()) == 0


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_alter_res_batch_confidence(dev, manifest, kind):
    """The small PSPNet (fp32) and BiSeNet (bf16, fused x8 tail) of tests/test_gpu_models.py: alter_res_batch_confidence's labels equal
    alter_res_batch_render's, its conf8 holds the comparison rule against the oracle applied to the logits the net produced (the same
    phase 1 / phase 2 calls and route decision, made here by hand), and its statistics equal its planes."""
    import test_gpu_ingest_formats as tf          # its _nets wraps test_gpu_models' _psp / _bise (+ bf16 storage)
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth

    hr, lr = tf._nets(manifest, dev, kind)
    H, W = (64, 96) if kind == "psp" else (128, 256)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    clip = synth.make_clip(9, H, W, gop=4, mean=mean, std=std)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * 3
        labels_r, _ = ev.alter_res_batch_render(lr, refs, frames[1:4], mvs[1:4], 0.5)
        conf, labels, stats = ev.alter_res_batch_confidence(lr, refs, frames[1:4], mvs[1:4], 0.5, kind="top1", low=100)
        net = ev._unwrap(lr)
        h, w = ev._downscale_hw(H, W, 0.5)
        feat = net.phase1_nhwc4(ops.ingest_input(frames[1:4], h, w, net.storage_dtype), aux=ops.config.aux_outputs)[-1]
        if kind == "bise":
            lo, _ = net.phase2_warp(feat, list(refs), mvs[1:4], upsample=False)
            assert (8 * lo.shape[-2], 8 * lo.shape[-1]) == (H, W)
        else:
            lo, _ = net.phase2_warp(feat, list(refs), mvs[1:4])
    assert int((labels != labels_r).sum()) == 0
    lo_np = lo.float().cpu().numpy()
    print(f"\n{kind}: logits {lo_np.shape}, max |logit| {np.abs(lo_np).max():.2f}")
    oracle.check(conf.cpu().numpy(), oracle.exact(lo_np, H, W, kind != "bise", "top1"), f"alter_res_batch_confidence {kind}")
    n_cls = lo.shape[1]
    assert np.array_equal(stats.cpu().numpy(), _want_stats(conf.cpu().numpy(), labels.cpu().numpy().astype(np.int64), 100, n_cls))


def test_full_size_x8_grid_arithmetic(dev):
    """One 1024x2048 frame, 19 classes, x8 run route: the statistics against the planes of the same launch, the labels against the tail."""
    from arseg_amd import egress

    H, W, n_cls = 1024, 2048, 19
    logits = torch.from_numpy(oracle.make_logits(171, 1, n_cls, H // 8, W // 8)).to(dev)
    conf, labels, stats = egress.confidence(logits, H, W, low=128, labels_out=True, stats=True, align_corners=False)
    pred = _existing(logits, H, W, False)
    assert int((labels.int() != pred).sum()) == 0
    want = torch.zeros((1, 34), dtype=torch.int64, device=dev)
    want[0, 0] = conf.long().sum()
    want[0, 1] = (conf < 128).sum()
    want[0, 2:2 + n_cls] = torch.bincount(pred.reshape(-1).long(), minlength=n_cls)
    assert torch.equal(stats, want) and int(stats[0, 2:].sum()) == H * W
