"""GPU tests of the grouped evaluator tail (one confusion matrix per keyframe distance) and of what is built on it: ops.argmax_confusion_grouped
against the ungrouped ops.argmax_confusion (which the op tests hold to torch and the oracle) and against torch directly, EvalByDistance
against EvalAlterRes / EvalConstRes run per distance, and the batched fast path with groups.  All comparisons are integer and exact."""
import math

import numpy as np
import pytest
import torch

from helpers import t
from test_gpu_models import _bise, _psp

pytestmark = pytest.mark.gpu

GROUPINGS = [(11, list(range(1, 12))), (7, [3, 3, 0, 5, 5, 5, 0])]          # a GOP's distances; repeated and unordered ids
N_GROUPS = 12
# (n_cls, h, w, H, W, align_corners): equal size, resized align_corners=True, the fused x8 / x4 / x2 run kernel, x3 (per-pixel kernel)
SHAPES = [(12, 12, 16, 12, 16, True), (12, 6, 8, 12, 16, True), (12, 24, 32, 13, 17, True),
          (19, 16, 24, 128, 192, False), (19, 5, 7, 40, 56, False), (19, 33, 65, 132, 260, False), (19, 9, 11, 18, 22, False),
          (19, 7, 5, 21, 15, False)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def rnd(seed, *shape):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32))


def labels(seed, N, H, W, n_cls):
    g = np.random.Generator(np.random.PCG64(seed))
    label = torch.from_numpy(g.integers(0, n_cls, (N, H, W)).astype(np.int64))
    label[0, :2, :3] = 255
    label[-1, -3:, :] = 255
    return label


@pytest.mark.parametrize("N,groups", GROUPINGS)
@pytest.mark.parametrize("n_cls,h,w,H,W,align", SHAPES)
def test_grouped_equals_ungrouped_frame_by_frame(dev, n_cls, h, w, H, W, align, N, groups):
    from arseg_amd import ops

    logits, label = rnd(162, N, n_cls, h, w).to(dev), labels(163, N, H, W, n_cls).to(dev)
    pred_u, hist_u = ops.argmax_confusion(logits, label, H, W, align_corners=align)
    pred_g, hist_g = ops.argmax_confusion_grouped(logits, label, groups, N_GROUPS, H, W, align_corners=align)
    assert pred_g.dtype == torch.int32 and hist_g.dtype == torch.int64 and tuple(hist_g.shape) == (N_GROUPS, n_cls, n_cls)
    assert torch.equal(pred_g, pred_u)                                           # bit-equal labels
    want = torch.zeros_like(hist_g)
    for n, g in enumerate(groups):
        p1, h1 = ops.argmax_confusion(logits[n:n + 1], label[n:n + 1], H, W, align_corners=align)
        assert torch.equal(p1[0], pred_g[n])
        want[g] += h1
    assert torch.equal(hist_g, want)
    assert torch.equal(hist_g.sum(0), hist_u)
    for g in set(range(N_GROUPS)) - set(groups):
        assert int(hist_g[g].sum()) == 0
    # the same ids as a device tensor
    pred_t, hist_t = ops.argmax_confusion_grouped(logits, label, torch.tensor(groups, dtype=torch.int32, device=dev), N_GROUPS, H, W, align_corners=align)
    assert torch.equal(pred_t, pred_g) and torch.equal(hist_t, hist_g)


@pytest.mark.parametrize("N,groups", GROUPINGS)
def test_grouped_against_torch_at_equal_size(dev, N, groups):
    from arseg_amd import ops

    n_cls, H, W = 12, 12, 16
    logits, label = rnd(164, N, n_cls, H, W), labels(165, N, H, W, n_cls)
    pred, hist = ops.argmax_confusion_grouped(logits.to(dev), label.to(dev), groups, N_GROUPS, H, W)
    want_p = torch.argmax(torch.softmax(logits, 1), 1)
    assert torch.equal(pred.cpu().long(), want_p)
    for g in range(N_GROUPS):
        sel = [n for n in range(N) if groups[n] == g]
        lab, prd = label[sel], want_p[sel]
        keep = lab != 255
        want_h = torch.bincount(lab[keep] * n_cls + prd[keep], minlength=n_cls * n_cls).view(n_cls, n_cls)
        assert torch.equal(hist[g].cpu(), want_h)


@pytest.mark.parametrize("n_cls,h,w,H,W,align", [SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[6]])
def test_grouped_semantics(dev, n_cls, h, w, H, W, align):
    from arseg_amd import ops

    N, groups = 7, [3, 3, 0, 5, 5, 5, 0]
    logits, label = rnd(166, N, n_cls, h, w).to(dev), labels(167, N, H, W, n_cls).to(dev)
    pred, hist = ops.argmax_confusion_grouped(logits, label, groups, 6, H, W, align_corners=align)
    # accumulation
    pred2, hist2 = ops.argmax_confusion_grouped(logits, label, groups, 6, H, W, hist=hist.clone(), align_corners=align)
    assert torch.equal(hist2, 2 * hist) and torch.equal(pred2, pred)
    # ids outside [0, n_groups) in a device tensor: the frame is labelled and counted nowhere; a guard group on each side stays zero
    ids = torch.tensor([3, 6, 0, -1, 5, 1 << 20, -(1 << 20)], dtype=torch.int32, device=dev)
    guarded = torch.zeros((8, n_cls, n_cls), dtype=torch.int64, device=dev)
    pred3, hist3 = ops.argmax_confusion_grouped(logits, label, ids, 6, H, W, hist=guarded[1:7], align_corners=align)
    assert torch.equal(pred3, pred)
    assert int(guarded[0].abs().sum()) == 0 and int(guarded[7].abs().sum()) == 0
    want = torch.zeros_like(hist)
    for n, g in enumerate(ids.tolist()):
        if 0 <= g < 6:
            want[g] += ops.argmax_confusion(logits[n:n + 1], label[n:n + 1], H, W, align_corners=align)[1]
    assert torch.equal(guarded[1:7], want) and hist3.data_ptr() == guarded[1:7].data_ptr()
    # want_pred=False: the histogram alone
    none, hist4 = ops.argmax_confusion_grouped(logits, label, groups, 6, H, W, want_pred=False, align_corners=align)
    assert none is None and torch.equal(hist4, hist)
    # label=None: the labels alone
    pred5, hist5 = ops.argmax_confusion_grouped(logits, None, groups, 6, H, W, align_corners=align)
    assert hist5 is None and torch.equal(pred5, pred)


def test_grouped_ties_and_nan(dev):
    """The NaN and tie cases of test_argmax_ties_and_nan, split over two groups (frame 0 -> group 1, frame 1 -> group 0)."""
    from arseg_amd import ops

    logits = torch.zeros(2, 5, 2, 4)
    logits[0, :, 0, 0] = torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0])                 # three-way tie -> 1
    logits[0, :, 0, 1] = torch.tensor([0.0, float("nan"), 9.0, float("nan"), 1.0])   # first NaN -> 1
    logits[0, :, 0, 2] = torch.tensor([-1.0, -2.0, -0.5, -0.5, -3.0])             # tie of negatives -> 2
    logits[1, :, 0, 3] = torch.tensor([float("-inf")] * 5)                        # all -inf -> 0
    logits[1, :, 1, 0] = torch.tensor([float("inf"), 1.0, float("inf"), 0.0, 0.0])   # tie of +inf -> 0
    logits[1, :, 1, 1] = torch.tensor([0.0, 0.0, float("nan"), float("inf"), float("nan")])   # NaN beats +inf -> 2
    want = torch.argmax(logits, dim=1)
    label = torch.zeros(2, 2, 4, dtype=torch.int64)
    got, hist = ops.argmax_confusion_grouped(logits.to(dev), label.to(dev), [1, 0], 2, 2, 4)
    assert torch.equal(got.cpu().long(), want)
    assert torch.equal(got, ops.argmax_confusion(logits.to(dev), None, 2, 4)[0])
    assert torch.equal(hist.cpu()[1, 0], torch.bincount(want[0].flatten(), minlength=5))
    assert torch.equal(hist.cpu()[0, 0], torch.bincount(want[1].flatten(), minlength=5))
    assert int(hist.sum()) == 16


# ---------------------------------------------------------------------------------------------- evaluators
def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _g7_samples(golden, kind):
    """The G7 sample and seeded variants of it, tagged d = 1, 4, 11 (two each), and two keyframe samples.  The distance is a tag to the
    evaluator; the variants only make the groups' histograms differ."""
    g = golden(f"g7_alter_{kind}")
    img, ref, label, flow = t(g["img"]), t(g["ref"]), t(g["label"]), t(g["mvq"]).double() / 4
    rng = torch.Generator().manual_seed(21)
    by_d = {}
    for i, d in enumerate((1, 1, 4, 4, 11, 11)):
        noise = 0.05 * torch.randn(img.shape, generator=rng)
        by_d.setdefault(d, []).append((img + noise, torch.roll(label, shifts=(i, 2 * i), dims=(1, 2)), None, ref, flow * (1.0 + 0.25 * i)))
    keys = [(ref, label, None), (torch.roll(ref, 3, dims=3), torch.roll(label, 3, dims=2), None)]
    return by_d, keys


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_eval_by_distance_equals_per_distance_evaluators(dev, golden, manifest, kind):
    from arseg_amd import evaluation as ev

    mk = _psp if kind == "psp" else _bise
    hr, lr = mk(manifest, dev, False), mk(manifest, dev, True)
    by_d, keys = _g7_samples(golden, kind)
    loader = [by_d[4][0] + (4,), keys[0], by_d[11][0] + (torch.tensor([11]),), by_d[1][0] + (1,), by_d[1][1] + (torch.tensor([1]),), keys[1],
              by_d[4][1] + (4,), by_d[11][1] + (11,)]                                # distances mixed
    with torch.no_grad():
        table = ev.EvalByDistance(scale=0.5, gop=12)(hr, torch.nn.DataParallel(lr), loader, 12)
        assert isinstance(table, ev.EvalTable) and tuple(table.hist.shape) == (12, 12, 12) and len(table.miou) == 12
        for d in (1, 4, 11):
            want_h = ev.EvalAlterRes(scale=0.5)._run(hr, lr, by_d[d], 12)
            want = ev.EvalAlterRes(scale=0.5)(hr, lr, by_d[d], 12)
            print(f"\n[{kind}] d={d}: mIoU {table.miou[d]!r} (EvalAlterRes {want!r}), {int(want_h.sum())} pixels")
            assert int(want_h.sum()) > 0 and torch.equal(table.hist[d], want_h)
            assert _same(table.miou[d], want)
        want_h = ev.EvalConstRes(scale=1.0)._run(hr, keys, 12)
        want = ev.EvalConstRes(scale=1.0)(hr, keys, 12)
        print(f"[{kind}] d=0: mIoU {table.miou[0]!r} (EvalConstRes {want!r})")
        assert int(want_h.sum()) > 0 and torch.equal(table.hist[0], want_h)
        assert _same(table.miou[0], want)
        for d in set(range(12)) - {0, 1, 4, 11}:
            assert int(table.hist[d].sum()) == 0 and math.isnan(table.miou[d])
        every = [s for d in (1, 4, 11) for s in by_d[d]]
        pooled = ev.EvalAlterRes(scale=0.5)(hr, lr, every, 12)
        assert _same(table.pooled(range(1, 12)), pooled)
        assert _same(ev.EvalTable(table.hist[1:]).pooled(), pooled)
        # two distances in one batch: the same counts as EvalAlterRes' on that batch, split by frame
        a, b = by_d[1][0], by_d[11][1]
        both = tuple(torch.cat([x, y]) for x, y in zip(a[:2], b[:2])) + (None,) + tuple(torch.cat([x, y]) for x, y in zip(a[3:], b[3:]))
        mixed = ev.EvalByDistance(scale=0.5, gop=12)(hr, lr, [both + (torch.tensor([1, 11]),)], 12)
        assert torch.equal(mixed.hist.sum(0), ev.EvalAlterRes(scale=0.5)._run(hr, lr, [both], 12))
        assert int(mixed.hist[1].sum()) == int((a[1] != 255).sum()) and int(mixed.hist[11].sum()) == int((b[1] != 255).sum())
        with pytest.raises(ValueError):
            ev.EvalByDistance(scale=0.5, gop=12)(hr, lr, [a + (12,)], 12)
        with pytest.raises(ValueError):
            ev.EvalByDistance(scale=0.5, gop=12)(hr, lr, [a], 12)                # EvalAlterRes' 5-tuple: no distance


def test_eval_by_distance_keyframe_cache(dev, golden, manifest):
    from arseg_amd import evaluation as ev

    hr, lr = _psp(manifest, dev, False), _psp(manifest, dev, True)
    by_d, keys = _g7_samples(golden, "psp")
    loader = [keys[0]] + [s + (d,) for d in (1, 4, 11) for s in by_d[d]]       # GOP ordered: one reference frame for all six
    with torch.no_grad():
        plain, cached = ev.EvalByDistance(scale=0.5), ev.EvalByDistance(scale=0.5, cache_keyframe=True)
        t0, t1 = plain(hr, lr, loader, 12), cached(hr, lr, loader, 12)
        ar = ev.EvalAlterRes(scale=0.5, cache_keyframe=True)
        ar(hr, lr, [s[:5] for s in loader[1:]], 12)
    assert torch.equal(t0.hist, t1.hist)
    assert plain.hr_forwards == 6 and cached.hr_forwards == ar.hr_forwards == 1


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_batch_pred_with_groups(dev, manifest, kind):
    """alter_res_batch_pred on a GOP-12 batch with groups = the distances 1 .. 11: the resized / identity tail (PSPNet) and the fused x8
    one (BiSeNet)."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth

    mk = _psp if kind == "psp" else _bise
    hr, lr = mk(manifest, dev, False), mk(manifest, dev, True)
    H, W = (48, 64) if kind == "psp" else (128, 256)
    clip = synth.make_clip(6, H, W, gop=12)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    label = labels(168, 11, H, W, 12).to(dev)
    with torch.no_grad():
        ref_p = ops.to_nhwc(hr(frames[0:1])[-1])[0]
        pred_u, hist_u = ev.alter_res_batch_pred(lr, [ref_p] * 11, frames[1:12], mvs[1:12], 0.5, labels=label)
        pred_g, hist_g = ev.alter_res_batch_pred(lr, [ref_p] * 11, frames[1:12], mvs[1:12], 0.5, labels=label, groups=list(range(1, 12)), n_groups=12)
        assert tuple(hist_g.shape) == (12, 12, 12) and tuple(hist_u.shape) == (12, 12)
        assert torch.equal(pred_g, pred_u)
        assert torch.equal(hist_g.sum(0), hist_u) and int(hist_g[0].sum()) == 0
        flips = 0
        for d in range(1, 12):
            pred_1, hist_1 = ev.alter_res_batch_pred(lr, [ref_p], frames[d:d + 1], mvs[d:d + 1], 0.5, labels=label[d - 1:d])
            flips += int((pred_1[0] != pred_g[d - 1]).sum())
            assert torch.equal(hist_g[d], hist_1), f"d={d}: {int((pred_1[0] != pred_g[d - 1]).sum())} labels differ between the batch and the one-frame call"
        print(f"\n[{kind}] labels that differ between the batched and the one-frame calls: {flips}")
        with pytest.raises(ValueError):
            ev.alter_res_batch_pred(lr, [ref_p] * 11, frames[1:12], mvs[1:12], 0.5, labels=label, groups=list(range(1, 12)))
