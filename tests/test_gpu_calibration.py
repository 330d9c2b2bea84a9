"""GPU checks of the calibration counts (csrc/calibration.hip, arseg_calibration_fwd; ops.calibration).  The yardstick is the code that was
there before: the table torch builds (one bincount on the key (group, k, q, right), tests/calibration_oracle.py from_planes) from the two
planes of egress.confidence(..., labels_out=...) on the same arguments, which tests/test_gpu_confidence.py holds to the float64 oracle.
Every comparison is of integers and exact: zero differences."""
import numpy as np
import pytest
import torch

import calibration_oracle as co
import confidence_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _planes_table(logits, label, H, W, groups, n_groups, kind, align, ignore=255):
    from arseg_amd import egress

    conf, labels, _ = egress.confidence(logits, H, W, kind=kind, labels_out=True, align_corners=align)
    return co.from_planes(conf, labels, label, groups, n_groups, logits.shape[1], ignore)


def _differ(got, want, what):
    d = int((got != want).sum())
    print(f"\n{what}: {d} differing counters of {want.numel()}, {int(want[..., 0].sum())} counting pixels, {int((want[..., 0] > 0).sum())} bins in use")
    return d


@pytest.fixture(scope="module")
def seeded(dev):
    """case name -> (logits, labels) on the device, made once per module."""
    cache = {}

    def get(case):
        if case[0] not in cache:
            cache[case[0]] = (torch.from_numpy(oracle.case_logits(case)).to(dev), torch.from_numpy(co.case_labels(case)).to(dev))
        return cache[case[0]]
    return get


@pytest.mark.parametrize("kind", oracle.KINDS)
@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_table_equals_the_planes_on_every_route(dev, seeded, case, kind):
    """All seven cases, both kinds, two groups: the table is the planes' table, and summed over the codes it is the columns and the diagonal
    of the grouped tail's confusion matrices."""
    from arseg_amd import ops

    name, _, N, n_cls, h, w, H, W, align = case
    logits, label = seeded(case)
    groups = co.case_groups(case)
    cal = ops.calibration(logits, label, H, W, groups=groups, n_groups=2, kind=kind, align_corners=align)
    assert cal.dtype == torch.int64 and tuple(cal.shape) == (2, n_cls, 256, 2)
    want = _planes_table(logits, label, H, W, groups, 2, kind, align)
    assert _differ(cal, want, f"{name} {kind}") == 0
    assert int((want.sum(dim=(0, 1))[:, 0] > 0).sum()) >= 128                        # the comparison is over most of the codes
    _, hist = ops.argmax_confusion_grouped(logits, label, groups, 2, H, W, want_pred=False, align_corners=align)
    assert torch.equal(cal[..., 0].sum(dim=2), hist.sum(dim=1))
    assert torch.equal(cal[..., 1].sum(dim=2), hist.diagonal(dim1=1, dim2=2))


@pytest.mark.parametrize("case", [oracle.CASES[0], oracle.CASES[4]], ids=[oracle.CASE_IDS[0], oracle.CASE_IDS[4]])
def test_groups(dev, seeded, case):
    """Group ids on the device are taken as they are: -1 and n_groups count nowhere; None is one group of all frames; another ignore label."""
    from arseg_amd import ops

    name, _, N, n_cls, h, w, H, W, align = case
    logits, label = seeded(case)
    for ids in ([-1] + [1] * (N - 1), [0] * (N - 1) + [2], [2, -1, 5][:N]):
        grp = torch.tensor(ids, dtype=torch.int32, device=dev)
        cal = ops.calibration(logits, label, H, W, groups=grp, n_groups=2, align_corners=align)
        want = _planes_table(logits, label, H, W, ids, 2, "top1", align)
        assert _differ(cal, want, f"{name} groups {ids}") == 0
        frames = [n for n, g in enumerate(ids) if 0 <= g < 2]
        counting = (label >= 0) & (label < n_cls) & (label != 255)
        assert int(cal[..., 0].sum()) == int(counting[frames].sum()) if frames else int(cal.sum()) == 0
    one = ops.calibration(logits, label, H, W, align_corners=align)
    assert tuple(one.shape) == (1, n_cls, 256, 2) and _differ(one, _planes_table(logits, label, H, W, None, 1, "top1", align), f"{name} one group") == 0
    assert torch.equal(one[0], ops.calibration(logits, label, H, W, groups=[1, 0, 1][:N], n_groups=2, align_corners=align).sum(dim=0))
    other = ops.calibration(logits, label, H, W, ignore_label=3, align_corners=align)
    assert _differ(other, _planes_table(logits, label, H, W, None, 1, "top1", align, ignore=3), f"{name} ignore 3") == 0
    assert int(other[..., 0].sum()) == int(((label >= 0) & (label < n_cls) & (label != 3)).sum())


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_ignored_labels_and_one_class(dev, seeded, case):
    from arseg_amd import ops

    name, seed, N, n_cls, h, w, H, W, align = case
    logits, label = seeded(case)
    for fill in (255, -1, n_cls, 2 ** 40):
        assert int(ops.calibration(logits, torch.full_like(label, fill), H, W, align_corners=align).abs().sum()) == 0
    # n_cls == 1: every pixel is class 0 with code 255; right where the label is 0; labels 1.. are outside the classes
    single = torch.from_numpy(oracle.make_logits(seed + 50, N, 1, h, w)).to(dev)
    lab = label % 3
    for kind in oracle.KINDS:
        cal = ops.calibration(single, lab, H, W, kind=kind, align_corners=align)
        zeros = int((lab == 0).sum())
        assert tuple(cal.shape) == (1, 1, 256, 2) and cal[0, 0, 255].tolist() == [zeros, zeros] and int(cal.sum()) == 2 * zeros and zeros > 0


@pytest.mark.parametrize("kind", oracle.KINDS)
@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_ties_nans_and_infinities(dev, seeded, case, kind):
    """confidence_oracle.plant_specials: the table equals the planes' with the plants in; on the same-size route the three pixels whose
    confidence is NaN are exactly what row q = 0 gains, at the classes the label rule gives them (the NaN's class, the +inf's class, 0)."""
    from arseg_amd import egress, ops

    name, _, N, n_cls, h, w, H, W, align = case
    x = oracle.case_logits(case)
    where = oracle.plant_specials(x)
    logits = torch.from_numpy(x).to(dev)
    conf, labels, _ = egress.confidence(logits, H, W, kind=kind, labels_out=True, align_corners=align)
    label = labels.long()                                                            # every pixel counts and is right
    cal = ops.calibration(logits, label, H, W, kind=kind, align_corners=align)
    assert _differ(cal, co.from_planes(conf, labels, label, None, 1, n_cls), f"{name} {kind} with plants") == 0
    assert torch.equal(cal[..., 0], cal[..., 1]) and int(cal[..., 0].sum()) == N * H * W
    assert int(cal[0, :, 0, 0].sum()) == int((conf == 0).sum()) >= len(where)
    if name == "same":
        clean = ops.calibration(torch.from_numpy(oracle.case_logits(case)).to(dev), label, H, W, kind=kind, align_corners=align)
        gained = cal[0, :, 0, 0] - clean[0, :, 0, 0]
        if kind == "top1":                                                           # (the margin of the planted two-way ties is 0 as well)
            assert gained.tolist() == [1 if k == 0 else 1 if k == 2 else 1 if k == 5 else 0 for k in range(n_cls)]
        for n, yy, xx in where:
            assert int(conf[n, yy, xx]) == 0
        assert [int(labels[n, yy, xx]) for n, yy, xx in where] == [5, 2, 0]


def _hot(N, n_cls, h, w, H, W, board):
    """Logits with one class 30 above the rest at every pixel: class 3 everywhere, or (``board``) classes 3 and 7 in a checkerboard of
    cells of 4 output pixels (of low-resolution pixels on the x8 frame).  Labels: the class on three rows of four, another elsewhere."""
    x = np.zeros((N, n_cls, h, w), np.float32)
    cell = 4 if (h, w) == (H, W) else 1
    yy, xx = np.mgrid[:h, :w]
    second = ((yy // cell + xx // cell) % 2 == 1) if board else np.zeros((h, w), bool)
    x[:, 3][:, ~second] = 30.0
    x[:, 7][:, second] = 30.0
    return x


@pytest.mark.parametrize("board", [False, True], ids=["one-class", "checkerboard"])
@pytest.mark.parametrize("shape", [(2, 12, 64, 96, 64, 96, True), (3, 19, 9, 11, 72, 88, False)], ids=["same", "x8"])
def test_hot_bin(dev, shape, board):
    """Saturated logits: every pixel has code 255, so a wave's 64 (x S) pixels fall into one or two bins -- the path the wave-level
    aggregation exists for.  Against the planes, and against the count of the pixels directly."""
    from arseg_amd import egress, ops

    N, n_cls, h, w, H, W, align = shape
    logits = torch.from_numpy(_hot(N, n_cls, h, w, H, W, board)).to(dev)
    conf, labels, _ = egress.confidence(logits, H, W, labels_out=True, align_corners=align)
    if not board or (h, w) == (H, W):
        assert bool((conf == 255).all())                                             # (between two cells of the x8 board the blend is a tie)
    g = np.random.Generator(np.random.PCG64(5))
    label = torch.where(torch.from_numpy(g.random((N, H, W)) < 0.75).to(dev), labels.long(), torch.full((N, H, W), 255 if board else 5, device=dev))
    groups = [1, 0, 1][:N]
    for kind in oracle.KINDS:
        cal = ops.calibration(logits, label, H, W, groups=groups, n_groups=2, kind=kind, align_corners=align)
        assert _differ(cal, _planes_table(logits, label, H, W, groups, 2, kind, align), f"hot {shape} board={board} {kind}") == 0
    cal = ops.calibration(logits, label, H, W, groups=groups, n_groups=2, align_corners=align)
    for k in (3, 7):
        for grp in (0, 1):
            frames = [n for n in range(N) if groups[n] == grp]
            at = (labels[frames] == k) & (conf[frames] == 255)
            assert cal[grp, k, 255].tolist() == [int((at & (label[frames] != 255)).sum()), int((at & (label[frames] == k)).sum())]
    if not board:
        assert int(cal[:, 3, 255, 0].sum()) == N * H * W == int(cal[..., 0].sum()) and int(cal[..., 1].sum()) == int((label == 3).sum())


@pytest.mark.parametrize("case", oracle.CASES[:5], ids=oracle.CASE_IDS[:5])
def test_accumulation_and_repeatability(dev, seeded, case):
    from arseg_amd import ops

    _, _, N, n_cls, h, w, H, W, align = case
    logits, label = seeded(case)
    groups = co.case_groups(case)
    once = ops.calibration(logits, label, H, W, groups=groups, n_groups=2, align_corners=align)
    cal = once.clone()
    back = ops.calibration(logits, label, H, W, groups=groups, n_groups=2, cal=cal, align_corners=align)
    assert back is cal and torch.equal(cal, 2 * once)
    assert torch.equal(ops.calibration(logits, label, H, W, groups=groups, n_groups=2, align_corners=align), once)
    from arseg_amd import _lib
    for bad in (torch.zeros((2, n_cls, 256), dtype=torch.int64, device=dev), torch.zeros((2, n_cls, 256, 2), dtype=torch.int32, device=dev)):
        with pytest.raises(_lib.ArsegError):
            ops.calibration(logits, label, H, W, groups=groups, n_groups=2, cal=bad, align_corners=align)
    with pytest.raises(_lib.ArsegError):
        ops.calibration(logits, label[:, :-1], H, W, align_corners=align)
    with pytest.raises(_lib.ArsegError):
        ops.calibration(logits, label.int(), H, W, align_corners=align)


def test_calibration_in_one_graph(dev):
    """ops.calibration(..., cal=) captured once; logits, labels and group ids are refilled in place; each of two replays equals the eager
    result for its own inputs (the table is zeroed before a replay: it is accumulated into)."""
    from arseg_amd import ops

    case = oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align = case
    static = torch.from_numpy(oracle.case_logits(case)).to(dev)
    label = torch.from_numpy(co.case_labels(case)).to(dev)
    grp = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    cal = torch.zeros((2, n_cls, 256, 2), dtype=torch.int64, device=dev)
    ops.calibration(static, label, H, W, groups=grp, n_groups=2, cal=cal, kind="margin", align_corners=align)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.calibration(static, label, H, W, groups=grp, n_groups=2, cal=cal, kind="margin", align_corners=align)
    for s, ids in ((seed + 60, [0, 0, 1]), (seed + 61, [1, 2, 0])):
        fresh = torch.from_numpy(oracle.make_logits(s, N, n_cls, h, w)).to(dev)
        lab = torch.roll(label, s, dims=2)
        static.copy_(fresh)
        label.copy_(lab)
        grp.copy_(torch.tensor(ids, dtype=torch.int32))
        cal.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _differ(cal, _planes_table(fresh, label, H, W, ids, 2, "margin", align), f"replay {s}") == 0
        assert int(cal.sum()) > 0


def test_full_size_x8(dev):
    """One 1024x2048 frame, 19 classes, x8 run route -- as many workgroups as the caps allow, several classes per workgroup."""
    from arseg_amd import ops

    H, W, n_cls = 1024, 2048, 19
    logits = torch.from_numpy(oracle.make_logits(171, 1, n_cls, H // 8, W // 8)).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=False)[0].long()
    g = torch.Generator(device="cpu").manual_seed(172)
    r = torch.rand((1, H, W), generator=g).to(dev)
    label = torch.where(r < 0.7, pred, (pred + 1 + (r * 1000).long() % (n_cls - 1)) % n_cls)
    label[r > 0.95] = 255
    cal = ops.calibration(logits, label, H, W, align_corners=False)
    assert _differ(cal, _planes_table(logits, label, H, W, None, 1, "top1", False), "full size x8") == 0
    assert int(cal[..., 0].sum()) == int((label != 255).sum()) and int(cal[..., 1].sum()) == int((label == pred).sum())


@pytest.mark.parametrize("route", ["same", "x8"])
def test_a_workgroup_flushes_before_a_half_of_its_counters_is_full(dev, route):
    """So many frames that the launch caps (1024 / 4096 workgroups) leave one workgroup per frame, and frames of more than 65535 pixels
    that all fall into one bin (n_cls == 1: class 0, code 255): a 16-bit half of the LDS word would wrap before the end of the frame, so the
    workgroup has to flush inside its loop.  The smallest such input: these counts are the only ones that reach that path."""
    from arseg_amd import ops

    N, h, w, H, W, align = (600, 256, 260, 256, 260, True) if route == "same" else (2100, 8, 135, 64, 1080, False)
    assert N > (1024 if route == "same" else 4096) // 2 and H * W > 65535
    logits = torch.zeros((N, 1, h, w), device=dev)
    label = torch.zeros((N, H, W), dtype=torch.int64, device=dev)
    label[:, 3, :] = 255
    label[:, :, 5] = 1                                                               # outside the one class
    grp = (torch.arange(N, device=dev) % 3).to(torch.int32)
    cal = ops.calibration(logits, label, H, W, groups=grp, n_groups=3, align_corners=align)
    per_frame = (H - 1) * (W - 1)
    want = [per_frame * int((grp == g).sum()) for g in range(3)]
    assert cal[:, 0, 255, 0].tolist() == want and cal[:, 0, 255, 1].tolist() == want and int(cal.sum()) == 2 * sum(want)


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_alter_res_batch_calibration(dev, manifest, kind):
    """The small PSPNet (fp32) and BiSeNet (bf16, fused x8 tail) of tests/test_gpu_models.py: alter_res_batch_calibration is the same phase 1
    / phase 2 calls and route decision, made here by hand, followed by the planes' table; its hist is alter_res_batch_pred's."""
    import test_gpu_ingest_formats as tf          # its _nets wraps test_gpu_models' _psp / _bise (+ bf16 storage)
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from test_gpu_eval_grouped import labels as random_labels

    hr, lr = tf._nets(manifest, dev, kind)
    H, W = (64, 96) if kind == "psp" else (128, 256)
    clip = synth.make_clip(9, H, W, gop=4, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    groups = [1, 2, 3]
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * 3
        net = ev._unwrap(lr)
        h, w = ev._downscale_hw(H, W, 0.5)
        feat = net.phase1_nhwc4(ops.ingest_input(frames[1:4], h, w, net.storage_dtype), aux=ops.config.aux_outputs)[-1]
        if kind == "bise":
            lo, _ = net.phase2_warp(feat, list(refs), mvs[1:4], upsample=False)
            assert (8 * lo.shape[-2], 8 * lo.shape[-1]) == (H, W)
        else:
            lo, _ = net.phase2_warp(feat, list(refs), mvs[1:4])
        n_cls = lo.shape[1]
        pred, _ = ev.alter_res_batch_pred(lr, refs, frames[1:4], mvs[1:4], 0.5)
        label = random_labels(168, 3, H, W, n_cls).to(dev)
        label = torch.where(label % 2 == 0, pred.long(), label)                      # about half the pixels right
        label[0, :2, :3] = 255
        cal, hist = ev.alter_res_batch_calibration(lr, refs, frames[1:4], mvs[1:4], label, 0.5, groups=groups, n_groups=4, hist=True)
        assert tuple(cal.shape) == (4, n_cls, 256, 2)
        assert _differ(cal, _planes_table(lo.contiguous(), label, H, W, groups, 4, "top1", kind != "bise"), f"alter_res_batch_calibration {kind}") == 0
        _, hist_p = ev.alter_res_batch_pred(lr, refs, frames[1:4], mvs[1:4], 0.5, labels=label, groups=groups, n_groups=4)
        assert torch.equal(hist, hist_p) and int(cal[0].sum()) == 0 and int(cal[..., 0].sum()) == int((label != 255).sum())
        assert torch.equal(cal[..., 0].sum(dim=2), hist.sum(dim=1)) and torch.equal(cal[..., 1].sum(dim=2), hist.diagonal(dim1=1, dim2=2))
        assert int(cal[..., 1].sum()) == int((label == pred).sum())
        again, none = ev.alter_res_batch_calibration(lr, refs, frames[1:4], mvs[1:4], label, 0.5, cal=cal, groups=groups, n_groups=4, kind="top1")
        assert again is cal and none is None and torch.equal(cal[..., 0].sum(dim=2), 2 * hist.sum(dim=1))
        alone, _ = ev.alter_res_batch_calibration(lr, refs, frames[1:4], mvs[1:4], label, 0.5, kind="margin")          # one group, the margin
        assert tuple(alone.shape) == (1, n_cls, 256, 2)
        assert _differ(alone, _planes_table(lo.contiguous(), label, H, W, None, 1, "margin", kind != "bise"), f"one group, margin, {kind}") == 0


def test_eval_by_calibration(dev, golden, manifest):
    """EvalByCalibration on the small PSPNet and a loader of four of test_gpu_eval_grouped's samples: the evaluator's own logits, sample by
    sample, through the confidence planes give its table; summed over the codes the table is the columns and the diagonal of
    EvalByDistance's histograms on the same loader.  (The evaluator is held to its own logits, as EvalByContour's test holds it, not to
    alter_res_batch_calibration's: the fast path's logits agree with the evaluator's to a tolerance only and its labels differ at
    near-ties -- test_gpu_models.py::test_eval_alter_res_golden counts them -- so integer counts from the two paths are not comparable
    exactly.  test_alter_res_batch_calibration holds the fast path to its own logits the same way.)"""
    from arseg_amd import evaluation as ev
    from test_gpu_eval_grouped import _g7_samples
    from test_gpu_models import _psp

    hr, lr = _psp(manifest, dev, False), _psp(manifest, dev, True)
    by_d, keys = _g7_samples(golden, "psp")
    loader = [by_d[4][0] + (4,), keys[0], by_d[11][0] + (torch.tensor([11]),), by_d[1][0] + (1,)]
    with torch.no_grad():
        for kind in ("top1", "margin"):
            table = ev.EvalByCalibration(scale=0.5, gop=12, kind=kind)(hr, torch.nn.DataParallel(lr), loader, 12)
            assert isinstance(table, ev.CalibrationTable) and table.kind == kind and tuple(table.cal.shape) == (12, 12, 256, 2)
            again = torch.zeros_like(table.cal)
            e = ev.EvalByDistance(scale=0.5, gop=12)
            cache = [None, None]
            for sample in loader:
                label = sample[1].to(dev)
                if len(sample) == 3:
                    out, groups = hr(sample[0].to(dev))[0], [0] * label.shape[0]
                else:
                    out, groups = e._logits(hr, lr, sample[0], sample[3], sample[4], cache), e._groups(sample[5], label.shape[0])
                again += _planes_table(out.contiguous(), label, label.shape[-2], label.shape[-1], groups, 12, kind, True)
            assert _differ(table.cal, again, f"EvalByCalibration {kind}") == 0
            assert int(table.cal[[0, 1, 4, 11]].sum()) > 0 and int(table.cal[[2, 3, 5]].sum()) == 0
        hist = ev.EvalByDistance(scale=0.5, gop=12)(hr, lr, loader, 12).hist
        assert torch.equal(table.cal[..., 0].sum(dim=2), hist.sum(dim=1)) and torch.equal(table.cal[..., 1].sum(dim=2), hist.diagonal(dim1=1, dim2=2))
        acc = table.accuracy()
        assert tuple(acc.shape) == (12,) and acc[[0, 1, 4, 11]].isnan().sum() == 0 and acc[[2, 3, 5]].isnan().all()
        assert tuple(table.ece().shape) == (12,) and tuple(table.pooled().ece().shape) == (1,)
