"""GPU checks of the keyframe prior (csrc/stabilise.hip, arseg_segment_stabilise_fwd; arseg_amd.egress.stabilise): the label plane, the hold
plane and the statistics of one launch against the CPU oracle under the comparison rule of tests/stabilise_oracle.py -- k* from the
EXISTING evaluator tail (ops.argmax_confusion); everything exact on the same-size route; on the resized routes every label k* or c_ref, the
HELD / OWN decision the oracle's outside a band of 2e-5 around beta, at most 0.5 % band pixels -- and in every case the statistics exactly
what the two planes of the same launch say."""
import numpy as np
import pytest
import torch

import stabilise_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0xA5
NS = oracle.ST_NSTATS
ROUTES = oracle.CASES[:5]
ROUTE_IDS = oracle.CASE_IDS[:5]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs(dev):
    """case -> its seeded input on the device, the tail's pred and the oracle's answer for it (both gates on, the median thresholds),
    computed once per module and not modified: dict(logits, ref, mv, link, conf, beta (device tensors), np (the host arrays and the class
    values), pred (numpy int64), o (the oracle's dict))."""
    from arseg_amd import ops

    cache = {}

    def get(case):
        if case[0] not in cache:
            b = oracle.build(case)
            logits = torch.from_numpy(b["logits"]).to(dev)
            pred = ops.argmax_confusion(logits, None, case[6], case[7], align_corners=case[8])[0].cpu().numpy().astype(np.int64)
            b, o = oracle.solve(case, b, pred)
            t = {k: torch.from_numpy(b[k]).to(dev) for k in ("ref", "mv", "link", "conf", "beta")}
            cache[case[0]] = dict(t, logits=logits, np=b, pred=pred, o=o)
        return cache[case[0]]
    return get


def _np(*ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _run(i, case, **kw):
    """egress.stabilise on a case's input with both gates on unless ``kw`` says otherwise -> (labels, hold, stats) tensors."""
    from arseg_amd import egress

    args = dict(link=i["link"], link_mask=oracle.LINK_MASK, ref_conf=i["conf"], ref_low=oracle.REF_LOW, hold_out=True, align_corners=case[8])
    args.update(kw)
    ref, mv, beta = args.pop("ref", i["ref"]), args.pop("mv", i["mv"]), args.pop("bonus", i["beta"])
    return egress.stabilise(args.pop("logits", i["logits"]), ref, mv, case[6], case[7], beta, **args)


def _want(i, **kw):
    """The oracle on a case's class values and the tail's pred, both gates on unless ``kw`` says otherwise."""
    b = i["np"]
    args = dict(ref=b["ref"], mv_q=b["mv"], beta=b["beta"], link=b["link"], link_mask=oracle.LINK_MASK, ref_conf=b["conf"], ref_low=oracle.REF_LOW)
    args.update(kw)
    return oracle.stabilise(b["values"], kstar=i["pred"], **args)


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
def test_labels_hold_and_stats_on_every_route(dev, inputs, case):
    """One launch writes labels8, hold8 and stats on every route, with 12, 19 and 32 classes, shared and per-frame reference planes, both
    gates on and the median thresholds: against the oracle under the comparison rule."""
    name, _, N, n_cls, h, w, H, W, align, shared = case
    i = inputs(case)
    labels, hold, stats = _run(i, case)
    assert labels.dtype == hold.dtype == torch.uint8 and tuple(labels.shape) == tuple(hold.shape) == (N, H, W) and tuple(stats.shape) == (N, NS)
    flipped = oracle.compare(i["o"], *_np(labels, hold, stats), n_cls)
    s = stats.cpu().numpy()
    print(f"\n{name}: outcomes per frame {s[:, :7].tolist()}; {int(i['o']['band'].sum())} band pixels of {N * H * W}, {flipped} decided the other way")
    assert (s[:, :7].sum(axis=1) == H * W).all() and (s[:, oracle.HELD] > 0).all() and (s[:, oracle.OWN] > 0).all()
    if (h, w) == (H, W):
        assert flipped == 0 and np.array_equal(s, i["o"]["stats"])


@pytest.mark.parametrize("case", [oracle.CASES[0], oracle.CASES[1], oracle.CASES[4]], ids=lambda c: c[0])
def test_one_class(dev, inputs, case):
    """n_cls == 1 on the three routes with an infinite threshold: every label is 0, nothing is ever HELD or OWN."""
    _, seed, N, _, h, w, H, W, align, _ = case
    i = inputs(case)
    g = np.random.Generator(np.random.PCG64(seed + 50))
    logits = g.standard_normal((N, 1, h, w)).astype(np.float32)
    ref_np = np.where(i["np"]["ref"] == 255, 255, 0).astype(np.uint8)
    beta = np.full(N, np.inf, dtype=np.float32)
    labels, hold, stats = _run(i, case, logits=torch.from_numpy(logits).to(dev), ref=torch.from_numpy(ref_np).to(dev), bonus=torch.from_numpy(beta).to(dev))
    want = oracle.stabilise(oracle.class_values(logits, H, W, align), ref_np, i["np"]["mv"], beta, i["np"]["link"], oracle.LINK_MASK, i["np"]["conf"],
                            oracle.REF_LOW, kstar=np.zeros((N, H, W), dtype=np.int64))
    assert oracle.compare(want, *_np(labels, hold, stats), 1) == 0 and not want["band"].any()
    s = stats.cpu().numpy()
    assert bool((labels == 0).all()) and not s[:, oracle.HELD].any() and not s[:, oracle.OWN].any() and (s[:, oracle.AGREE] > 0).all()
    assert np.array_equal(s, want["stats"]) and (s[:, :4] > 0).all()


@pytest.mark.parametrize("case", ROUTES, ids=ROUTE_IDS)
def test_equivalences(dev, inputs, case):
    """beta = 0 (and below) gives egress.labels8 bit for bit; the link gate off: link_mask = 0 equals link=None; ref_conf=None equals
    ref_low = 0; and each gate moves pixels when it is on."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    plain = egress.labels8(i["logits"], H, W, align_corners=align)
    for beta in (0.0, -1.5):
        labels, hold, stats = _run(i, case, bonus=beta)
        assert torch.equal(labels, plain) and not bool((hold == 255).any()) and not bool(stats[:, oracle.HELD].any())
        assert not bool(stats[:, oracle.INTO:].any())
    on = _run(i, case)
    a, b = _run(i, case, link_mask=0), _run(i, case, link=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not bool(a[2][:, oracle.UNLINKED].any()) and not torch.equal(a[1], on[1])
    a, b = _run(i, case, ref_low=0), _run(i, case, ref_conf=None, ref_low=77)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not bool(a[2][:, oracle.WEAK].any()) and not torch.equal(a[1], on[1])
    assert oracle.compare(_want(i, ref_conf=None), *_np(*a), n_cls) >= 0
    top = _run(i, case, ref_low=256)                                                     # every code is below 256: no pixel offers a prior
    assert not bool(top[2][:, oracle.AGREE:oracle.OWN + 1].any()) and torch.equal(top[0], plain) and bool((top[1] == 128).all())


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "linked"])
@pytest.mark.parametrize("case", ROUTES, ids=ROUTE_IDS)
def test_agreement_identity(dev, inputs, case, gated):
    """What the feature exists for: with the same link gate and ref_conf off, egress.consistency_of_planes on the stabilised planes finds
    exactly AGREE + HELD agreeing pixels, AGREE alone on the plain planes -- agreement along the chain can only rise -- and compares
    exactly AGREE + HELD + OWN pixels."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    link = dict(link=i["link"], link_mask=oracle.LINK_MASK) if gated else dict(link=None)
    labels, _, stats = _run(i, case, ref_conf=None, **link)
    plain = egress.labels8(i["logits"], H, W, align_corners=align)
    after = egress.consistency_of_planes(labels, i["ref"], i["mv"], n_cls, **(dict(link, unlinked=True) if gated else {}))[1]
    before = egress.consistency_of_planes(plain, i["ref"], i["mv"], n_cls, **(dict(link, unlinked=True) if gated else {}))[1]
    agree_after, agree_before = after[:, 67:99].sum(dim=1), before[:, 67:99].sum(dim=1)
    assert torch.equal(agree_after, stats[:, oracle.AGREE] + stats[:, oracle.HELD]) and torch.equal(agree_before, stats[:, oracle.AGREE])
    assert torch.equal(after[:, 0], stats[:, oracle.AGREE:oracle.OWN + 1].sum(dim=1)) and bool((agree_after > agree_before).all())


@pytest.mark.parametrize("case", [oracle.CASES[1], oracle.CASES[2]], ids=lambda c: c[0])
def test_shared_against_per_frame_reference_planes(dev, inputs, case):
    """Shared planes ([1,H,W], and [H,W]) give what N copies of them give as per-frame stacks, and a stack of different planes differs."""
    _, _, N, n_cls, h, w, H, W, align, shared = case
    assert shared
    i = inputs(case)
    want = _run(i, case)
    stack_r, stack_c = i["ref"].expand(N, H, W).contiguous(), i["conf"].expand(N, H, W).contiguous()
    for ref, conf in ((i["ref"][0], i["conf"][0]), (stack_r, stack_c), (i["ref"], stack_c), (stack_r, i["conf"])):
        assert all(torch.equal(x, y) for x, y in zip(_run(i, case, ref=ref, ref_conf=conf), want))
    rolled = stack_r.clone()
    rolled[1] = torch.roll(stack_r[1], shifts=(1, 2), dims=(0, 1))
    got = _run(i, case, ref=rolled)
    assert oracle.compare(_want(i, ref=rolled.cpu().numpy()), *_np(*got), n_cls) >= 0
    assert torch.equal(got[1][0], want[1][0]) and not torch.equal(got[1][1], want[1][1])


@pytest.mark.parametrize("case", ROUTES, ids=ROUTE_IDS)
def test_int16_corners_all_outside_all_void_and_all_unlinked(dev, inputs, case):
    """Vectors at the corners of int16 planted over the seeded field; frames whose every vector points off the frame (nothing is read from
    the reference), a reference of 255s, link planes with every pixel flagged: no prior anywhere, the labels are the plain ones."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    plain = egress.labels8(i["logits"], H, W, align_corners=align)
    mv = i["np"]["mv"].copy()
    corners = np.array([-32768, 32767, -32767, 32766, -32766, 0], dtype=np.int16)
    g = np.random.Generator(np.random.PCG64(case[1] + 7))
    mask = g.random((N, H, W)) < 0.3
    planted = g.choice(corners, (N, H, W, 2))
    planted[..., 0] = np.where(planted[..., 0] == 0, 32767, planted[..., 0])          # at least one component at a corner
    mv[mask] = planted[mask]
    got = _run(i, case, mv=torch.from_numpy(mv).to(dev))
    want = _want(i, mv_q=mv)
    assert oracle.compare(want, *_np(*got), n_cls) >= 0 and (want["stats"][:, oracle.OUTSIDE] >= (mask & (want["pre"] != -1)).sum(axis=(1, 2))).all()

    out = np.empty_like(mv)
    out[..., 0], out[..., 1] = 4 * W, -4 * H
    out[0, :, :, 1] = 0                                                                # frame 0 leaves through the right edge alone
    labels, hold, stats = _run(i, case, mv=torch.from_numpy(out).to(dev), link=None)
    s = stats.cpu().numpy()
    assert torch.equal(labels, plain) and bool((hold == 128).all()) and (s[:, oracle.OUTSIDE] == H * W).all() and s.sum() == N * H * W

    labels, hold, stats = _run(i, case, ref=torch.full_like(i["ref"], 255))
    s = stats.cpu().numpy()
    assert torch.equal(labels, plain) and bool((hold == 128).all()) and not s[:, oracle.WEAK:].any() and (s[:, oracle.VOID] > 0).all()
    assert np.array_equal(s, _want(i, ref=np.full_like(i["np"]["ref"], 255))["stats"])

    labels, hold, stats = _run(i, case, link=torch.full_like(i["link"], 0xF1), link_mask=1)
    s = stats.cpu().numpy()
    assert torch.equal(labels, plain) and bool((hold == 128).all()) and (s[:, oracle.UNLINKED] == H * W).all() and s.sum() == N * H * W


@pytest.mark.parametrize("case", ROUTES, ids=ROUTE_IDS)
def test_lut_changes_labels_out_only(dev, inputs, case):
    """With a LUT labels8 is lut[label]; the reference stays in train ids, so hold8 and stats do not move."""
    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    lut = np.random.Generator(np.random.PCG64(2)).permutation(256)[:n_cls].astype(np.uint8)
    labels0, hold0, stats0 = _run(i, case)
    labels, hold, stats = _run(i, case, lut=lut)
    assert torch.equal(hold, hold0) and torch.equal(stats, stats0)
    assert np.array_equal(labels.cpu().numpy(), lut[labels0.cpu().numpy()])
    assert oracle.compare(i["o"], *_np(labels, hold, stats), n_cls, lut=lut) >= 0


@pytest.mark.parametrize("pitch", ["odd", "aligned"])
@pytest.mark.parametrize("case", ROUTES, ids=ROUTE_IDS)
def test_pitched_planes_and_a_frame_slice(dev, inputs, case, pitch):
    """labels8, hold8, the reference, its confidence plane and the link plane in [1:3] slices of pitched buffers (an odd pitch, and a
    4-byte aligned one): the planes equal the dense call's frames 1..2, frame 0 and the guard bytes after every row and after the last
    image stay as they were; the statistics rows belong to the slice; every input is intact after the call."""
    from arseg_amd import egress

    _, _, _, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    N, n0 = 3, i["logits"].shape[0]
    rep = lambda a: np.ascontiguousarray(np.concatenate([np.broadcast_to(a, (n0,) + a.shape[1:])] * 2)[:N])
    logits, mv, beta = (torch.from_numpy(rep(i["np"][k])).to(dev) for k in ("logits", "mv", "beta"))
    ref_np, conf_np, link_np = rep(i["np"]["ref"]), rep(i["np"]["conf"]), rep(i["np"]["link"])
    gates = dict(link_mask=oracle.LINK_MASK, ref_low=oracle.REF_LOW, align_corners=align)
    dense = egress.stabilise(logits, torch.from_numpy(ref_np).to(dev), mv, H, W, beta, link=torch.from_numpy(link_np).to(dev),
                             ref_conf=torch.from_numpy(conf_np).to(dev), hold_out=True, **gates)
    pad = 3 if pitch == "odd" else ((-W) % 4 or 4)                                # every W here is even
    assert (W + pad) % 2 == 1 if pitch == "odd" else (W + pad) % 4 == 0
    step = 2 if pitch == "odd" else 4                                             # every plane has its own pitch, of the same kind
    hb, hv = _backed(N, H, W, pad, dev, 7)
    lb, lv = _backed(N, H, W, pad + step, dev, 9)
    rb, rv = _backed(N, H, W, pad + 2 * step, dev, ref_np)
    cb, cv = _backed(N, H, W, pad + 3 * step, dev, conf_np)
    kb, kv = _backed(N, H, W, pad + 4 * step, dev, link_np)
    stats = torch.zeros((N, NS), dtype=torch.int64, device=dev)
    lg, mvs, bs = logits[1:3].contiguous(), mv[1:3].contiguous(), beta[1:3].contiguous()
    before = [t.clone() for t in (lg, mvs, bs, rb, cb, kb)]
    egress.stabilise(lg, rv[1:3], mvs, H, W, bs, link=kv[1:3], ref_conf=cv[1:3], labels_out=lv[1:3], hold_out=hv[1:3], stats=stats[1:3], **gates)
    assert torch.equal(lv[1:3], dense[0][1:3]) and torch.equal(hv[1:3], dense[1][1:3])
    assert bool((hv[0] == 7).all()) and bool((lv[0] == 9).all())
    assert all(_guards_intact(x, N, W) for x in (hb, lb, rb, cb, kb))
    assert torch.equal(stats[1:3], dense[2][1:3]) and bool((stats[0] == 0).all())
    assert all(torch.equal(x, y) for x, y in zip(before, (lg, mvs, bs, rb, cb, kb)))


@pytest.mark.parametrize("case", ROUTES, ids=ROUTE_IDS)
def test_statistics(dev, inputs, case):
    """stats alone == stats with planes; two launches into one buffer give exactly twice one launch; two runs are bit-equal; the reserved
    word and the entries from n_cls on stay untouched; the inputs are intact."""
    from arseg_amd import egress, ops

    _, _, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    keep = {k: i[k].clone() for k in ("logits", "ref", "mv", "link", "conf", "beta")}
    labels, hold, stats = _run(i, case)
    kw = dict(align_corners=align, link=i["link"], link_mask=oracle.LINK_MASK, ref_conf=i["conf"], ref_low=oracle.REF_LOW)
    alone = torch.full((N, NS), 5, dtype=torch.int64, device=dev)
    ops.segment_stabilise(i["logits"], i["ref"], i["mv"], H, W, i["beta"], stats=alone, **kw)
    assert torch.equal(alone - 5, stats)
    ops.segment_stabilise(i["logits"], i["ref"], i["mv"], H, W, i["beta"], stats=alone, **kw)
    assert torch.equal(alone - 5, 2 * stats)
    assert bool((alone[:, 7] == 5).all()) and bool((alone[:, oracle.INTO + n_cls:oracle.FROM] == 5).all()) and bool((alone[:, oracle.FROM + n_cls:] == 5).all())
    again = _run(i, case)
    assert all(torch.equal(x, y) for x, y in zip(again, (labels, hold, stats)))
    only_l, none_h, none_s = _run(i, case, hold_out=None, stats=None)
    assert none_h is None and none_s is None and torch.equal(only_l, labels)
    none_l, only_h, none_s = _run(i, case, labels_out=None, stats=None)
    assert none_l is None and none_s is None and torch.equal(only_h, hold)
    with pytest.raises(ValueError):
        _run(i, case, labels_out=None, hold_out=None, stats=None)
    assert all(torch.equal(keep[k], i[k]) for k in keep)


@pytest.mark.parametrize("case", [oracle.CASES[0], oracle.CASES[5]], ids=lambda c: c[0])
def test_planted_ties_nan_and_inf_on_the_same_size_route(dev, inputs, case):
    """Exact ties between the top two classes, NaN, +inf and -inf logits and all -inf pixels planted over the seeded logits, an infinite
    threshold in frame 0 and a NaN threshold in frame 1: every byte and counter equals the oracle's (the same-size route is exact)."""
    from arseg_amd import ops

    _, seed, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    g = np.random.Generator(np.random.PCG64(seed + 90))
    x = i["np"]["logits"].copy()
    kind = g.integers(0, 12, (N, H, W))                                                # per pixel: 0..5 planted, the rest as seeded
    a, b = g.integers(0, n_cls, (N, H, W)), g.integers(0, n_cls, (N, H, W))
    nn, yy, xx = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    for code, (va, vb) in enumerate(((9.0, 9.0), (np.nan, 9.0), (np.inf, np.inf), (np.inf, -np.inf), (np.nan, np.nan))):
        m = kind == code
        x[nn[m], b[m], yy[m], xx[m]] = vb
        x[nn[m], a[m], yy[m], xx[m]] = va
    x[np.broadcast_to((kind == 5)[:, None], x.shape)] = -np.inf
    beta = np.array([np.inf, np.nan], dtype=np.float32)
    logits = torch.from_numpy(x).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=align)[0].cpu().numpy().astype(np.int64)
    assert np.array_equal(pred, oracle.label_rule(x))
    got = _run(i, case, logits=logits, bonus=torch.from_numpy(beta).to(dev))
    want = oracle.stabilise(x, i["np"]["ref"], i["np"]["mv"], beta, i["np"]["link"], oracle.LINK_MASK, i["np"]["conf"], oracle.REF_LOW, kstar=pred)
    assert oracle.compare(want, *_np(*got), n_cls) == 0 and np.array_equal(got[2].cpu().numpy(), want["stats"])
    s = want["stats"]
    assert s[0, oracle.HELD] > 0 and s[0, oracle.OWN] > 0 and s[1, oracle.HELD] == 0 and s[1, oracle.OWN] > 0
    assert np.isnan(want["d"][0][want["outcome"][0] == oracle.OWN]).any()              # frame 0's OWN pixels are the non-finite margins


@pytest.mark.parametrize("case", [oracle.CASES[1], oracle.CASES[4]], ids=lambda c: c[0])
def test_planted_ties_nan_and_inf_on_the_resized_routes(dev, inputs, case):
    """Low-resolution patches where two classes tie at the top (the blends of equal taps are equal: d = 0 exactly, held by any positive
    threshold) under the comparison rule; then NaN and infinite taps, whose blends are NaN over a neighbourhood that depends on the
    grouping of the sum: there the gathers stay exact (no prior and AGREE where the oracle says so on the tail's k*), every label is k*
    or c_ref, the statistics are what the planes say, and a NaN threshold holds nothing."""
    from arseg_amd import egress, ops

    _, seed, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    g = np.random.Generator(np.random.PCG64(seed + 91))
    x = i["np"]["logits"].copy()
    ref_np = np.full((1, H, W), n_cls - 1, dtype=np.uint8)                             # the keyframe held the last class everywhere
    ref = torch.from_numpy(ref_np).to(dev)
    for n in range(N):
        for _ in range(4):                                                             # ... and here it ties with an earlier class, which is k*
            y0, x0, ka = int(g.integers(0, h - 3)), int(g.integers(0, w - 3)), int(g.integers(0, n_cls - 1))
            x[n, [ka, n_cls - 1], y0:y0 + 3, x0:x0 + 3] = 7.75
    logits = torch.from_numpy(x).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=align)[0].cpu().numpy().astype(np.int64)
    got = _run(i, case, logits=logits, ref=ref)
    want = oracle.stabilise(oracle.class_values(x, H, W, align), kstar=pred, ref=ref_np, mv_q=i["np"]["mv"], beta=i["np"]["beta"], link=i["np"]["link"],
                            link_mask=oracle.LINK_MASK, ref_conf=i["np"]["conf"], ref_low=oracle.REF_LOW)
    assert oracle.compare(want, *_np(*got), n_cls) >= 0
    ties = (want["d"] == 0) & (want["outcome"] == oracle.HELD)
    assert ties.sum() > 0 and (got[1].cpu().numpy()[ties] == 255).all()

    for n in range(N):
        for v in (np.nan, np.inf, -np.inf):
            x[n, int(g.integers(0, n_cls)), int(g.integers(0, h)), int(g.integers(0, w))] = v
    logits = torch.from_numpy(x).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=align)[0].cpu().numpy().astype(np.int64)
    for beta in (i["beta"], torch.full_like(i["beta"], float("nan"))):
        labels, hold, stats = _np(*_run(i, case, logits=logits, ref=ref, bonus=beta))
        pre = want["pre"]
        assert np.array_equal(hold == 128, pre < 0) and np.array_equal(hold == 0, pre == pred)
        assert np.array_equal(labels, np.where(hold == 255, pre, pred).astype(np.uint8))
        outcome = np.where(hold == 255, oracle.HELD, np.where(hold == 192, oracle.OWN, want["outcome"]))
        assert np.array_equal(stats, oracle.stats_of(outcome, pre, pred, n_cls))
        assert (hold == 255).any() != bool(torch.isnan(beta).all())
    assert np.array_equal(labels, egress.labels8(logits, H, W, align_corners=align).cpu().numpy())


def test_stabilise_in_one_graph(dev, inputs):
    """egress.stabilise(..., labels_out=, hold_out=, stats=) with a device bonus captured once; the logits, mv_q and bonus are refilled in
    place; each of two replays equals the eager result for its own inputs and meets the oracle (the statistics buffer is zeroed before a
    replay: it is accumulated into)."""
    from arseg_amd import egress, ops

    case = oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align, _ = case
    i = inputs(case)
    logits, mv, beta = i["logits"].clone(), i["mv"].clone(), i["beta"].clone()
    labels = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    hold = torch.zeros_like(labels)
    stats = torch.zeros((N, NS), dtype=torch.int64, device=dev)
    kw = dict(link=i["link"], link_mask=oracle.LINK_MASK, ref_conf=i["conf"], ref_low=oracle.REF_LOW, align_corners=align)
    egress.stabilise(logits, i["ref"], mv, H, W, beta, labels_out=labels, hold_out=hold, stats=stats, **kw)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        egress.stabilise(logits, i["ref"], mv, H, W, beta, labels_out=labels, hold_out=hold, stats=stats, **kw)
    for s in (seed + 60, seed + 61):
        fresh = oracle.build((case[0], s) + case[2:])
        fresh["ref"], fresh["link"], fresh["conf"] = i["np"]["ref"], i["np"]["link"], i["np"]["conf"]
        f_logits, f_mv = torch.from_numpy(fresh["logits"]).to(dev), torch.from_numpy(fresh["mv"]).to(dev)
        pred = ops.argmax_confusion(f_logits, None, H, W, align_corners=align)[0].cpu().numpy().astype(np.int64)
        fresh, want = oracle.solve(case, fresh, pred)
        f_beta = torch.from_numpy(fresh["beta"]).to(dev)
        assert not torch.equal(f_beta, i["beta"])
        logits.copy_(f_logits)
        mv.copy_(f_mv)
        beta.copy_(f_beta)
        labels.zero_()
        hold.zero_()
        stats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = egress.stabilise(f_logits, i["ref"], f_mv, H, W, f_beta, hold_out=True, **kw)
        assert torch.equal(labels, eager[0]) and torch.equal(hold, eager[1]) and torch.equal(stats, eager[2])
        assert oracle.compare(want, *_np(labels, hold, stats), n_cls) >= 0 and bool((stats[:, oracle.HELD] > 0).all())


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_alter_res_batch_stabilised(dev, manifest, kind):
    """The small PSPNet (fp32) and BiSeNet (bf16, fused x8 tail) of tests/test_gpu_models.py, motion and link planes from an
    ingest.MotionChain(track_links=True), the keyframe's labels8 and conf8: with a zero threshold the labels are alter_res_batch_render's;
    with a threshold the hold plane's no-prior and AGREE pixels are the oracle's on those labels, every label is k* or the keyframe's
    class, the statistics are what the planes say, and the agreement consistency_of_planes finds is AGREE + HELD; an infinite threshold
    leaves nothing OWN."""
    import test_gpu_ingest_formats as tf          # its _nets wraps test_gpu_models' _psp / _bise (+ bf16 storage)
    from arseg_amd import egress, ingest, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, kind)
    H, W, gop = ((64, 96) if kind == "psp" else (128, 256)) + (4,)
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    chain = ingest.MotionChain(H, W, gop=gop, device=dev, track_links=True)
    recs = synth.make_link_chain(31, H, W, gop - 1, intra=0.1, holes=0.1)
    mvs = chain.push_gop([torch.from_numpy(np.ascontiguousarray(r, dtype=np.int16)).to(dev) for r in recs])[1:]
    link = chain.link()[1:]
    with torch.no_grad():
        key_logits, feat_k = hr.forward_keyframe(frames[0:1])
        key_conf, key_labels, _ = egress.confidence(key_logits.float(), H, W, labels_out=True)
        low = int(key_conf.median())                                                   # the synthetic weights are random: gate on the lower half
        refs = [feat_k[0]] * (gop - 1)
        plain, _ = ev.alter_res_batch_render(lr, refs, frames[1:gop], mvs, 0.5)
        zero = ev.alter_res_batch_stabilised(lr, refs, frames[1:gop], mvs, key_labels, 0.0, link=link, key_conf=key_conf, ref_low=low, hold_out=True)
        some = ev.alter_res_batch_stabilised(lr, refs, frames[1:gop], mvs, key_labels, egress.hold_bonus([1, 2, 3], 1.0, 2.0, device=dev), link=link,
                                             key_conf=key_conf, ref_low=low, hold_out=True)
        every = ev.alter_res_batch_stabilised(lr, refs, frames[1:gop], mvs, key_labels, float("inf"), link=link, key_conf=key_conf, ref_low=low,
                                              hold_out=True)
        ungated = ev.alter_res_batch_stabilised(lr, refs, frames[1:gop], mvs, key_labels, float("inf"), link=link, hold_out=True)
    n_cls = key_logits.shape[1]
    assert tuple(key_labels.shape) == (1, H, W) and torch.equal(zero[0], plain) and not bool(zero[2][:, oracle.HELD].any()) and bool((mvs != 0).any())
    k = plain.cpu().numpy().astype(np.int64)
    pre = oracle.prior(key_labels.cpu().numpy(), mvs.cpu().numpy(), n_cls, link.cpu().numpy(), oracle.LINK_MASK, key_conf.cpu().numpy(), low)
    for labels, hold, stats in (zero, some, every):
        labels, hold, stats = _np(labels, hold, stats)
        assert np.array_equal(hold == 128, pre < 0) and np.array_equal(hold == 0, pre == k)
        assert np.array_equal(labels, np.where(hold == 255, pre, k).astype(np.uint8))
        outcome = np.where(hold == 255, oracle.HELD, np.where(hold == 192, oracle.OWN, np.where(pre < 0, -(pre + 1), oracle.AGREE)))
        assert np.array_equal(stats, oracle.stats_of(outcome, pre, k, n_cls))
    table = egress.hold_table(some[2], n_cls)
    print(f"\n{kind}: outcomes {some[2][:, :7].tolist()}, held of differing {table['held_of_differing'].tolist()}")
    assert not bool(every[2][:, oracle.OWN].any()) and not bool(ungated[2][:, oracle.OWN].any()) and not bool(ungated[2][:, oracle.WEAK].any())
    assert bool((ungated[2][:, oracle.HELD] > 0).all()) and bool((every[2][:, oracle.UNLINKED] > 0).all())
    assert bool((some[2][:, oracle.HELD] <= every[2][:, oracle.HELD]).all()) and bool((every[2][:, oracle.HELD] <= ungated[2][:, oracle.HELD]).all())
    agree = egress.consistency_of_planes(ungated[0], key_labels, mvs, n_cls, link=link, unlinked=True)[1][:, 67:99].sum(dim=1)
    assert torch.equal(agree, ungated[2][:, oracle.AGREE] + ungated[2][:, oracle.HELD])


def test_full_size_x8_grid_arithmetic(dev):
    """One 1024x2048 frame, 19 classes, x8 run route, both gates on: against the oracle on the tail's pred under the comparison rule.  The
    reference is the pred itself displaced, with a void rectangle; the field is block constant, partly pointing back, partly wrong, partly
    off the frame."""
    from arseg_amd import egress, ops

    H, W, n_cls, bs = 1024, 2048, 19, 64
    g = np.random.Generator(np.random.PCG64(271))
    x = oracle.tc.make_logits(g, 1, n_cls, H // 8, W // 8)
    logits = torch.from_numpy(x).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=False)[0]
    ref = torch.roll(pred, shifts=(3, -5), dims=(1, 2)).to(torch.uint8)
    ref[0, 300:420, 900:1300] = 255
    blocks = np.tile(np.array([-20, 12], dtype=np.int16), (H // bs, W // bs, 1))          # points back: round(-20 / 4) = -5, 12 / 4 = 3
    blocks[g.random((H // bs, W // bs)) < 0.3] = (-46, 30)                                # -11.5 -> -12, 7.5 -> 8: wrong by several pixels
    blocks[0, :] = (0, -4 * bs - 2)                                                       # the top block row leaves the frame
    blocks[:, -1] = (32767, -32768)
    mv = np.ascontiguousarray(np.repeat(np.repeat(blocks, bs, axis=0), bs, axis=1)[None])
    flags = np.where(g.random((H // bs, W // bs)) < 0.1, 2, 0).astype(np.uint8)
    link = np.repeat(np.repeat(flags, bs, axis=0), bs, axis=1)[None] | 0x30
    conf = g.integers(100, 256, (1, H, W)).astype(np.uint8)
    b = {"logits": x, "ref": ref.cpu().numpy(), "mv": mv, "link": link, "conf": conf}
    b, want = oracle.solve(("full", 271, 1, n_cls, H // 8, W // 8, H, W, False, True), b, pred.cpu().numpy().astype(np.int64))
    got = egress.stabilise(logits, ref, torch.from_numpy(mv).to(dev), H, W, torch.from_numpy(b["beta"]).to(dev), link=torch.from_numpy(link).to(dev),
                           ref_conf=torch.from_numpy(conf).to(dev), ref_low=oracle.REF_LOW, hold_out=True, align_corners=False)
    assert oracle.compare(want, *_np(*got), n_cls) >= 0
    s = want["stats"][0]
    assert s[:7].sum() == H * W and (s[:7] > 0).all() and s[oracle.HELD] > 0.001 * H * W
