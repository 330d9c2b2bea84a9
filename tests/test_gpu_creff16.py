"""GPU tests of the rolling warp + CReFF kernel's 16-bit input form (arseg_creff_warp16_fwd_ex, ``ops.config.creff_warp16 = "direct"``).

fp16 / bf16 -> fp32 widening is exact and everything behind the kernel's loads is the fp32 kernel's arithmetic, so the criterion is bit
equality with the cast-once route (ops.cast to fp32, then the fp32 instantiation): torch.equal, no tolerance.  A case that is not bit-equal is
a defect in the new loads / offsets.  On top: the launches each route makes, the CPU oracle as an independent anchor, and the model paths."""
import numpy as np
import pytest
import torch

from helpers import maxdiff, sd_from_manifest

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def feat(seed, shape, dtype, top=65504.0):
    """Standard normal scaled to a few units, rounded to ``dtype``, with planted edge values: fp16 subnormals, +-0, the largest finite fp16 (in
    the keyframe features only: ``top`` is a quarter of it for the LR features, whose upsampled values are added to p and would leave the fp16 range of
    the classifier's split operands), and for bf16 values of magnitude
    1e-3 .. 1e3 that fp16 would round.  No infinities or NaNs: they compare unequal to themselves."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = torch.from_numpy((3.0 * g.standard_normal(shape)).astype(np.float32))
    flat = x.reshape(-1)
    special = [5.9604645e-08, -5.9604645e-08, 3.0e-06, -2.0e-07, 6.0e-05, 0.0, -0.0, top, -top, top / 2]
    if dtype == torch.bfloat16:
        special += [1.2345e-3, -9.8765e-3, 0.123456, 3.14159, 123.456, -987.654, 1001.0, 1.0e-3, 999.5]
    pos = g.choice(flat.numel(), size=4 * len(special), replace=False)
    for i, p in enumerate(pos):
        flat[p] = special[i % len(special)]
    return x.to(dtype)


def mvs(kind, seed, B, H, W):
    from arseg_amd import synth

    if kind == "clip":          # synthetic GOP motion (pan + object motion)
        return torch.from_numpy(synth.make_clip(seed, H, W, gop=B + 1)["mv"][1:1 + B].copy())
    g = np.random.Generator(np.random.PCG64(seed))
    mv = g.integers(-41, 42, (B, H, W, 2)).astype(np.int16)          # +-10 px in quarter-pels, fractional positions
    mv[0, : H // 2] = mv[0, 0, 0]
    mv[-1, H // 2:, : W // 2] = (600, -480)          # 150 / 120 px: samples far outside a small map (zero padding, clamped taps)
    mv[-1, : H // 4, W // 2:] = g.integers(-600, 601, (H // 4, W - W // 2, 2)).astype(np.int16)
    return torch.from_numpy(mv)


def attn_and_head(dev, n_cls, seed=7):
    from arseg_amd import synth
    from arseg_amd.model import MyAttention
    from arseg_amd.packing import PackedAttention

    m = synth.load_synth_weights(MyAttention(64, kW=7, kH=7), seed, attn_gain=0.35)
    g = np.random.Generator(np.random.PCG64(seed + 100))
    head = None
    if n_cls:
        head = (torch.from_numpy((0.1 * g.standard_normal((n_cls, 64))).astype(np.float32)).to(dev),
                torch.from_numpy((0.1 * g.standard_normal(n_cls)).astype(np.float32)).to(dev))
    return PackedAttention(m, dev), head


# Hp, Wp, hp, wp, MV scale (H = s Hp), B, shared keyframe feature, n_cls, log_softmax, p layout, MVs, creff_seg_rows
CASES = [
    (48, 64, 24, 32, 1, 3, True, 12, True, "c8", "clip", 0),            # a GOP batch: one keyframe feature, identity MV resize
    (48, 64, 24, 32, 1, 3, False, 12, True, "nhwc", "rand", 0),         # three distinct keyframe features
    (7, 9, 4, 5, 1, 1, True, 0, False, "nhwc", "rand", 0),              # smaller than a strip, no head
    (51, 70, 26, 35, 2, 2, False, 16, False, "c8", "rand", 0),          # odd height, width not a multiple of 16, MVs at 2x (mv_at), 16 classes
    (48, 64, 24, 32, 1, 3, True, 0, False, "c8", "clip", 0),            # no head
    (48, 64, 24, 32, 2, 2, True, 16, True, "nhwc", "clip", 0),          # MVs at twice the feature resolution, clip motion
    (48, 64, 24, 32, 1, 3, True, 12, False, "c8", "rand", 6),           # fixed 6-row segments
    (51, 70, 26, 35, 1, 2, False, 12, True, "nhwc", "clip", 10),        # fixed segments on the ragged shape
    (40, 70, 40, 70, 1, 2, True, 12, True, "c8", "rand", 0),            # lr at the feature's own size
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}s{c[4]}B{c[5]}{'sh' if c[6] else 'di'}n{c[7]}{'L' if c[8] else ''}{c[9]}{c[10]}seg{c[11]}")
def test_direct_equals_cast_once_bit_for_bit(dev, case, dtype):
    from arseg_amd import _lib, ops

    Hp, Wp, hp, wp, s, B, shared, n_cls, logsm, layout, mvk, seg = case
    H, W = s * Hp, s * Wp
    pa, head = attn_and_head(dev, n_cls)
    refs = [feat(50, (Hp, Wp, 64), dtype).to(dev)] * B if shared else [feat(50 + i, (Hp, Wp, 64), dtype).to(dev) for i in range(B)]
    lr = feat(60, (B, hp, wp, 64), dtype, top=16376.0).to(dev)
    mvq = mvs(mvk, 3, B, H, W).to(dev)
    lay = _lib.C8 if layout == "c8" else _lib.NHWC
    prev = ops.configure(creff_warp16="direct", creff_seg_rows=seg)
    try:
        assert ops.creff_warp_kernel(B, 64, Hp, Wp, hp, wp, n_cls) == "roll"
        with ops.profile() as prof:
            p16, l16 = ops.creff_warp(refs, mvq, lr, pa, head, logsm, 7, 7, p_layout=lay)
        summ = prof.summary()
        assert summ["creff_warp"]["launches"] == 1 and "cast" not in summ and "warp_mvq" not in summ, summ
        cast = {}
        refs32 = [cast.setdefault(r.data_ptr(), ops.cast(r, torch.float32)) for r in refs]
        p32, l32 = ops.creff_warp(refs32, mvq, ops.cast(lr, torch.float32), pa, head, logsm, 7, 7, p_layout=lay)
    finally:
        ops.configure(**prev)
    assert p16.dtype == torch.float32 and p16.shape == p32.shape
    nonfinite = int((~torch.isfinite(p32)).sum())
    dp = maxdiff(p16, p32) if nonfinite == 0 else float("nan")
    print(f"\n[{dtype}] {case}: max |p16 - p32| = {dp}, non-finite in p32: {nonfinite}, |p| max {float(p32.abs().max()):.3e}")
    assert torch.equal(p16, p32)
    if n_cls:
        assert l16.dtype == torch.float32 and torch.equal(l16, l32), maxdiff(l16, l32)
    else:
        assert l16 is None and l32 is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_launches_of_the_two_routes(dev, dtype):
    """direct: exactly one creff_warp launch, no cast, no warp_mvq.  cast: the casts (one per distinct keyframe feature + one for the LR batch)
    ahead of one creff_warp launch.  Mixed element types are refused on either."""
    from arseg_amd import _lib, ops

    B, Hp, Wp = 3, 48, 64
    pa, head = attn_and_head(dev, 12)
    ref, lr = feat(1, (Hp, Wp, 64), dtype).to(dev), feat(2, (B, Hp // 2, Wp // 2, 64), dtype, top=16376.0).to(dev)
    mvq = mvs("clip", 5, B, Hp, Wp).to(dev)
    got = {}
    for knob in ("direct", "cast"):
        prev = ops.configure(creff_warp16=knob)
        try:
            with ops.profile() as prof:
                got[knob] = ops.creff_warp([ref] * B, mvq, lr, pa, head, True, 7, 7)
            summ = prof.summary()
        finally:
            ops.configure(**prev)
        assert summ["creff_warp"]["launches"] == 1 and "warp_mvq" not in summ, (knob, summ)
        if knob == "direct":
            assert "cast" not in summ, summ
        else:
            assert summ["cast"]["launches"] == 2, summ
    assert torch.equal(got["direct"][0], got["cast"][0]) and torch.equal(got["direct"][1], got["cast"][1])
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    for r_, l_ in ((ref.float(), lr), (ref, lr.float()), (ref.to(other), lr)):
        with pytest.raises(_lib.ArsegError):
            ops.creff_warp([r_] * B, mvq, l_, pa, head, True, 7, 7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_direct_route_against_the_oracle(dev, manifest, dtype):
    """The direct route against the CPU oracle's warp + my_attention + head on the same rounded inputs, within the bound the cast-once route is
    held to (2e-4 of the magnitude, test_gpu_psp16.py::test_phase2_cast_once_on_the_fused_kernel)."""
    from arseg_amd import _lib, ops, synth
    from arseg_amd.model import PSPNetWithFuse
    from oracle import cpu_ref

    kw = dict(sizes=(1, 2, 3, 6), n_classes=12, psp_size=512, deep_features_size=256, backend="resnet18")
    lr = PSPNetWithFuse(atten_k=7, **kw)
    spec = [(k, tuple(s)) for k, s in manifest["PSPNetWithFuse"]["keys"]]
    lr.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 1, 0.12, 0.3).items()})
    lr = lr.to(dev).eval().set_storage(dtype)
    sd = sd_from_manifest(manifest, "PSPNetWithFuse", 1)
    H, W, B = 48, 64, 3
    g = np.random.Generator(np.random.PCG64(30))
    ref16 = torch.from_numpy(g.standard_normal((H, W, 64)).astype(np.float32)).to(dtype)
    lr16 = torch.from_numpy(g.standard_normal((B, H // 2, W // 2, 64)).astype(np.float32)).to(dtype)
    mvq = torch.from_numpy(synth.make_clip(3, H, W, gop=4)["mv"][1:1 + B])
    prev = ops.configure(creff_warp16="direct")
    try:
        with torch.no_grad(), ops.profile() as prof:
            out, p_c8 = lr.phase2_warp(lr16.to(dev), [ref16.to(dev)] * B, mvq.to(dev))
        summ = prof.summary()
    finally:
        ops.configure(**prev)
    assert summ["creff_warp"]["launches"] == 1 and "cast" not in summ and "warp_mvq" not in summ, summ
    ref_nchw = ref16.float().permute(2, 0, 1)[None]
    outs, ps = [], []
    for i in range(B):
        warped = cpu_ref.warp_feature(ref_nchw, cpu_ref.mv_resize(cpu_ref.mv_from_int16(mvq[i:i + 1]), H, W))
        o, pp = cpu_ref.pspnet_fuse_phase2(sd, lr16[i:i + 1].float().permute(0, 3, 1, 2), warped)
        outs.append(o)
        ps.append(pp)
    o_ref, p_ref = torch.cat(outs), torch.cat(ps)
    p = ops.from_c8(p_c8, _lib.NCHW)
    e_p, e_o = maxdiff(p, p_ref) / float(p_ref.abs().max()), maxdiff(out, o_ref) / float(o_ref.abs().max())
    print(f"\n[{dtype}] phase 2 (direct 16-bit loads): p rel err {e_p:.2e}, log-probs rel err {e_o:.2e}")
    assert out.dtype == torch.float32 and e_p <= 2e-4 and e_o <= 2e-4


def _nets(dev, dtype, n_classes=12):
    from arseg_amd import synth
    from arseg_amd.model import PSPNet, PSPNetWithFuse

    kw = dict(sizes=(1, 2, 3, 6), n_classes=n_classes, psp_size=512, deep_features_size=256, backend="resnet18")
    hr, lr = PSPNet(**kw), PSPNetWithFuse(atten_k=7, **kw)
    synth.load_synth_weights(hr, 0)
    synth.load_synth_weights(lr, 1)
    return hr.to(dev).eval().set_storage(dtype), lr.to(dev).eval().set_storage(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_paths_equal_under_both_routes(dev, dtype):
    """set_storage(dtype) on a 48x64 GOP-12 clip: the batched path, the per-frame path and the single-GPU GopRunner give the same bits under
    "direct" and "cast"."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from arseg_amd.gop import GopRunner

    hr, lr = _nets(dev, dtype)
    clip = synth.make_clip(6, 48, 64, gop=12)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mv = torch.from_numpy(clip["mv"]).to(dev)
    res = {}
    for knob in ("cast", "direct", "cast"):          # (the first pass also tunes the conv plans both routes then share)
        prev = ops.configure(creff_warp16=knob)
        try:
            with torch.no_grad():
                ref_p = ops.to_nhwc(hr(frames[0:1])[-1])[0]
                assert ref_p.dtype == dtype
                with ops.profile() as prof:
                    out_b, p_b = ev.alter_res_batch_fast(lr, [ref_p] * 11, frames[1:12], mv[1:12], 0.5)
                summ = prof.summary()
                per = [ev.alter_res_step_fast(lr, ref_p.unsqueeze(0), frames[d:d + 1], mv[d:d + 1], 0.5) for d in (1, 5, 11)]
                runner = GopRunner(lambda k: ops.to_nhwc(hr(k)[-1])[0],
                                   lambda ref, img, m: ev.alter_res_step_fast(lr, ref.unsqueeze(0), img, m, 0.5)[0], n_gops=1, gop=12)
                out_r = runner.run_batched({0: frames[0:1]}, frames[1:12], mv[1:12],
                                           lambda refs, imgs, m: ev.alter_res_batch_fast(lr, refs, imgs, m, 0.5)[0])
        finally:
            ops.configure(**prev)
        assert summ["creff_warp"]["launches"] == 1 and "warp_mvq" not in summ
        assert ("cast" in summ) == (knob == "cast"), (knob, sorted(summ))
        res[knob] = (out_b, p_b, [o for o, _ in per], [p for _, p in per], out_r)
    d, c = res["direct"], res["cast"]
    assert torch.equal(d[0], c[0]) and torch.equal(d[1], c[1]) and torch.equal(d[4], c[4])
    for i in range(3):
        assert torch.equal(d[2][i], c[2][i]) and torch.equal(d[3][i], c[3][i])


@pytest.mark.parametrize("dtype", DTYPES)
def test_routes_the_rolling_kernel_does_not_serve_are_untouched(dev, dtype):
    """A 19-class head (tile kernel) is cast once and runs the fp32 fused entry point under either knob; a C = 8 MyAttention takes
    warp_mvq16 + CReFF under either knob.  Same bits under both knobs."""
    from arseg_amd import ops, synth
    from arseg_amd.model import MyAttention

    _, lr = _nets(dev, dtype, n_classes=19)
    B, H, W = 2, 33, 47
    ref, low = feat(7, (H, W, 64), dtype).to(dev), feat(8, (B, 17, 24, 64), dtype, top=16376.0).to(dev)
    mvq = mvs("rand", 9, B, H, W).to(dev)
    assert ops.creff_warp_kernel(B, 64, H, W, 17, 24, 19) == "tiles"
    m8 = synth.load_synth_weights(MyAttention(8, kW=7, kH=7), 3).to(dev).eval()
    ref8, low8 = feat(10, (H, W, 8), dtype).to(dev), feat(11, (B, 17, 24, 8), dtype, top=16376.0).to(dev)
    got = {}
    for knob in ("direct", "cast"):
        prev = ops.configure(creff_warp16=knob)
        try:
            with torch.no_grad(), ops.profile() as prof:
                out, p = lr.phase2_warp(low, [ref] * B, mvq)
            summ = prof.summary()
            assert summ["cast"]["launches"] == 2 and summ["creff_warp"]["launches"] == 1 and "warp_mvq" not in summ, (knob, summ)
            with torch.no_grad(), ops.profile() as prof:
                p8, _ = m8.fuse_warp([ref8] * B, mvq, low8)
            summ = prof.summary()
            assert "warp_mvq" in summ and "creff" in summ and "creff_warp" not in summ, (knob, summ)
        finally:
            ops.configure(**prev)
        got[knob] = (out, p, p8)
    for a, b in zip(got["direct"], got["cast"]):
        assert torch.equal(a, b)


def test_full_size_bf16_direct_equals_cast(dev):
    """11 frames at 512x1024, 12 classes, bf16: the balanced schedule on every compute unit (whole-strip passes and remainder runs)."""
    from arseg_amd import ops

    B, Hp, Wp = 11, 512, 1024
    dtype = torch.bfloat16
    pa, head = attn_and_head(dev, 12)
    g = torch.Generator(device="cpu").manual_seed(4)
    ref = (3.0 * torch.randn(Hp, Wp, 64, generator=g)).to(dtype).to(dev)
    lr = (3.0 * torch.randn(B, Hp // 2, Wp // 2, 64, generator=g)).to(dtype).to(dev)
    mvq = mvs("clip", 2, B, Hp, Wp).to(dev)
    assert ops.creff_warp_kernel(B, 64, Hp, Wp, Hp // 2, Wp // 2, 12) == "roll"
    got = {}
    for knob in ("direct", "cast"):
        prev = ops.configure(creff_warp16=knob)
        try:
            with ops.profile() as prof:
                got[knob] = ops.creff_warp([ref] * B, mvq, lr, pa, head, True, 7, 7)
            summ = prof.summary()
        finally:
            ops.configure(**prev)
        assert summ["creff_warp"]["launches"] == 1 and ("cast" in summ) == (knob == "cast")
    assert torch.equal(got["direct"][0], got["cast"][0])
    assert torch.equal(got["direct"][1], got["cast"][1])
