"""GPU tests of the CamVid PSPNet-18 16-bit storage path (set_storage(torch.bfloat16 | torch.float16)).

Op level: the 16-bit conv with the x2 upsample fused into its patch staging is bit-identical to resize16 -> conv2d16 under the same plan and
within one rounding of fp64 on the rounded upsample; the 16-bit pyramid (pool matrix, prior sum) against fp64 on the same rounded input;
the 16-bit global max exactly.  Model level: the reference's fp32 fixtures G4 / G5 / G7-psp / G10-psp with the measured error per dtype,
phase 2 of the fuse net on the fp32 fused warp + CReFF kernel, and the batched / runner paths against the per-frame path."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import maxdiff, t

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}          # spacing relative to the bottom of a binade; one rounding errs <= ULP / 2
REL = {torch.float16: 4e-3, torch.bfloat16: 3e-2}                      # BiSeNet's 16-bit bounds (test_gpu_16bit.py), relative to the magnitude
AGREE = {torch.float16: 0.998, torch.bfloat16: 0.99}                  # BiSeNet's label-agreement bounds
AGREE2 = {torch.float16: 0.996, torch.bfloat16: 0.98}                  # twice BiSeNet's miss rate: the loosest allowed (set where measured is close)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def rnd(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32))


def close16(got, want, dtype, extra=0.0):
    """|got - want| <= ulp/2 * |want| + (fp32 accumulation slack) elementwise (the bound of test_gpu_16bit.py)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    tol = ULP[dtype] * 0.51 * want.abs() + extra + 1e-6
    bad = (got - want).abs() > tol
    assert not bool(bad.any()), (float((got - want).abs().max()), int(bad.sum()))


# ------------------------------------------------------------------------------------------------ op level

UP_CASES = [            # N, h, w (low resolution), Cin, Cout, act: shapes like up_1 / up_2 / up_3 at small maps, and an odd low-resolution size
    (3, 8, 16, 1024, 256, "prelu"),
    (3, 16, 32, 256, 64, "prelu"),
    (3, 32, 64, 64, 64, "prelu"),
    (3, 7, 9, 64, 64, "relu"),
    (3, 7, 9, 128, 192, "prelu"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: f"{c[1]}x{c[2]}c{c[3]}to{c[4]}{c[5]}")
def test_conv16_fused_upsample(dev, case, dtype):
    from arseg_amd import _lib, ops
    from arseg_amd.packing import PackedConv

    N, h, w, Cin, Cout, act = case
    g = np.random.Generator(np.random.PCG64(4))
    bnp = (t(g.uniform(0.75, 1.25, Cout).astype(np.float32)), rnd(5, Cout, scale=0.1), rnd(6, Cout, scale=0.1),
           t(g.uniform(0.5, 1.5, Cout).astype(np.float32)))
    wt, b = rnd(2, Cout, Cin, 3, 3, scale=(2.0 / (Cin * 9)) ** 0.5), rnd(3, Cout, scale=0.1)
    code = {"relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU}[act]
    pc = PackedConv(wt, b, bnp, 1, 1, 1, code, 0.25, dev)
    x = rnd(1, N, h, w, Cin).to(dtype).to(dev)
    up = ops.resize_nhwc(x, 2 * h, 2 * w, _lib.BILINEAR, False)              # the materialised upsample (16-bit, rounded once)
    # fp64 on the rounded upsample
    y = F.conv2d(up.cpu().double().permute(0, 3, 1, 2), wt.to(dtype).double(), None, padding=1)
    gam, bet, mu, var = (v.double() for v in bnp)
    sc = gam / torch.sqrt(var + 1e-5)
    y = y * sc[None, :, None, None] + (bet - mu * sc + b.double() * sc)[None, :, None, None]
    y = torch.relu(y) if act == "relu" else torch.where(y >= 0, y, 0.25 * y)
    n_run = 0
    for cfg in (5, 6, 7, 8, 10, 11, 12, 13):
        try:
            got = ops.conv2d(x, pc, up2=True, tile_cfg=cfg)
        except _lib.ArsegError as exc:                      # the squarer tiles are refused on maps whose default tile is that narrow
            assert cfg >= 10 and ("unsupported" in str(exc).lower() or "-2" in str(exc)), exc
            continue
        n_run += 1
        want = ops.conv2d(up, pc, tile_cfg=cfg)
        assert got.dtype == dtype and got.shape == (N, 2 * h, 2 * w, Cout)
        assert torch.equal(got, want), (cfg, maxdiff(got, want))
        close16(got.permute(0, 3, 1, 2), y, dtype, extra=2e-5 * float(y.abs().max()))
    assert n_run >= 4
    # automatic plan (fused or materialised, whichever was timed faster): the same numbers as one of the two
    auto = ops.conv2d(x, pc, up2=True)
    close16(auto.permute(0, 3, 1, 2), y, dtype, extra=2e-5 * float(y.abs().max()))
    # pinned non-patch plans: resize16 + conv2d16 with that plan (the library itself refuses upsample2x there, see the next test)
    for cfg in (1, 2, 3, 4):
        assert torch.equal(ops.conv2d(x, pc, up2=True, tile_cfg=cfg), ops.conv2d(up, pc, tile_cfg=cfg))


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv16_upsample2x_refusals_on_device(dev, dtype):
    """ARSEG_EUNSUPPORTED for the non-patch plans, an odd H and dil = 2, on real device buffers."""
    import ctypes

    from arseg_amd import _lib
    from arseg_amd.packing import PackedConv

    lib = _lib.load()
    pc = PackedConv(rnd(2, 64, 64, 3, 3, scale=0.05), None, None, 1, 1, 1, _lib.ACT_RELU, 0.0, dev)
    w16, _ = pc.weights16(dtype)
    x = rnd(1, 2, 7, 9, 64).to(dtype).to(dev)
    out = torch.empty(2, 14, 18, 64, dtype=dtype, device=dev)

    def run(cfg, H=14, W=18, dil=1):
        d = _lib.ConvDesc()
        d.N, d.H, d.W, d.Cin, d.in_ld, d.Cout, d.out_ld, d.res_ld = 2, H, W, 64, 64, 64, 64, 64
        d.R, d.S, d.stride, d.pad, d.dil = 3, 3, 1, dil, dil
        d.act, d.tile_cfg, d.upsample2x = _lib.ACT_RELU, cfg, 1
        return lib.arseg_conv2d16_fwd(ctypes.byref(d), {torch.float16: _lib.DT_F16, torch.bfloat16: _lib.DT_BF16}[dtype],
                                      ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(w16.data_ptr()), None, None, None,
                                      ctypes.c_void_p(out.data_ptr()), None, 0, None)

    for cfg in (1, 2, 3, 4, 9):
        assert run(cfg) == _lib.ARSEG_EUNSUPPORTED
    assert run(7, H=13) == _lib.ARSEG_EUNSUPPORTED
    assert run(7, dil=2) == _lib.ARSEG_EUNSUPPORTED
    assert run(7) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(32, 64), (7, 11)])
def test_psp_pyramid16_and_global_max(dev, dtype, hw):
    from arseg_amd import _lib, ops

    sizes = (1, 2, 3, 6)
    H, W = hw
    N, C = 2, 64
    x = rnd(20, N, H, W, C).to(dtype)
    xd = x.to(dev)
    rows = sum(s * s for s in sizes)
    poison = torch.full((N, rows, 1, len(sizes) * C), float("nan"), dtype=dtype, device=dev)      # the caching allocator hands this block back
    del poison
    pm = ops.psp_pool_matrix(xd, sizes)
    assert pm.dtype == dtype and pm.shape == (N, rows, 1, len(sizes) * C)
    want = torch.zeros(N, rows, len(sizes) * C, dtype=torch.float64)
    xc = x.double().permute(0, 3, 1, 2)
    off = 0
    for i, s in enumerate(sizes):
        want[:, off:off + s * s, i * C:(i + 1) * C] = F.adaptive_avg_pool2d(xc, s).permute(0, 2, 3, 1).reshape(N, s * s, C)
        off += s * s
    close16(pm[:, :, 0], want, dtype, extra=1e-6)
    assert bool((pm[:, :, 0].cpu().double()[want == 0] == 0).all())                     # the zero blocks are written, exactly
    # prior sum: sum over levels of the bilinear (align_corners=False) upsamples of the 16-bit maps
    tm = rnd(21, N, rows, C).to(dtype)
    got = ops.psp_prior_sum(tm.to(dev), sizes, H, W)
    assert got.dtype == dtype and got.shape == (N, H, W, C)
    want = torch.zeros(N, C, H, W, dtype=torch.float64)
    off = 0
    for s in sizes:
        m = tm[:, off:off + s * s].double().reshape(N, s, s, C).permute(0, 3, 1, 2)
        want += F.interpolate(m, (H, W), mode="bilinear", align_corners=False)
        off += s * s
    close16(got.permute(0, 3, 1, 2), want, dtype, extra=1e-5 * float(want.abs().max()))
    # global max: exact
    mx = ops.global_reduce(xd, _lib.REDUCE_MAX)
    assert mx.dtype == dtype and torch.equal(mx[:, 0, 0].cpu(), torch.amax(x, dim=(1, 2)))
    # a NaN in a channel gives NaN there, nowhere else
    xn = x.clone()
    xn[1, H // 2, W // 3, 5] = float("nan")
    mn = ops.global_reduce(xn.to(dev), _lib.REDUCE_MAX)[:, 0, 0].cpu()
    assert bool(torch.isnan(mn[1, 5])) and int(torch.isnan(mn).sum()) == 1
    again = ops.global_reduce(xn.to(dev), _lib.REDUCE_MAX)[:, 0, 0].cpu()
    assert torch.equal(mn.view(torch.int16), again.view(torch.int16))                    # deterministic, bit for bit (NaN included)
    assert torch.equal(mn[0], torch.amax(x[0], dim=(0, 1)))


# ------------------------------------------------------------------------------------------------ model level

def _psp16(manifest, dev, fuse, dtype, seed=None, gains=(0.12, 0.3)):
    from arseg_amd import synth
    from arseg_amd.model import PSPNet, PSPNetWithFuse

    kw = dict(sizes=(1, 2, 3, 6), n_classes=12, psp_size=512, deep_features_size=256, backend="resnet18")
    m = PSPNetWithFuse(atten_k=7, **kw) if fuse else PSPNet(**kw)
    name, dseed = ("PSPNetWithFuse", 1) if fuse else ("PSPNet", 0)
    spec = [(k, tuple(s)) for k, s in manifest[name]["keys"]]
    seed = dseed if seed is None else seed
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed, *gains).items()})
    m = m.to(dev).eval()
    return m if dtype == torch.float32 else m.set_storage(dtype)


def _rel(got, want):
    return maxdiff(got, want) / float(np.abs(np.asarray(want)).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pspnet16_golden(dev, golden, manifest, dtype):
    """G4 (PSPNet) and G5 (PSPNetWithFuse: phase 1, phase 2 NCHW / channels_last, normal, merge) with 16-bit storage, against the reference's
    fp32 fixtures: error relative to the tensor's magnitude, label agreement."""
    g = golden("g4_pspnet")
    net = _psp16(manifest, dev, False, dtype)
    with torch.no_grad():
        out, cls, p = net(t(g["x"]).to(dev))
    assert out.dtype == torch.float32 and cls.dtype == torch.float32 and p.dtype == dtype
    assert out.shape == g["out"].shape and cls.shape == g["cls"].shape and p.shape == g["p"].shape
    e = {"out": _rel(out, g["out"]), "cls": _rel(cls, g["cls"]), "p": _rel(p.float(), g["p"])}
    agree = float((out.argmax(1).cpu().numpy() == g["out"].argmax(1)).mean())
    print(f"\n[{dtype}] G4 PSPNet: rel err {e}, labels equal {agree:.4f}")
    # measured (3 runs): rel err <= 2.1e-3 (fp16) / 1.3e-2 (bf16); labels 0.9984-0.9990 / 0.9951-0.9974
    assert all(v <= REL[dtype] for v in e.values()) and agree >= AGREE[dtype]

    g5 = golden("g5_pspfuse")
    ref_p = t(g["p"]).to(dev)
    lr = _psp16(manifest, dev, True, dtype)
    with torch.no_grad():
        cls1, p1 = lr.forward_phase1(t(g5["x"]).to(dev))
        assert p1.dtype == dtype and cls1.dtype == torch.float32
        out2, p2 = lr.forward_phase2(p1, ref_p.to(dtype))                                          # 16-bit, channels_last views
        out2b, p2b = lr.forward_phase2(p1.float().contiguous(), ref_p)                               # fp32, NCHW-contiguous
        outn, clsn, pn = lr(t(g5["x"]).to(dev), mode="normal")
        outm, clsm, pm = lr(t(g5["x"]).to(dev), mode="merge", ref_p=ref_p.to(dtype).contiguous(memory_format=torch.channels_last))
    assert out2.dtype == torch.float32 and p2.dtype == torch.float32
    e5 = {"cls1": _rel(cls1, g5["cls1"]), "p1": _rel(p1.float(), g5["p1"]), "out2": _rel(out2, g5["out2"]), "p2": _rel(p2, g5["p2"]),
          "out2b": _rel(out2b, g5["out2"]), "normal": _rel(outn, g5["out_normal"]), "merge": _rel(outm, g5["out2"]), "clsm": _rel(clsm, g5["cls1"])}
    agree5 = float((out2.argmax(1).cpu().numpy() == g5["out2"].argmax(1)).mean())
    print(f"[{dtype}] G5 PSPNetWithFuse: rel err {e5}, labels equal {agree5:.4f}")
    # measured (3 runs): rel err <= 1.5e-3 (fp16) / 1.35e-2 (bf16); labels 0.9997 / 0.9938
    assert all(v <= REL[dtype] for v in e5.values()) and agree5 >= AGREE[dtype]
    assert torch.equal(outm, out2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_alter_res_psp16_golden(dev, golden, manifest, dtype):
    """G7-psp: one EvalAlterRes step on the fast path with 16-bit storage (keyframe HR forward, LR backbone, cast-once fp32 warp + CReFF +
    head, fused argmax tail) against the reference's fp32 logits / labels / histogram count."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops

    g = golden("g7_alter_psp")
    hr, lr = _psp16(manifest, dev, False, dtype), _psp16(manifest, dev, True, dtype)
    img, ref, label, mvq = t(g["img"]), t(g["ref"]), t(g["label"]), t(g["mvq"])
    with torch.no_grad():
        ref_p = hr(ref.to(dev))[-1]
        assert ref_p.dtype == dtype
        out, _ = ev.alter_res_step_fast(lr, ops.to_nhwc(ref_p), img.to(dev), mvq.to(dev), 0.5)
        pred, hist = ev.alter_res_batch_pred(lr, [ops.to_nhwc(ref_p)[0]], img.to(dev), mvq.to(dev), 0.5, labels=label.to(dev))
    e = _rel(out, g["out"])
    agree = float((pred.cpu().long().numpy() == g["preds"]).mean())
    print(f"\n[{dtype}] G7-psp step: logits rel err {e:.3e}, labels equal {agree:.4f}")
    # measured (3 runs): fp16 9.2e-4 / 0.9984-0.9987, bf16 9.4e-3 / 0.9880-0.9883.  bf16 misses BiSeNet's 0.99 label bound on this fixture; the
    # bound here is twice BiSeNet's miss rate, the loosest allowed
    assert e <= REL[dtype] and agree >= AGREE2[dtype]
    assert int(hist.sum()) == int((label != 255).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_undamped_psp16_golden(dev, golden, manifest, dtype):
    """G10-undamped-psp (He initialisation everywhere, activations in the hundreds) with 16-bit storage: end-to-end logits and labels."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops

    g = golden("g10_undamped_psp")
    hr = _psp16(manifest, dev, False, dtype, seed=20, gains=(1.0, 1.0))
    lr = _psp16(manifest, dev, True, dtype, seed=21, gains=(1.0, 1.0))
    img, ref, label, mvq = t(g["img"]), t(g["ref"]), t(g["label"]), t(g["mvq"])
    with torch.no_grad():
        ref_p = hr(ref.to(dev))[-1]
        out, _ = ev.alter_res_step_fast(lr, ops.to_nhwc(ref_p), img.to(dev), mvq.to(dev), 0.5)
        pred, _ = ops.argmax_confusion(out, label.to(dev), label.shape[-2], label.shape[-1])
    e = _rel(out, g["out"])
    agree = float((pred.cpu().long().numpy() == g["preds"]).mean())
    print(f"\n[{dtype}] G10-undamped-psp: logits rel err {e:.3e}, labels equal {agree:.5f}")
    # measured: labels 0.99935 (fp16) / 0.99447 (bf16).  The log-probs themselves are NOT held to BiSeNet's relative bound here: measured 6.8e-2
    # (fp16) / 4.1e-1 (bf16) of the magnitude.  At this conditioning the sharp softmax amplifies rounding (even an fp32 evaluation is defined
    # only to ~1e-2 absolute, test_gpu_models.py::test_eval_alter_res_undamped_golden), so only the labels are asserted
    assert agree >= AGREE[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_phase2_cast_once_on_the_fused_kernel(dev, manifest, dtype):
    """Phase 2 on rounded 16-bit inputs at C = 64: the keyframe and LR features are cast to fp32 once and the fp32 fused warp + CReFF + head
    kernel runs (a creff_warp launch, no warp_mvq launch); against the CPU oracle's warp + my_attention + head on the same rounded inputs."""
    from arseg_amd import _lib, ops, synth
    from helpers import sd_from_manifest
    from oracle import cpu_ref

    lr = _psp16(manifest, dev, True, dtype)
    sd = sd_from_manifest(manifest, "PSPNetWithFuse", 1)
    H, W, B = 48, 64, 3
    ref16 = rnd(30, H, W, 64).to(dtype)
    lr16 = rnd(31, B, H // 2, W // 2, 64).to(dtype)
    clip = synth.make_clip(3, H, W, gop=4)
    mvq = torch.from_numpy(clip["mv"][1:1 + B])
    assert ops.creff_warp_kernel(B, 64, H, W, H // 2, W // 2, 12) == "roll"
    refd = ref16.to(dev)
    with torch.no_grad(), ops.profile() as prof:
        out, p_c8 = lr.phase2_warp(lr16.to(dev), [refd] * B, mvq.to(dev))
    summ = prof.summary()
    assert summ["creff_warp"]["launches"] == 1 and "warp_mvq" not in summ, summ
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
    print(f"\n[{dtype}] phase 2 (cast once, fused kernel): p rel err {e_p:.2e}, log-probs rel err {e_o:.2e}")
    assert out.dtype == torch.float32 and e_p <= 2e-4 and e_o <= 2e-4


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_and_runner16_equal_per_frame(dev, manifest, dtype):
    """The single-GPU GopRunner (which exchanges the 16-bit keyframe feature) equals alter_res_batch_fast over the 11 frames bit for bit; the
    batched path equals the per-frame path within the 16-bit bound (REL x magnitude), not bit for bit: the per-shape conv plans differ
    between N = 11 and N = 1."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from arseg_amd.gop import GopRunner

    hr, lr = _psp16(manifest, dev, False, dtype), _psp16(manifest, dev, True, dtype)
    clip = synth.make_clip(6, 48, 64, gop=12)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    with torch.no_grad():
        ref_p = ops.to_nhwc(hr(frames[0:1])[-1])[0]
        assert ref_p.dtype == dtype
        out_b, p_b = ev.alter_res_batch_fast(lr, [ref_p] * 11, frames[1:12], mvs[1:12], 0.5)
        per = [ev.alter_res_step_fast(lr, ref_p.unsqueeze(0), frames[d:d + 1], mvs[d:d + 1], 0.5) for d in range(1, 12)]
        runner = GopRunner(lambda k: ops.to_nhwc(hr(k)[-1])[0],
                           lambda ref, img, mv: ev.alter_res_step_fast(lr, ref.unsqueeze(0), img, mv, 0.5)[0], n_gops=1, gop=12)
        out_r = runner.run_batched({0: frames[0:1]}, frames[1:12], mvs[1:12],
                                   lambda refs, imgs, mv: ev.alter_res_batch_fast(lr, refs, imgs, mv, 0.5)[0])
    diffs = [maxdiff(out_b[i:i + 1], per[i][0]) for i in range(11)]
    print(f"\n[{dtype}] batch vs per-frame: max |diff| {max(diffs):.3e}; runner vs batch {maxdiff(out_r, out_b):.3e}")
    # the runner replays the batched path: bit for bit.  Batch against per-frame is NOT bit for bit in 16-bit (measured max |diff| of the
    # log-probs 1.2e-2 fp16 / 8.0e-2 bf16): the per-shape conv plans (tile, split-K, fused or materialised upsample) differ between N = 11 and
    # N = 1 and each rounds to 16 bits at a different point; held to the 16-bit bound instead
    assert torch.equal(out_r, out_b)
    mag = max(float(o.abs().max()) for o, _ in per)
    for i in range(11):
        assert maxdiff(out_b[i:i + 1], per[i][0]) <= REL[dtype] * mag


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_size_psp16_step(dev, dtype):
    """The headline shape: 512x1024 keyframe + one non-keyframe in 16-bit against the fp32 GPU path (itself held to 1e-3 against the oracle
    by test_gpu_models.py::test_full_size_end_to_end_headline): worst pixel, relative RMS and label agreement of the logits and of ref_p."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from arseg_amd.model import PSPNet, PSPNetWithFuse

    H, W = 512, 1024
    kw = dict(sizes=(1, 2, 3, 6), n_classes=12, psp_size=512, deep_features_size=256, backend="resnet18")
    hr, lr = PSPNet(**kw), PSPNetWithFuse(atten_k=7, **kw)
    synth.load_synth_weights(hr, 0)
    synth.load_synth_weights(lr, 1)
    hr, lr = hr.to(dev).eval(), lr.to(dev).eval()
    clip = synth.make_clip(2, H, W, gop=6, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    key, img, mvq = (torch.from_numpy(clip[k][i:i + 1]).to(dev) for k, i in (("frames", 0), ("frames", 5), ("mv", 5)))
    with torch.no_grad():
        ref32 = hr(key)[-1]
        out32, _ = ev.alter_res_step_fast(lr, ops.to_nhwc(ref32), img, mvq, 0.5)
        hr.set_storage(dtype)
        lr.set_storage(dtype)
        ref16 = hr(key)[-1]
        out16, _ = ev.alter_res_step_fast(lr, ops.to_nhwc(ref16), img, mvq, 0.5)

    def stats(a, b):
        a, b = a.float().cpu().double(), b.float().cpu().double()
        return float((a - b).abs().max()) / float(b.abs().max()), float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())

    wo, rmso = stats(out16, out32)
    wp, rmsp = stats(ref16, ref32)
    agree = float((out16.argmax(1) == out32.argmax(1)).float().mean())
    # labels exactly wherever the fp32 top-2 margin exceeds twice the worst logit error (no argmax can flip there)
    err = float((out16 - out32).abs().max())
    top2 = out32.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 2 * err
    print(f"\n[{dtype}] full size: logits worst {wo:.2e} rms {rmso:.2e}; ref_p worst {wp:.2e} rms {rmsp:.2e}; labels equal {agree:.5f} "
          f"(exact on {float(safe.float().mean()):.4f} of the pixels)")
    assert ref16.dtype == dtype and out16.dtype == torch.float32
    assert wo <= REL[dtype] and wp <= REL[dtype]
    assert torch.equal(out16.argmax(1)[safe], out32.argmax(1)[safe])
    # measured raw label agreement: fp16 0.99800, bf16 0.9745-0.9770 -- bf16 misses BiSeNet's 0.99 on these random-init weights (many near-tied
    # classes); fp16 sits at BiSeNet's bound, so it is held to twice BiSeNet's miss rate.  bf16 is below even that and is reported, not
    # asserted at a looser value: for bf16 the margin test above is what is asserted (measured worst logit error 1.1e-3 fp16 / 8.9e-3 - 1.0e-2
    # bf16 of the magnitude)
    if dtype == torch.float16:
        assert agree >= AGREE2[dtype]
