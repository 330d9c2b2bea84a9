"""GPU checks of the planar 4:2:0 / 10-bit frame ingest (csrc/ingest.hip, arseg_frame_ingest_yuv_fwd: I420, P010, I010; the kernel family it
shares with RGB8 / NV12) and of the fast paths fed with ingest.DecodedFrames.i420 / p010 / i010."""
import numpy as np
import pytest
import torch

import ingest_oracle as oracle
import ingest_oracle_yuv as yuv
from helpers import maxdiff
from test_gpu_ingest_formats import NV12_BOUND, NV12_CASES, _nets, _saturated_frame, _u8_clip

pytestmark = pytest.mark.gpu

# NV12_CASES = (N, H, W, h, w, luma pad, chroma pad (columns), strided batch), and the same shapes on plane views that start one sample into
# their buffer (pointers not 4-byte aligned: the per-pixel kernel for every format -- tight P010 rows are always 4-byte multiples)
CASES = [c + (False,) for c in NV12_CASES] + [(1, 36, 48, 18, 24, 0, 0, False, True), (1, 20, 32, 20, 32, 0, 0, False, True), (2, 24, 40, 12, 20, 8, 4, False, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _place(a, pad, offset, dev):
    """numpy plane [N,H,W(,2)] -> device view of the same shape: rows ``pad`` columns longer and / or starting one sample into the buffer
    (all filler bits set: must not be read)."""
    fill = np.iinfo(a.dtype).max
    buf = np.full(a.shape[:2] + (a.shape[2] + pad,) + a.shape[3:], fill, dtype=a.dtype)
    buf[:, :, :a.shape[2]] = a
    if not offset:
        return torch.from_numpy(buf).to(dev)[:, :, :a.shape[2]]
    flat = torch.from_numpy(np.concatenate([np.full(1, fill, a.dtype), buf.reshape(-1)])).to(dev)
    return flat[1:].view(buf.shape)[:, :, :a.shape[2]]


def _frames(fmt, planes, pl, pc, strided, offset, dev, name="bt709", full=False, mean=None, std=None):
    from arseg_amd import ingest

    mean, std = (ingest.CAMVID_MEAN, ingest.CAMVID_STD) if mean is None else (mean, std)
    t = [_place(p, pl if i == 0 else pc, offset, dev) for i, p in enumerate(planes)]
    if strided:
        t = [p[::2] for p in t]
    d = getattr(ingest.DecodedFrames, fmt)(*t, mean, std, matrix=name, full_range=full)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(d.planes, t))          # views, not copies
    return d


def _random_planes(fmt, g, n, H, W):
    """Random samples that use the format's whole depth; junk in the bits the format ignores (low 6 of P010, high 6 of I010)."""
    if fmt == "i420":
        return [g.integers(0, 256, s, dtype=np.uint8) for s in ((n, H, W), (n, H // 2, W // 2), (n, H // 2, W // 2))]
    if fmt == "i010":
        return [(g.integers(0, 1024, s, dtype=np.uint16) | (g.integers(0, 64, s, dtype=np.uint16) << 10)) for s in ((n, H, W), (n, H // 2, W // 2), (n, H // 2, W // 2))]
    return [((g.integers(0, 1024, s, dtype=np.uint16) << 6) | g.integers(0, 64, s, dtype=np.uint16)) for s in ((n, H, W), (n, H // 2, W // 2, 2))]


def _from_bytes(fmt, y, uv, g=None, top=False):
    """The picture of NV12 bytes (y, uv) in ``fmt``: 10-bit codes = 4 x the bytes (``top``: byte 255 -> code 1023), junk in the ignored bits."""
    if fmt == "i420":
        return [y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])]
    up = lambda a: np.where(a == 255, 1023, a.astype(np.uint16) * 4).astype(np.uint16) if top else a.astype(np.uint16) * 4
    y4, uv4 = up(y), up(uv)
    if fmt == "i010":
        j = (lambda s: g.integers(0, 64, s, dtype=np.uint16) << 10) if g is not None else (lambda s: np.uint16(0))
        return [y4 | j(y4.shape), np.ascontiguousarray(uv4[..., 0]) | j(uv4.shape[:-1]), np.ascontiguousarray(uv4[..., 1]) | j(uv4.shape[:-1])]
    j = (lambda s: g.integers(0, 64, s, dtype=np.uint16)) if g is not None else (lambda s: np.uint16(0))
    return [(y4 << 6) | j(y4.shape), (uv4 << 6) | j(uv4.shape)]


@pytest.mark.parametrize("name,full", oracle.COLOURS)
@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_against_oracle(dev, fmt, name, full):
    """Each format -> fp32 NHWC4 against the fp64 oracle (tests/ingest_oracle_yuv.py) for one colour enum over CASES on random samples that use
    every bit of the depth, and on the frame with saturated corners (identity and downscale) so that the clip is exercised.  Bound: NV12_BOUND,
    the 1e-5 the RGB8 arithmetic is held to.  Measured on MI355X: worst 6.0e-7 for each of the three formats (BT.601 limited); per format
    and enum in DESIGN.md section 6.3."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(77))
    runs = []
    for (N, H, W, h, w, pl, pc, strided, offset) in CASES:
        runs.append((_random_planes(fmt, g, 2 * N if strided else N, H, W), h, w, pl, pc, strided, offset))
    ys, uvs = _saturated_frame(32, 40)
    sat = _from_bytes(fmt, ys, uvs, g, top=True)
    runs += [(sat, 32, 40, 0, 0, False, False), (sat, 16, 20, 0, 0, False, False), (sat, 16, 20, 0, 0, False, True)]
    worst, clipped = 0.0, 0
    for (planes, h, w, pl, pc, strided, offset) in runs:
        d = _frames(fmt, planes, pl, pc, strided, offset, dev, name, full)
        got = d.to_input(h, w, torch.float32)
        used = [p[::2] for p in planes] if strided else planes
        want = yuv.ingest_yuv(fmt, used, h, w, ingest.CAMVID_MEAN, ingest.CAMVID_STD, name, full)
        assert got.shape == want.shape[:3] + (4,) and float(got[..., 3].abs().max()) == 0.0
        e = maxdiff(got[..., :3], want)
        rgb = yuv.yuv_to_rgb(fmt, used, name, full)
        clipped += int(((rgb == 0.0) | (rgb == 255.0)).sum())
        print(f"\n{fmt} {name} {'full' if full else 'limited'} {tuple(planes[0].shape)} -> {h}x{w} pads {pl}/{pc} offset {offset}: max |err| = {e:.3e}")
        worst = max(worst, e)
    print(f"{fmt} {name} {'full' if full else 'limited'}: worst max |err| = {worst:.3e} (bound {NV12_BOUND:.1e}); clipped oracle samples: {clipped}")
    assert clipped > 0
    assert worst <= NV12_BOUND


@pytest.mark.parametrize("name", ["bt601", "bt709"])
def test_same_values_same_bits(dev, name):
    """For equal sample values every instantiation of the one kernel family gives the same fp32 bits (fp contract off, explicit fma): I420, I010
    and P010 holding one picture (10-bit codes = 4 x the bytes, limited range: the factor 4 is exact through every fp32 step of the contract),
    each on its aligned planes (row-staged kernel where the case allows) and on views one sample into their buffer (per-pixel kernel), and NV12
    on the same bytes: the same picture gives the same network input whatever layout the decoder delivered it in."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(78))
    for (N, H, W, h, w, pl, pc, strided, _) in CASES[:len(NV12_CASES)]:
        n_all = 2 * N if strided else N
        y, uv = g.integers(0, 256, (n_all, H, W), dtype=np.uint8), g.integers(0, 256, (n_all, H // 2, W // 2, 2), dtype=np.uint8)
        outs = {}
        for fmt in yuv.FORMATS:
            planes = _from_bytes(fmt, y, uv, g)
            for offset in (False, True):
                outs[(fmt, offset)] = _frames(fmt, planes, pl, pc, strided, offset, dev, name, False).to_input(h, w, torch.float32)
        yd, ud = _place(y, pl, False, dev), _place(uv, pc, False, dev)
        if strided:
            yd, ud = yd[::2], ud[::2]
        outs[("nv12", False)] = ingest.DecodedFrames.nv12(yd, ud, ingest.CAMVID_MEAN, ingest.CAMVID_STD, matrix=name, full_range=False).to_input(h, w, torch.float32)
        first = outs[("i420", False)]
        for key, o in outs.items():
            assert torch.equal(o, first), (key, (N, H, W, h, w, pl, pc, strided), maxdiff(o, first))
        print(f"\n{name} limited {(N, H, W)} -> {h}x{w} pads {pl}/{pc}: seven routes bit-equal")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("H,W,h,w", [(64, 1200, 32, 600), (36, 48, 18, 24), (34, 46, 17, 23), (20, 32, 20, 32)])
def test_16bit_equals_rounded_fp32(dev, dtype, fmt, H, W, h, w):
    """fp16 / bf16 NHWC8 output == the fp32 output rounded to the storage type, by the rule of test_16bit_equals_rounded_fp32
    (tests/test_gpu_ingest_formats.py): within one unit of the storage type everywhere, < 1e-3 of the elements rounded differently, padding
    channels exactly 0.  With contraction off the three output types share their arithmetic up to the store.  Measured on MI355X: fraction 0
    for bf16 in every case and for fp16 in all but the 64x1200 case (2 or 3 of 115200 elements, 1.7e-5 to 2.6e-5)."""
    g = np.random.Generator(np.random.PCG64(91))
    d = _frames(fmt, _random_planes(fmt, g, 2, H, W), 0, 0, False, False, dev)
    got = d.to_input(h, w, dtype)
    ref = d.to_input(h, w, torch.float32)
    assert got.shape == (2, h, w, 8) and got.dtype == dtype
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    assert bool(((got[..., :3].float() - ref[..., :3]).abs() <= ulp * ref[..., :3].abs() + 1e-7).all())
    frac = float((got[..., :3].float() != ref[..., :3].to(dtype).float()).float().mean())
    print(f"\n{fmt} {H}x{W} -> {h}x{w} {dtype}: fraction rounded differently from the fp32 output = {frac:.3e}")
    assert frac < 1e-3
    assert float(got[..., 3:].float().abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_end_to_end_decoded_frames(dev, manifest, kind):
    """CamVid PSPNet fp32 and BiSeNet bf16, weights and clip as test_end_to_end_decoded_frames (tests/test_gpu_ingest_formats.py) builds them:
    forward_keyframe, alter_res_batch_pred and alter_res_batch_fast fed I420, P010 and I010 of ONE picture (10-bit codes = 4 x the bytes) give
    the same logits and labels, bit for bit.  Against the NV12-fed run the label agreement is printed (the ingest output is bit-equal:
    test_same_values_same_bits).  True 10-bit P010 from rgb_to_yuv420: finite outputs, label agreement with the RGB8-fed run printed.
    Measured on MI355X: DESIGN.md section 6.3."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, synth

    hr, lr = _nets(manifest, dev, kind)
    H, W = (64, 96) if kind == "psp" else (128, 256)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    clip = synth.make_clip(9, H, W, gop=4, mean=mean, std=std)
    u8 = _u8_clip(clip, mean, std)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    y, uv = ingest.rgb_to_nv12(u8, "bt709", False)
    src = {fmt: _frames(fmt, _from_bytes(fmt, y, uv), 0, 0, False, False, dev, "bt709", False, mean, std) for fmt in yuv.FORMATS}
    src["nv12"] = ingest.DecodedFrames.nv12(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev), mean, std, matrix="bt709", full_range=False)
    src["rgb8"] = ingest.DecodedFrames.rgb8(torch.from_numpy(u8).to(dev), mean, std)
    src["p010_true"] = _frames("p010", list(ingest.rgb_to_yuv420(u8, "p010", "bt709", False)), 0, 0, False, False, dev, "bt709", False, mean, std)
    res = {}
    with torch.no_grad():
        for tag, s in src.items():
            out_k, feat_k = hr.forward_keyframe(s[0:1])
            pred, _ = ev.alter_res_batch_pred(lr, [feat_k[0]] * 3, s[1:4], mvs[1:4], 0.5)
            out_b, _ = ev.alter_res_batch_fast(lr, [feat_k[0]] * 3, s[1:4], mvs[1:4], 0.5)
            res[tag] = (out_k, pred, out_b)
    for tag in ("p010", "i010"):
        for a, b in zip(res[tag], res["i420"]):
            assert a.shape == b.shape and torch.equal(a, b), tag
    agree = lambda a, b: float((a == b).float().mean())
    for a in res["i420"] + res["p010_true"]:
        assert bool(torch.isfinite(a.float()).all())
    assert res["i420"][0].shape[-2:] == (H, W) and res["p010_true"][1].shape == res["rgb8"][1].shape
    print(f"\n[{kind}] I420 = P010 = I010 (one picture) bit for bit; vs the NV12-fed run: labels equal {agree(res['i420'][0].argmax(1), res['nv12'][0].argmax(1)):.4f} (keyframe) "
          f"{agree(res['i420'][1], res['nv12'][1]):.4f} (non-keyframes)")
    print(f"[{kind}] true 10-bit P010 (bt709 limited, 2x2 box chroma) vs RGB8: labels equal {agree(res['p010_true'][0].argmax(1), res['rgb8'][0].argmax(1)):.4f} (keyframe) "
          f"{agree(res['p010_true'][1], res['rgb8'][1]):.4f} (non-keyframes); 8-bit NV12 vs RGB8: {agree(res['nv12'][0].argmax(1), res['rgb8'][0].argmax(1)):.4f} "
          f"{agree(res['nv12'][1], res['rgb8'][1]):.4f}")


def test_evaluator_and_runner_take_the_new_decoded_frames(dev, manifest):
    """EvalAlterRes, EvalByDistance and GopRunner.run_batched fed DecodedFrames.i420 / p010 / i010 (host planes for the evaluators, as a
    dataset would hand them over; device planes for the runner): one keyframe forward per pass with the cache (16-bit planes compare equal
    across samples), the same mIoU / table / logits from the three formats of one picture, the sub-batched pass slices them."""
    import test_gpu_models as tm
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, ops, synth
    from arseg_amd.gop import GopRunner

    hr, lr = tm._psp(manifest, dev, False), tm._psp(manifest, dev, True)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    clip = synth.make_clip(6, 48, 64, gop=5, mean=mean, std=std)
    u8 = _u8_clip(clip, mean, std)
    mvs = torch.from_numpy(clip["mv"])
    g = np.random.Generator(np.random.PCG64(3))
    labels = torch.from_numpy(g.integers(0, 12, (5, 48, 64)).astype(np.int64))
    y, uv = ingest.rgb_to_nv12(u8, "bt709", False)
    decs = {fmt: getattr(ingest.DecodedFrames, fmt)(*[torch.from_numpy(np.ascontiguousarray(p)) for p in _from_bytes(fmt, y, uv)], mean, std) for fmt in yuv.FORMATS}
    mious, tables, outs = {}, {}, {}
    with torch.no_grad():
        for fmt, dec in decs.items():
            assert not dec.is_cuda
            dl = [(dec[d], labels[d:d + 1], None, dec[0], mvs[d:d + 1]) for d in range(1, 5)]
            e = ev.EvalAlterRes(scale=0.5, cache_keyframe=True)
            mious[fmt] = e(hr, lr, dl, 12)
            assert e.hr_forwards == 1 and 0.0 <= mious[fmt] <= 1.0
            t = ev.EvalByDistance(scale=0.5, gop=5, cache_keyframe=True)
            tables[fmt] = t(hr, lr, [(dec[0], labels[0:1], None)] + [s + (d,) for d, s in zip(range(1, 5), dl)], 12)
            assert tuple(tables[fmt].hist.shape) == (5, 12, 12) and all(int(tables[fmt].hist[d].sum()) == 48 * 64 for d in range(5))
            dd = dec.cuda()
            runner = GopRunner(lambda k: hr.forward_keyframe(k)[1][0], lambda ref, img, mv: ev.alter_res_step_fast(lr, ref.unsqueeze(0), img, mv, 0.5)[0], n_gops=1, gop=5)
            batch = lambda refs, imgs, mv: ev.alter_res_batch_fast(lr, refs, imgs, mv, 0.5)[0]
            outs[fmt] = runner.run_batched({0: dd[0]}, dd[1:5], mvs[1:5].to(dev), batch)
            assert outs[fmt].shape == (4, 12, 48, 64) and bool(torch.isfinite(outs[fmt]).all())
            prev = ops.configure(lr_subbatch=2)            # the sub-batched pass slices the frames along the batch axis
            try:
                out_s = batch([hr.forward_keyframe(dd[0])[1][0]] * 4, dd[1:5], mvs[1:5].to(dev))
            finally:
                ops.configure(**prev)
            assert maxdiff(out_s, outs[fmt]) <= 2e-4
    print(f"\nEvalAlterRes mIoU from I420 / P010 / I010 frames: {mious}")
    for fmt in ("p010", "i010"):
        assert mious[fmt] == mious["i420"] and torch.equal(tables[fmt].hist, tables["i420"].hist) and torch.equal(outs[fmt], outs["i420"])


def test_graph_capture_replays_refilled_planes(dev, manifest):
    """A GopGraph (one lane, independent) over a closure that holds DecodedFrames.i420 on static plane tensors: refill the planes in place
    with copy_ from a second clip, replay -- the output equals the eager result on the second clip bit for bit (the ingest kernel reads the
    planes it was captured with; nothing of the frames is baked into the graph)."""
    import test_gpu_models as tm
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, synth
    from arseg_amd.executor import GopGraph

    hr, lr = tm._psp(manifest, dev, False), tm._psp(manifest, dev, True)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    H, W = 64, 96

    def planes_of(seed):
        clip = synth.make_clip(seed, H, W, gop=4, mean=mean, std=std)
        return [torch.from_numpy(p).to(dev) for p in ingest.rgb_to_yuv420(_u8_clip(clip, mean, std), "i420")], torch.from_numpy(clip["mv"]).to(dev)

    (p1, mv1), (p2, mv2) = planes_of(12), planes_of(13)
    static, mv = [p.clone() for p in p1], mv1.clone()
    frames = ingest.DecodedFrames.i420(*static, mean, std)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(frames.planes, static))

    def step_on(f, m):
        _, ref = hr.forward_keyframe(f[0:1])
        return ev.alter_res_batch_fast(lr, [ref[0]] * 3, f[1:4], m[1:4], 0.5)[0]

    with torch.no_grad():
        want1 = step_on(ingest.DecodedFrames.i420(*p1, mean, std), mv1).clone()
        want2 = step_on(ingest.DecodedFrames.i420(*p2, mean, std), mv2).clone()
        assert not torch.equal(want1, want2)
        graph = GopGraph([lambda: step_on(frames, mv)], warmup=1, independent=True)
        out = graph.replay()[0]
        torch.cuda.synchronize()
        assert torch.equal(out, want1)
        for s, p in zip(static, p2):
            s.copy_(p)
        mv.copy_(mv2)
        out = graph.replay()[0]
        torch.cuda.synchronize()
        assert torch.equal(out, want2)
