"""GPU checks of the 8-bit frame ingest (csrc/ingest.hip, arseg_frame_ingest_fwd) and of the fast paths fed with ingest.DecodedFrames."""
import numpy as np
import pytest
import torch

import ingest_oracle as oracle
from helpers import maxdiff

pytestmark = pytest.mark.gpu

# NV12 -> fp32 against the fp64 oracle: max |error| of the normalised output.  Measured on MI355X over the cases of test_nv12_against_oracle
# (worst per colour enum 6.0e-7 / 4.2e-7 / 5.2e-7 / 4.2e-7: DESIGN.md section 6.3), all inside the 1e-5 the RGB8 arithmetic is held to, so that bound is kept.
NV12_BOUND = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _padded(a, pad, dev):
    """numpy [N,H,W,...] -> device view of the same shape whose rows are ``pad`` elements of axis 2 longer (filled with 255: must not be read)."""
    buf = np.full(a.shape[:2] + (a.shape[2] + pad,) + a.shape[3:], 255, dtype=a.dtype)
    buf[:, :, :a.shape[2]] = a
    return torch.from_numpy(buf).to(dev)[:, :, :a.shape[2]]


@pytest.mark.parametrize("H,W,h,w,pad", [(36, 48, 18, 24, 0), (35, 47, 17, 23, 0), (20, 30, 20, 30, 0), (512, 1024, 256, 512, 32), (512, 1024, 512, 1024, 0),
                                         (40, 1200, 20, 600, 4), (20, 24, 30, 36, 0)])
def test_rgb8_fp32_equals_existing_u8_ingest(dev, H, W, h, w, pad):
    """RGB8 -> fp32 NHWC4 == ingest.frames_to_nhwc4 (the existing uint8 kernel, pinned to the oracle by test_frame_u8_ingest) within the 1e-5
    that test uses for the same arithmetic; row-staged kernel (4-byte aligned rows), per-pixel kernel (47-pixel rows: 141-byte pitch), a
    padded pitch, identity size, several 256-pixel segments per row, an upscale.  Padding channel exactly 0."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(61))
    img = g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    want = ingest.frames_to_nhwc4(img, h, w, ingest.CITY_BISE_MEAN, ingest.CITY_BISE_STD, device=dev)
    src = _padded(img, pad, dev) if pad else torch.from_numpy(img).to(dev)
    d = ingest.DecodedFrames.rgb8(src, ingest.CITY_BISE_MEAN, ingest.CITY_BISE_STD)
    assert d.planes[0].data_ptr() == src.data_ptr()                  # the padded view itself, not a copy
    got = d.to_input(h, w, torch.float32)
    assert got.shape == (2, h, w, 4) and got.dtype == torch.float32 and float(got[..., 3].abs().max()) == 0.0
    e = maxdiff(got, want)
    print(f"\nRGB8 {H}x{W} -> {h}x{w} pad {pad}: max |new - existing| = {e:.3e}")
    assert e <= 1e-5
    ref = oracle.ingest(img, h, w, ingest.CITY_BISE_MEAN, ingest.CITY_BISE_STD)
    assert maxdiff(got[..., :3], ref) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("src", ["rgb8", "nv12"])
@pytest.mark.parametrize("H,W,h,w", [(64, 1200, 32, 600), (36, 48, 18, 24), (35, 47, 17, 23), (20, 32, 20, 32)])
def test_16bit_equals_rounded_fp32(dev, dtype, src, H, W, h, w):
    """fp16 / bf16 NHWC8 output == the fp32 output rounded to the storage type, by the rule of test_frame_ingest_16bit_equals_rounded_fp32
    (tests/test_gpu_16bit.py): within one unit of the storage type everywhere (contraction is off in csrc/ingest.hip: the output types share their arithmetic up to the store), the same
    rounding nearly always (< 1e-3 of the elements differ), padding channels exactly 0."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(91))
    if src == "nv12":
        H, W = H + H % 2, W + W % 2
        d = ingest.DecodedFrames.nv12(torch.from_numpy(g.integers(0, 256, (2, H, W), dtype=np.uint8)).to(dev),
                                      torch.from_numpy(g.integers(0, 256, (2, H // 2, W // 2, 2), dtype=np.uint8)).to(dev))
    else:
        d = ingest.DecodedFrames.rgb8(torch.from_numpy(g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)).to(dev))
    got = d.to_input(h, w, dtype)
    ref = d.to_input(h, w, torch.float32)
    assert got.shape == (2, h, w, 8) and got.dtype == dtype
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    assert bool(((got[..., :3].float() - ref[..., :3]).abs() <= ulp * ref[..., :3].abs() + 1e-7).all())
    assert float((got[..., :3].float() != ref[..., :3].to(dtype).float()).float().mean()) < 1e-3
    assert float(got[..., 3:].float().abs().max()) == 0.0


def _saturated_frame(H, W):
    """NV12 planes whose corners hold Y = 235 / 16 with extreme chroma (RGB far outside [0, 255] before the clip), noise elsewhere."""
    g = np.random.Generator(np.random.PCG64(33))
    y = g.integers(0, 256, (1, H, W), dtype=np.uint8)
    uv = g.integers(0, 256, (1, H // 2, W // 2, 2), dtype=np.uint8)
    q = 6
    for (ys, xs, yv, cb, cr) in ((slice(0, q), slice(0, q), 235, 240, 240), (slice(0, q), slice(W - q, W), 235, 16, 16),
                                 (slice(H - q, H), slice(0, q), 16, 240, 16), (slice(H - q, H), slice(W - q, W), 16, 0, 255)):
        y[0, ys, xs] = yv
        cy = slice(0, q // 2) if ys.start == 0 else slice(H // 2 - q // 2, H // 2)
        cx = slice(0, q // 2) if xs.start == 0 else slice(W // 2 - q // 2, W // 2)
        uv[0, cy, cx] = (cb, cr)
    return y, uv


NV12_CASES = [  # (N, H, W, h, w, luma pad, chroma pad (pairs), strided batch)
    (1, 36, 48, 18, 24, 0, 0, False),            # downscale, staged kernel
    (1, 20, 32, 20, 32, 0, 0, False),            # identity
    (2, 34, 46, 17, 23, 0, 0, False),            # width not a multiple of 16 (nor of 4: per-pixel kernel)
    (1, 36, 46, 18, 23, 2, 1, False),            # the same width on 4-byte aligned rows (staged kernel, partial last chunk of every row)
    (1, 36, 48, 18, 24, 16, 8, False),           # padded pitch, both planes
    (3, 24, 40, 12, 20, 8, 4, True),             # batch of 3 with an image stride (every other image of a batch of 6) and a pitch
    (1, 64, 1200, 32, 600, 0, 0, False),         # several 256-pixel segments per row
    (1, 16, 24, 24, 36, 0, 0, False),            # upscale
]


@pytest.mark.parametrize("name,full", oracle.COLOURS)
def test_nv12_against_oracle(dev, name, full):
    """NV12 -> fp32 NHWC4 against the fp64 oracle (tests/ingest_oracle.py) for one colour enum over NV12_CASES on random bytes, and on a frame
    with saturated corners (identity and downscale) so that the clip is exercised.  Bound: NV12_BOUND (see its comment)."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(77))
    worst = 0.0
    cases = []
    for (N, H, W, h, w, pl, pc, strided) in NV12_CASES:
        n_all = 2 * N if strided else N
        cases.append((g.integers(0, 256, (n_all, H, W), dtype=np.uint8), g.integers(0, 256, (n_all, H // 2, W // 2, 2), dtype=np.uint8), h, w, pl, pc, strided))
    ys, uvs = _saturated_frame(32, 40)
    cases += [(ys, uvs, 32, 40, 0, 0, False), (ys, uvs, 16, 20, 0, 0, False)]
    clipped = 0
    for (y, uv, h, w, pl, pc, strided) in cases:
        yd = _padded(y, pl, dev) if pl else torch.from_numpy(y).to(dev)
        ud = _padded(uv, pc, dev) if pc else torch.from_numpy(uv).to(dev)
        if strided:
            yd, ud, y, uv = yd[::2], ud[::2], y[::2], uv[::2]
        d = ingest.DecodedFrames.nv12(yd, ud, ingest.CAMVID_MEAN, ingest.CAMVID_STD, matrix=name, full_range=full)
        assert d.planes[0].data_ptr() == yd.data_ptr() and d.planes[1].data_ptr() == ud.data_ptr()          # views, not copies
        got = d.to_input(h, w, torch.float32)
        want = oracle.ingest_nv12(y, uv, h, w, ingest.CAMVID_MEAN, ingest.CAMVID_STD, name, full)
        assert got.shape == want.shape[:3] + (4,) and float(got[..., 3].abs().max()) == 0.0
        e = maxdiff(got[..., :3], want)
        rgb = oracle.nv12_to_rgb(y, uv, name, full)
        clipped += int(((rgb == 0.0) | (rgb == 255.0)).sum())
        print(f"\nNV12 {name} {'full' if full else 'limited'} {tuple(y.shape)} -> {h}x{w} pads {pl}/{pc}: max |err| = {e:.3e}")
        worst = max(worst, e)
    print(f"NV12 {name} {'full' if full else 'limited'}: worst max |err| = {worst:.3e} (bound {NV12_BOUND:.1e}); clipped oracle samples: {clipped}")
    assert clipped > 0
    assert worst <= NV12_BOUND


def _u8_clip(clip, mean, std):
    """The bytes behind synth.make_clip's frames (it quantises to k / 255 before normalising): uint8 [gop,H,W,3]."""
    f = clip["frames"].transpose(0, 2, 3, 1).astype(np.float64) * np.asarray(std) + np.asarray(mean)
    u8 = np.rint(f * 255.0)
    assert np.abs(f * 255.0 - u8).max() < 1e-3
    return u8.astype(np.uint8)


def _nets(manifest, dev, kind):
    import test_gpu_models as tm

    if kind == "psp":
        return tm._psp(manifest, dev, False), tm._psp(manifest, dev, True)
    return tm._bise(manifest, dev, False).set_storage(torch.bfloat16), tm._bise(manifest, dev, True).set_storage(torch.bfloat16)


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_float_input_takes_the_unchanged_path(dev, manifest, kind):
    """For float frames alter_res_batch_fast and forward_keyframe return the same bits as the sequence they ran before the 8-bit route
    existed, called by hand in the same process: ops.frame_ingest -> phase1_nhwc4 -> phase2_warp / the head."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth

    hr, lr = _nets(manifest, dev, kind)
    H, W = (64, 96) if kind == "psp" else (128, 256)
    clip = synth.make_clip(8, H, W, gop=4)
    frames, mvs = torch.from_numpy(clip["frames"]).to(dev), torch.from_numpy(clip["mv"]).to(dev)
    with torch.no_grad():
        out_k, feat_k = hr.forward_keyframe(frames[0:1])
        x = ops.frame_ingest(frames[0:1], H, W, hr.storage_dtype)
        if kind == "psp":
            _, p = hr.phase1_nhwc4(x, aux=False)
            want_k = hr._final(p, H, W)
        else:
            p = hr._trunk_nhwc4(x)[-1]
            want_k = hr.conv_out.head_nhwc(p)
        assert torch.equal(out_k, want_k) and torch.equal(feat_k, p)
        refs = [feat_k[0]] * 3
        out_b, p_b = ev.alter_res_batch_fast(lr, refs, frames[1:4], mvs[1:4], 0.5)
        feat = lr.phase1_nhwc4(ops.frame_ingest(frames[1:4], H // 2, W // 2, lr.storage_dtype), aux=ops.config.aux_outputs)[-1]
        want_b, want_p = lr.phase2_warp(feat, refs, mvs[1:4])
        assert torch.equal(out_b, want_b) and torch.equal(p_b, want_p)


# Label agreement of the NV12 run with the RGB8 run of the same clip.  4:2:0 halves the chroma resolution and Y, Cb, Cr are rounded to 8 bits,
# so the two runs see different frames; the figure is a property of synth.make_clip's texture and the synthetic weights, not of the kernel.
# Floors = the first measurement on MI355X -- PSPNet fp32 0.9919 (keyframe) / 0.9029 (non-keyframes), BiSeNet bf16 0.9896 / 0.9330 -- of the lower
# figure minus a 0.02 margin for plan-dependent conv arithmetic; they catch a broken colour route (a swapped matrix row drops agreement to chance).
NV12_AGREE_FLOOR = {"psp": 0.88, "bise": 0.91}


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_end_to_end_decoded_frames(dev, manifest, kind):
    """CamVid PSPNet fp32 and BiSeNet bf16, weights and clip as tests/test_gpu_models.py builds them: alter_res_batch_pred and forward_keyframe
    fed DecodedFrames.rgb8(clip bytes) against the same calls on the float frames those bytes normalise to.  fp32: logits within 1e-3.  bf16
    (both runs store bf16; their inputs differ where the two ingest kernels round a last bit differently): label agreement >= 0.99, the floor
    tests/test_gpu_16bit.py accepts for bf16 on this network.  NV12 of the same bytes: shapes, finiteness, label agreement with the RGB8 run
    above NV12_AGREE_FLOOR."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, synth
    from oracle import cpu_ref

    hr, lr = _nets(manifest, dev, kind)
    H, W = (64, 96) if kind == "psp" else (128, 256)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    clip = synth.make_clip(9, H, W, gop=4, mean=mean, std=std)
    u8 = _u8_clip(clip, mean, std)
    frames = cpu_ref.to_tensor_normalize(u8, mean, std).to(dev)
    assert maxdiff(frames, clip["frames"]) <= 1e-5
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    rgb = ingest.DecodedFrames.rgb8(torch.from_numpy(u8).to(dev), mean, std)
    y, uv = ingest.rgb_to_nv12(u8, "bt709", False)
    nv = ingest.DecodedFrames.nv12(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev), mean, std, matrix="bt709", full_range=False)
    res = {}
    with torch.no_grad():
        for tag, src in (("float", frames), ("rgb8", rgb), ("nv12", nv)):
            out_k, feat_k = hr.forward_keyframe(src[0:1])
            pred, _ = ev.alter_res_batch_pred(lr, [feat_k[0]] * 3, src[1:4], mvs[1:4], 0.5)
            out_b, _ = ev.alter_res_batch_fast(lr, [feat_k[0]] * 3, src[1:4], mvs[1:4], 0.5)
            res[tag] = (out_k.float(), pred, out_b.float())
    for tag in ("rgb8", "nv12"):
        for a, b in zip(res[tag], res["float"]):
            assert a.shape == b.shape and bool(torch.isfinite(a.float()).all())
    agree = lambda a, b: float((a == b).float().mean())
    k_agree, p_agree = agree(res["rgb8"][0].argmax(1), res["float"][0].argmax(1)), agree(res["rgb8"][1], res["float"][1])
    e_k, e_b = maxdiff(res["rgb8"][0], res["float"][0]), maxdiff(res["rgb8"][2], res["float"][2])
    print(f"\n[{kind}] RGB8 vs float frames: keyframe logits err {e_k:.3e}, non-keyframe logits err {e_b:.3e}, labels equal {k_agree:.4f} (keyframe) {p_agree:.4f} (non-keyframes)")
    if kind == "psp":
        assert e_k <= 1e-3 and e_b <= 1e-3
    else:
        assert k_agree >= 0.99 and p_agree >= 0.99
    nk, npred = agree(res["nv12"][0].argmax(1), res["rgb8"][0].argmax(1)), agree(res["nv12"][1], res["rgb8"][1])
    print(f"[{kind}] NV12 (bt709 limited, 2x2 box chroma) vs RGB8: labels equal {nk:.4f} (keyframe) {npred:.4f} (non-keyframes); floor {NV12_AGREE_FLOOR[kind]}")
    assert min(nk, npred) >= NV12_AGREE_FLOOR[kind]


def test_evaluator_and_runner_take_decoded_frames(dev, manifest):
    """EvalAlterRes and GopRunner fed DecodedFrames: the evaluator's mIoU from uint8 samples equals the one from the float frames of the same
    bytes (fp32 PSPNet: the logits agree to 1e-3, the labels of this clip do not move), the runner's batched schedule passes them through."""
    import test_gpu_models as tm
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, ops, synth
    from arseg_amd.gop import GopRunner
    from oracle import cpu_ref

    hr, lr = tm._psp(manifest, dev, False), tm._psp(manifest, dev, True)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    clip = synth.make_clip(6, 48, 64, gop=5, mean=mean, std=std)
    u8 = _u8_clip(clip, mean, std)
    frames = cpu_ref.to_tensor_normalize(u8, mean, std)
    mvs = torch.from_numpy(clip["mv"])
    g = np.random.Generator(np.random.PCG64(3))
    labels = torch.from_numpy(g.integers(0, 12, (5, 48, 64)).astype(np.int64))
    dec = ingest.DecodedFrames.rgb8(u8, mean, std)
    dl_f = [(frames[d:d + 1], labels[d:d + 1], None, frames[0:1], mvs[d:d + 1]) for d in range(1, 5)]
    dl_d = [(dec[d], labels[d:d + 1], None, dec[0], mvs[d:d + 1]) for d in range(1, 5)]
    with torch.no_grad():
        e = ev.EvalAlterRes(scale=0.5, cache_keyframe=True)
        m_f, m_d = e(hr, lr, dl_f, 12), e(hr, lr, dl_d, 12)
        assert e.hr_forwards == 2                      # one keyframe forward per pass: DecodedFrames compare equal across samples
        print(f"\nEvalAlterRes mIoU float {m_f:.6f} decoded {m_d:.6f}")
        assert abs(m_f - m_d) <= 1e-3
        dd, fd = dec.cuda(), frames.to(dev)
        runner = GopRunner(lambda k: hr.forward_keyframe(k)[1][0], lambda ref, img, mv: ev.alter_res_step_fast(lr, ref.unsqueeze(0), img, mv, 0.5)[0], n_gops=1, gop=5)
        batch = lambda refs, imgs, mv: ev.alter_res_batch_fast(lr, refs, imgs, mv, 0.5)[0]
        out_d = runner.run_batched({0: dd[0]}, dd[1:5], mvs[1:5].to(dev), batch)
        out_f = runner.run_batched({0: fd[0:1]}, fd[1:5], mvs[1:5].to(dev), batch)
        assert out_d.shape == out_f.shape == (4, 12, 48, 64) and maxdiff(out_d, out_f) <= 1e-3
        prev = ops.configure(lr_subbatch=2)            # the sub-batched pass slices the frames along the batch axis
        try:
            out_s = batch([hr.forward_keyframe(dd[0])[1][0]] * 4, dd[1:5], mvs[1:5].to(dev))
        finally:
            ops.configure(**prev)
        assert maxdiff(out_s, out_d) <= 2e-4
