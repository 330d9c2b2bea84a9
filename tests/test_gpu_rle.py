"""GPU checks of the run-length codes (csrc/rle.hip, arseg_labels_rle_fwd / arseg_rle_decode_fwd; arseg_amd.egress.rle): row_start and the
run words against the numpy oracle written from the contract (tests/rle_oracle.py), the decoder against the planes, the fused form
against the EXISTING evaluator tail (ops.argmax_confusion).  Every output is an integer: every comparison is np.array_equal."""
import numpy as np
import pytest
import torch

import consistency_oracle
import rle_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GW = oracle.GUARD_WORD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _row_planes(seed, N, H, W):
    """Planes for the width / height sweeps: rows of random runs (mean length about 5), every third row constant, every third row a new
    value at almost every pixel."""
    g = np.random.Generator(np.random.PCG64(seed))
    p = np.empty((N, H, W), dtype=np.uint8)
    for n in range(N):
        for y in range(H):
            if (y + n) % 3 == 1:
                p[n, y] = g.integers(0, 256)
            elif (y + n) % 3 == 2:
                p[n, y] = g.integers(0, 3, W) * 127
            else:
                p[n, y] = np.repeat(g.integers(0, 256, W), g.integers(1, 10, W))[:W]
    return p


def _encode(dev, plane_t, cap, extra=8):
    """ops.labels_rle into a garbage-filled row_start and a guarded run buffer [N,cap] followed by ``extra`` guard words ->
    (row_start numpy, runs numpy uint32 [N,cap], tail guard numpy, the device tensors)."""
    from arseg_amd import ops

    N, H, _ = plane_t.shape
    row_start = torch.full((N, H + 1), -7, dtype=torch.int32, device=dev)
    backing = torch.from_numpy(np.full(N * cap + extra, GW, dtype=np.uint32).view(np.int32)).to(dev)
    runs = backing[:N * cap].view(N, cap)
    ops.labels_rle(plane_t, row_start, runs)
    b = backing.cpu().numpy().view(np.uint32)
    return row_start.cpu().numpy(), b[:N * cap].reshape(N, cap), b[N * cap:], (row_start, runs)


def _check_encoded(planes, got_start, got_runs, tail, cap):
    """row_start exact; per frame the words below min(cap, needed) exact and the words from needed to cap still guards; the tail intact."""
    want_start, want_runs = oracle.encode(planes)
    assert np.array_equal(got_start, want_start)
    for n, w in enumerate(want_runs):
        k = min(len(w), cap)
        assert np.array_equal(got_runs[n, :k], w[:k])
        assert (got_runs[n, k:] == GW).all()
    assert (tail == GW).all()
    return want_start, want_runs


def _round_trip(dev, planes, cap=None):
    """encode (capacity = the most a plane can need unless given) against the oracle, then decode over a 0xA5 prefill against the plane."""
    from arseg_amd import ops

    N, H, W = planes.shape
    t = torch.from_numpy(planes).to(dev)
    cap = H * W if cap is None else cap
    got_start, got_runs, tail, (row_start, runs) = _encode(dev, t, cap)
    _check_encoded(planes, got_start, got_runs, tail, cap)
    out = torch.full((N, H, W), GUARD, dtype=torch.uint8, device=dev)
    ops.rle_decode(row_start, runs, out)
    assert np.array_equal(out.cpu().numpy(), planes)


@pytest.mark.parametrize("W", [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025])
def test_widths_around_a_piece_and_a_wave_pass(dev, W):
    """One lane piece (16 pixels), one pass of a wave (1024 pixels), and one more or less of each."""
    _round_trip(dev, _row_planes(300 + W, 2, 3, W))


@pytest.mark.parametrize("H", [1, 255, 256, 257, 1025])
def test_heights_around_the_scan_chunk(dev, H):
    """The prefix over the rows works in chunks of 256 entries with a carry."""
    _round_trip(dev, _row_planes(500 + H, 2, H, 16))


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_seeded_blob_planes(dev, case):
    _round_trip(dev, oracle.build(case))


@pytest.mark.parametrize("hand", oracle.HAND, ids=oracle.HAND_IDS)
def test_hand_made_rows(dev, hand):
    """Against the words written out by hand (not against the oracle)."""
    plane = oracle.hand_plane(hand)
    got_start, got_runs, tail, _ = _encode(dev, torch.from_numpy(plane).to(dev), len(hand[3]) + 2)
    assert got_start[0].tolist() == hand[2] and got_runs[0].tolist() == hand[3] + [GW, GW] and (tail == GW).all()
    _round_trip(dev, plane)


@pytest.mark.parametrize("pitch", ["odd", "aligned", "odd-image-stride"])
def test_pitched_planes_and_a_frame_slice(dev, pitch):
    """The plane as a [1:3] slice of a pitched, guarded buffer (an odd pitch: rows start at every alignment; a 4-byte aligned one; an odd
    pitch with an image stride that is no multiple of the pitch): the code equals the dense planes', the buffer is unchanged; and the
    decoder writes such a slice back without touching a guard byte or frame 0."""
    from arseg_amd import ops

    planes = oracle.build(oracle.CASES[1])
    N, H, W = planes.shape
    pad = 3 if pitch.startswith("odd") else 4
    assert (W + pad) % 2 == 1 if pad == 3 else (W + pad) % 4 == 0
    rows = H + (0 if pitch != "odd-image-stride" else 1)                   # image stride = (H + 1) rows: odd x even + ... any parity
    buf = np.full((N + 1, rows, W + pad), GUARD, dtype=np.uint8)
    buf[:N, :H, :W] = planes
    backing = torch.from_numpy(buf).to(dev)
    view = backing[1:3, :H, :W]
    got_start, got_runs, tail, (row_start, runs) = _encode(dev, view, H * W // 2)
    _check_encoded(planes[1:3], got_start, got_runs, tail, H * W // 2)
    assert np.array_equal(backing.cpu().numpy(), buf)
    out_buf = np.full_like(buf, GUARD)
    out_buf[:N, :H, :W] = 9
    out = torch.from_numpy(out_buf).to(dev)
    ops.rle_decode(row_start, runs, out[1:3, :H, :W])
    want = out_buf.copy()
    want[1:3, :H, :W] = planes[1:3]
    assert np.array_equal(out.cpu().numpy(), want)


def test_overflow(dev):
    """cap = needed, needed - 1, needed // 2 and 0 (needed: of the frame that needs most): row_start stays exact, the words below cap are
    exact, nothing from cap on is written; runs=None gives the same row_start; decoding the cut buffer leaves exactly the uncovered pixels."""
    from arseg_amd import ops

    planes = oracle.build(oracle.CASES[1])
    N, H, W = planes.shape
    t = torch.from_numpy(planes).to(dev)
    want_start, want_runs = oracle.encode(planes)
    needed = max(len(w) for w in want_runs)
    assert min(len(w) for w in want_runs) < needed
    for cap in (needed, needed - 1, needed // 2, 0):
        got_start, got_runs, tail, (row_start, runs) = _encode(dev, t, cap)
        _check_encoded(planes, got_start, got_runs, tail, cap)
        assert [int(k) > cap for k in got_start[:, H]] == [len(w) > cap for w in want_runs]
        out = torch.full((N, H, W), GUARD, dtype=torch.uint8, device=dev)
        ops.rle_decode(row_start, runs, out)
        got = out.cpu().numpy()
        for n in range(N):
            want = oracle.decode(want_start[n], want_runs[n][:cap], H, W, np.full((H, W), GUARD, np.uint8))
            assert np.array_equal(got[n], want)
            assert (want != planes[n]).any() == (len(want_runs[n]) > cap)
    sizing = torch.full((N, H + 1), -7, dtype=torch.int32, device=dev)
    ops.labels_rle(t, sizing)
    assert np.array_equal(sizing.cpu().numpy(), want_start)


def test_two_runs_are_bit_equal(dev):
    planes = torch.from_numpy(oracle.build(oracle.CASES[1])).to(dev)
    a = _encode(dev, planes, 2000)
    b = _encode(dev, planes, 2000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _logits_case(dev, case):
    from arseg_amd import ops

    b = consistency_oracle.build(case)
    logits = torch.from_numpy(b["logits"]).to(dev)
    pred = ops.argmax_confusion(logits, None, case[6], case[7], align_corners=case[8])[0].cpu().numpy()
    return logits, pred


@pytest.mark.parametrize("case", [consistency_oracle.CASES[0], consistency_oracle.CASES[1], consistency_oracle.CASES[4]], ids=lambda c: c[0])
def test_fused_form_against_the_tail(dev, case):
    """egress.rle(logits, ...).decode() equals ops.argmax_confusion's pred on the same-size, the bilinear and the x8 run route; with a lut it
    equals lut[pred]; to_host() and rle_decode_numpy give the same planes on the host."""
    from arseg_amd import egress

    _, _, N, n_cls, h, w, H, W, align, _ = case
    logits, pred = _logits_case(dev, case)
    frames = egress.rle(logits, H, W, H * W, align_corners=align)
    assert isinstance(frames, egress.RleFrames) and tuple(frames.labels.shape) == (N, H, W)
    assert np.array_equal(frames.decode().cpu().numpy(), pred) and np.array_equal(frames.labels.cpu().numpy(), pred)
    want_start, want_runs = oracle.encode(pred.astype(np.uint8))
    assert frames.needed().cpu().tolist() == [len(r) for r in want_runs]
    for n, (rs, words) in enumerate(frames.to_host()):
        assert np.array_equal(rs, want_start[n]) and np.array_equal(words, want_runs[n])
        assert np.array_equal(egress.rle_decode_numpy(rs, words, H, W), pred[n])
    lut = np.random.Generator(np.random.PCG64(2)).integers(0, 256, n_cls, dtype=np.uint8)
    mapped = egress.rle(logits, H, W, H * W, lut=lut, align_corners=align)
    assert np.array_equal(mapped.decode().cpu().numpy(), lut[pred])


def test_rle_in_one_graph(dev):
    """labels8 + encode captured once (labels_out and out given: nothing is allocated); the logits are refilled in place; each replay
    equals the oracle for its own logits, and the two replays need different numbers of runs."""
    from arseg_amd import egress, ops

    case = consistency_oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align, _ = case
    logits = torch.from_numpy(consistency_oracle.build(case)["logits"]).to(dev)
    cap = H * W // 2
    labels = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    out = egress.RleFrames(torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev), H, W)
    egress.rle(logits, H, W, cap, labels_out=labels, out=out, align_corners=align)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        egress.rle(logits, H, W, cap, labels_out=labels, out=out, align_corners=align)
    totals = []
    for s in (seed + 60, seed + 61):
        fresh = torch.from_numpy(consistency_oracle.build((case[0], s) + case[2:])["logits"]).to(dev)
        logits.copy_(fresh)
        labels.zero_()
        out.row_start.fill_(-7)
        out.runs.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        pred = ops.argmax_confusion(fresh, None, H, W, align_corners=align)[0].cpu().numpy().astype(np.uint8)
        want_start, want_runs = oracle.encode(pred)
        assert np.array_equal(labels.cpu().numpy(), pred) and np.array_equal(out.row_start.cpu().numpy(), want_start)
        for n, (_, words) in enumerate(out.to_host()):
            assert np.array_equal(words, want_runs[n])
        totals.append(int(want_start[:, H].sum()))
    assert totals[0] != totals[1]


def test_alter_res_batch_rle(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_rle's runs decode to alter_res_batch_render's planes."""
    import test_gpu_ingest_formats as tf          # its _nets wraps test_gpu_models' _psp (+ storage)
    from arseg_amd import synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop = 64, 96, 4
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"][1:gop]).to(dev)
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * (gop - 1)
        labels_r, _ = ev.alter_res_batch_render(lr, refs, frames[1:gop], mvs, 0.5)
        coded, labels = ev.alter_res_batch_rle(lr, refs, frames[1:gop], mvs, H * W, 0.5)
    assert torch.equal(labels, labels_r) and torch.equal(coded.decode(), labels_r)
    want_start, want_runs = oracle.encode(labels_r.cpu().numpy())
    print(f"\nruns per frame {want_start[:, H].tolist()} of {H * W} pixels")
    for n, (rs, words) in enumerate(coded.to_host()):
        assert np.array_equal(rs, want_start[n]) and np.array_equal(words, want_runs[n])


def test_full_size_frame_round_trips(dev):
    """One 1024x2048 frame of blob-like labels (19 classes, low-resolution noise resized on the device): the code equals the oracle's for
    the plane as it came out, and decodes to it."""
    from arseg_amd import egress

    H, W = 1024, 2048
    g = np.random.Generator(np.random.PCG64(77))
    low = torch.from_numpy(consistency_oracle.make_logits(g, 1, 19, 32, 64)).to(dev)
    plane = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).argmax(dim=1).to(torch.uint8)
    ref = plane.cpu().numpy()
    want_start, want_runs = oracle.encode(ref)
    needed = len(want_runs[0])
    coded = egress.rle_of_planes(plane, needed + 16)
    assert int(coded.needed()[0]) == needed and H < needed < H * W // 16
    rs, words = coded.to_host()[0]
    assert np.array_equal(rs, want_start[0]) and np.array_equal(words, want_runs[0])
    assert np.array_equal(coded.decode().cpu().numpy(), ref)
