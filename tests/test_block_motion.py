"""CPU checks of block motion estimation's host form (ingest.block_motion_numpy, ingest.luma8_numpy) against the loop oracle of
tests/block_motion_oracle.py, which is written from the definition in include/arseg_hip.h (arseg_block_motion_fwd).  Integers in, integers
out: every comparison is np.array_equal."""
import numpy as np
import pytest

import block_motion_oracle as oracle


def _numpy(cur, ref, **kw):
    from arseg_amd import ingest

    rec, sad, st = ingest.block_motion_numpy(cur, ref, **kw)
    assert rec.dtype == np.int16 and sad.dtype == np.uint32 and st.dtype == np.int64 and st.shape == (oracle.NSTATS,)
    return rec, sad, st


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("case", oracle.search_cases(), ids=oracle.case_id)
def test_numpy_form_equals_the_loop_oracle(case):
    kind, H, W, B, R, lam = case
    cur, ref = oracle.content(kind, H, W)
    winners = oracle.winners_of(*case)
    for intra in oracle.INTRAS:
        want = oracle.outputs(winners, intra)
        assert want[0].shape == (-(-H // B) * -(-W // B), 8)
        assert _same(_numpy(cur, ref, B=B, R=R, lam=lam, intra=intra), want), intra
    if kind == "constant":                                            # every candidate ties at SAD 0: rank 0, the zero vector
        assert all(w[4:] == (0, 0, 0) for w in winners)
    if kind == "stripes":                                             # the lowest rank among the ties: the smallest dy, then the smallest dx = 0 mod 4 ...
        assert all(w[6] == 0 for w in winners)
        if (H, W, R) == (37, 53, 6):                                   # ... unless (0, 0) ties too, which it always does here: rank 0 beats them all
            assert all(w[4:6] == (0, 0) for w in winners)


def test_rank_rule_decides_between_equal_costs():
    """Two candidates of equal cost and neither the zero vector: cur = ref shifted, on stripes of period 4, so dx = 1 and dx = -3 (and 5) both
    match with SAD 0 at every dy; at lam = 0 the smallest rank is dy = -R, dx = -3."""
    H, W, B, R = 16, 32, 8, 6
    row = np.where(np.arange(W + 8) % 4 < 2, 40, 200).astype(np.uint8)
    ref = np.ascontiguousarray(np.broadcast_to(row[:W], (H, W)))
    cur = np.ascontiguousarray(np.broadcast_to(row[1:W + 1], (H, W)))
    winners = oracle.search(cur, ref, B, R, 0)
    by_xy = {(w[0], w[1]): w[4:] for w in winners}
    assert by_xy[(8, 8)] == (-3, -6, 0) and by_xy[(0, 0)] == (1, 0, 0)          # (0, 0): no dx < 0 and no dy < 0 inside the frame
    assert _same(_numpy(cur, ref, B=B, R=R, lam=0, intra=255), oracle.outputs(winners, 255))
    with_lam = oracle.search(cur, ref, B, R, 1)                        # any lam > 0: the shortest match, (1, 0)
    assert all(w[4:] == (1, 0, 0) for w in with_lam if w[0] + w[2] + 1 <= W)
    assert _same(_numpy(cur, ref, B=B, R=R, lam=1, intra=255), oracle.outputs(with_lam, 255))


@pytest.mark.parametrize("sy,sx", [(3, -5), (-6, 6), (0, 1), (5, 0)])
def test_translation_is_recovered_exactly(sy, sx):
    """cur[y][x] = ref[y + sy][x + sx] on i.i.d. noise: every block whose true displacement is a candidate comes back with it and SAD 0."""
    H, W, B, R = 37, 53, 8, 6
    cur, ref = oracle.shifted_pair(H, W, sx, sy)
    assert np.array_equal(cur[max(0, -sy):H - max(0, sy), max(0, -sx):W - max(0, sx)], ref[max(0, sy):H + min(0, sy), max(0, sx):W + min(0, sx)])
    rec, sad, st = _numpy(cur, ref, B=B, R=R, lam=2, intra=255)
    n = 0
    for r, s in zip(rec.astype(np.int64), sad):
        x0, y0, w, h = r[:4]
        if 0 <= x0 + sx and x0 + w + sx <= W and 0 <= y0 + sy and y0 + h + sy <= H:
            assert (r[4], r[5], r[6], s) == (4 * sx, 4 * sy, 0, 0), (x0, y0)
            n += 1
    assert n == {(3, -5): 24, (-6, 6): 20, (0, 1): 30, (5, 0): 28}[(sy, sx)] and st[0] == 0          # geometry alone: 102 blocks in all
    assert _same((rec, sad, st), oracle.outputs(oracle.search(cur, ref, B, R, 2), 255))


@pytest.mark.parametrize("B", [8, 16])
def test_independent_noise_is_all_intra(B):
    H, W, R = 37, 53, 8
    cur, ref = oracle.canvas(oracle.SEED + 1, H, W), oracle.canvas(oracle.SEED + 2, H, W)
    rec, sad, st = _numpy(cur, ref, B=B, R=R, lam=2, intra=20)
    n = rec.shape[0]
    assert (rec[:, 4:] == (0, 0, oracle.INTRA_REF, 0)).all() and st.tolist() == [n, 0, 0, 0]
    assert (sad.astype(np.int64) > 20 * rec[:, 2].astype(np.int64) * rec[:, 3]).all()
    assert _same((rec, sad, st), oracle.outputs(oracle.search(cur, ref, B, R, 2), 20))
    rec255, _, st255 = _numpy(cur, ref, B=B, R=R, lam=2, intra=255)   # 255 never fires
    assert (rec255[:, 6] == 0).all() and st255[0] == 0 and st255[3] == H * W


def test_intra_bound_is_inclusive():
    """One 8 x 8 block, reference all 100: a block whose SAD is exactly intra w h is a match, one above it is intra."""
    ref = np.full((8, 8), 100, np.uint8)
    cur = np.full((8, 8), 107, np.uint8)                               # SAD = 7 * 64 at every candidate
    rec, sad, st = _numpy(cur, ref, B=8, R=2, lam=1, intra=7)
    assert rec.tolist() == [[0, 0, 8, 8, 0, 0, 0, 0]] and sad.tolist() == [448] and st.tolist() == [0, 1, 448, 64]
    cur[3, 4] = 108                                                    # SAD = 449
    rec, sad, st = _numpy(cur, ref, B=8, R=2, lam=1, intra=7)
    assert rec.tolist() == [[0, 0, 8, 8, 0, 0, oracle.INTRA_REF, 0]] and sad.tolist() == [449] and st.tolist() == [1, 0, 0, 0]
    assert _same((rec, sad, st), oracle.outputs(oracle.search(cur, ref, 8, 2, 1), 7))
    rec, _, _ = _numpy(cur, ref, B=8, R=2, lam=1, intra=8, ref_index=5)
    assert rec.tolist() == [[0, 0, 8, 8, 0, 0, 5, 0]]


@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_every_format_searches_its_luma8_plane(fmt):
    from arseg_amd import ingest

    H, W, B, R = 38, 54, 8, 4
    cur, ref = oracle.format_planes(fmt, H, W)
    a, b = oracle.luma8(cur, fmt), oracle.luma8(ref, fmt)
    assert a.dtype == np.uint8 and a.shape == (H, W) and np.array_equal(ingest.luma8_numpy(cur, fmt), a)
    if fmt == oracle.I010:
        assert (cur >> 10).any() and np.array_equal(a, oracle.luma8(cur & 0x3ff, fmt))          # junk in the high 6 bits, ignored
    want = oracle.outputs(oracle.search(a, b, B, R, 2), 40)
    assert (want[0][:, 4:6] == (12, 8)).sum() >= 10 and want[1].max() > 0           # the shift is found, through the noise
    assert _same(_numpy(cur, ref, B=B, R=R, lam=2, intra=40, src_format=fmt), want)
    # a pitched view: the planes as columns of a wider buffer
    wide_c, wide_r = (np.full((H, W + 9) + p.shape[2:], 171, p.dtype) for p in (cur, ref))
    wide_c[:, 4:4 + W], wide_r[:, 2:2 + W] = cur, ref
    assert _same(_numpy(wide_c[:, 4:4 + W], wide_r[:, 2:2 + W], B=B, R=R, lam=2, intra=40, src_format=fmt), want)
    import torch

    tc, tr = (torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p) for p in (cur, ref))
    assert _same(_numpy(tc[None], tr[None], B=B, R=R, lam=2, intra=40, src_format=fmt), want)          # tensors, a batch axis of one


def test_luma_plane_of_decoded_frames():
    import torch
    from arseg_amd import _lib, ingest

    g = np.random.default_rng(3)
    y, uv = g.integers(0, 256, (2, 8, 12), dtype=np.uint8), g.integers(0, 256, (2, 4, 6, 2), dtype=np.uint8)
    wide = torch.from_numpy(np.pad(y, ((0, 0), (0, 0), (0, 4))))
    f = ingest.DecodedFrames.nv12(wide[:, :, :12], uv)
    plane, fmt = f.luma_plane()
    assert fmt == _lib.SRC_NV12 and plane.data_ptr() == wide.data_ptr() and plane.stride(1) == 16 and tuple(plane.shape) == (2, 8, 12)
    rgb = ingest.DecodedFrames.rgb8(g.integers(0, 256, (8, 12, 3), dtype=np.uint8))
    plane, fmt = rgb.luma_plane()
    assert fmt == _lib.SRC_RGB8 and tuple(plane.shape) == (1, 8, 12, 3) and plane is rgb.planes[0]
    y16 = (g.integers(0, 1024, (8, 12)).astype(np.uint16) << 6)
    p10 = ingest.DecodedFrames.p010(y16, np.zeros((4, 6, 2), np.uint16))
    assert p10.luma_plane()[1] == _lib.SRC_P010 and p10.luma_plane()[0].dtype == torch.uint16


def test_records_chain_with_intra_links_and_no_clamp():
    """The estimated records go through records_to_dense and chain_records_numpy: intra blocks carry LINK_INTRA, nothing is clamped or uncovered."""
    from arseg_amd import ingest

    frames = oracle.gop_frames()
    H, W = frames[0].shape
    pushes, n_intra = [], 0
    for f in range(1, len(frames)):
        rec, _, st = _numpy(frames[f], frames[f - 1], B=16, R=8, lam=2, intra=20)
        pushes.append((f, rec))
        dense = ingest.records_to_dense(rec, H, W)
        assert (dense[..., 2] >= 0).all()                              # the records tile the frame
        intra_px = dense[..., 2] == oracle.INTRA_REF
        assert not dense[intra_px][:, :2].any() and intra_px.sum() + st[3] == H * W
        n_intra += int(st[0])
        if f == 3:
            assert intra_px[16:40, 32:64].all()                        # the rectangle of fresh noise (its blocks lie inside it)
    assert n_intra > 0
    for max_ref in (1, 3, 16):
        merged, link = ingest.chain_records_numpy(pushes, H, W, len(frames), max_ref, return_link=True)
        assert not (link[1:] & (ingest.LINK_CLAMPED | ingest.LINK_UNCOVERED)).any()
        d3 = ingest.records_to_dense(pushes[2][1], H, W)
        assert np.array_equal((link[3] & ingest.LINK_INTRA) != 0, (d3[..., 2] == oracle.INTRA_REF) | ((link[2] & ingest.LINK_INTRA) != 0)[
            np.clip(np.arange(H)[:, None] + d3[..., 1] // 4, 0, H - 1), np.clip(np.arange(W)[None, :] + d3[..., 0] // 4, 0, W - 1)])
    interior = merged[1][16:48, 16:80]                                 # the pan of (2, 1) per frame, away from the border
    assert (interior == (8, 4)).all()


def test_bad_arguments_are_refused():
    from arseg_amd import ingest

    a = np.zeros((16, 16), np.uint8)
    for kw in ({"B": 4}, {"B": 32}, {"R": 0}, {"R": 33}, {"lam": -1}, {"lam": 256}, {"intra": 256}, {"intra": -1}, {"ref_index": 16}, {"ref_index": -1},
               {"src_format": 9}):
        with pytest.raises(ValueError):
            ingest.block_motion_numpy(a, a, **kw)
    with pytest.raises(ValueError):
        ingest.block_motion_numpy(a, a[:8])
    with pytest.raises(ValueError):
        ingest.block_motion_numpy(a.astype(np.uint16), a.astype(np.uint16))
    with pytest.raises(ValueError):
        ingest.block_motion_numpy(a, a, src_format=oracle.P010)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Validation happens before any launch, so it is checkable without a GPU (the same cases run in tests/test_gpu_block_motion.py)."""
    from arseg_amd import _lib

    lib = _lib.load()
    assert lib.arseg_block_motion_workspace_bytes(720, 960, 16, 16) == 0
    for name, args, want in oracle.abi_cases():
        assert lib.arseg_block_motion_fwd(*args) == want, name
