"""CPU checks of the hierarchical block search's host forms (ingest.luma_pyramid_numpy, ingest.block_motion_pyr_numpy) against the loop oracle
of tests/block_motion_pyr_oracle.py, which is written from the definition in include/arseg_hip.h (arseg_luma_pyramid_fwd,
arseg_block_motion_pyr_fwd).  Integers in, integers out: every comparison is np.array_equal."""
import numpy as np
import pytest

import block_motion_oracle as bmo
import block_motion_pyr_oracle as oracle


def _numpy(cur, ref, **kw):
    from arseg_amd import ingest

    rec, sad, st = ingest.block_motion_pyr_numpy(cur, ref, **kw)
    assert rec.dtype == np.int16 and sad.dtype == np.uint32 and st.dtype == np.int64 and st.shape == (oracle.NSTATS,)
    return rec, sad, st


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("H,W", oracle.SIZES + ((100, 150),))
def test_pyramid_numpy_equals_the_loops(H, W):
    from arseg_amd import ingest

    p0 = bmo.canvas(oracle.SEED + H, H, W)
    want = oracle.pyramid(p0, 3)
    got = ingest.luma_pyramid_numpy(p0, bmo.NV12, 3)
    assert [g.shape for g in got] == [w.shape for w in want] and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got, want))
    if (H, W) == (5, 7):
        assert [g.shape for g in got] == [(5, 7), (3, 4), (2, 2), (1, 1)]
        a = p0.astype(np.int64)
        assert got[1][2, 3] == (4 * a[4, 6] + 2) >> 2 and got[1][0, 3] == (2 * a[0, 6] + 2 * a[1, 6] + 2) >> 2          # the replicated corner and column
    if (H, W) == (37, 53):
        assert [g.shape[0] for g in got] == [37, 19, 10, 5]
    lay, total = ingest.luma_pyramid_layout(H, W, 3)
    assert (lay, total) == oracle.layout(H, W, 3) and lay[0][0] == 0 and all(p % 16 == 0 and p >= w for _, p, _, w in lay)
    for L in (1, 2):
        assert _same(ingest.luma_pyramid_numpy(p0, bmo.NV12, L), want[:L + 1])


@pytest.mark.parametrize("case", oracle.search_cases(), ids=oracle.case_id)
def test_numpy_form_equals_the_loop_oracle(case):
    kind, H, W, B, L, r, lam = case
    cur, ref = oracle.content(kind, H, W)
    winners = oracle.winners_of(*case)
    for intra in oracle.INTRAS:
        want = oracle.outputs(winners, intra)
        assert want[0].shape == (-(-H // B) * -(-W // B), 8)
        assert _same(_numpy(cur, ref, B=B, Rt=oracle.RT, r=r, lam=lam, intra=intra, levels=L), want), intra
    if kind == "constant":                                            # every candidate ties at SAD 0: the zero vector
        assert all(w[4:] == (0, 0, 0) for w in winners)
    if kind == "stripes":
        assert all(w[6] == 0 for w in winners)


def test_parents_centres_and_the_candidate_union():
    """Block (2, 3) of a 3 x 4 parent grid: parent (1, 1), horizontal neighbour column 2 (bj odd), vertical neighbour row 0 (bi even); the
    corner blocks lack the neighbour that would lie outside the grid; two centres that propose the same vectors count once."""
    pv = {(i, j): (10 * i + j, -(10 * i + j)) for i in range(3) for j in range(4)}
    assert oracle.centres(2, 3, pv, 3, 4) == [(0, 0), (22, -22), (24, -24), (2, -2)]
    assert oracle.centres(0, 0, pv, 3, 4) == [(0, 0), (0, 0)]                                  # column -1 and row -1 are not in the grid
    assert oracle.centres(5, 7, pv, 3, 4) == [(0, 0), (46, -46)]                               # column 4 and row 3 neither
    assert oracle.centres(5, 6, pv, 3, 4) == [(0, 0), (46, -46), (44, -44)]
    big = dict(x0=100, y0=100, w=16, h=16, H=400, W=400)
    assert len(oracle.candidates([(0, 0), (0, 0)], 1, **big)) == 9
    assert len(oracle.candidates([(0, 0), (2, 0)], 1, **big)) == 15                             # the column dx = 1 is proposed twice
    assert len(oracle.candidates([(0, 0), (20, 0), (0, 20), (20, 20)], 3, **big)) == 4 * 49
    assert oracle.candidates([(0, 0), (-4, -4)], 1, x0=0, y0=0, w=16, h=16, H=32, W=32) == [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert oracle.interior(128, 192, 16, 2, -40, 9) == [bi * 12 + bj for bi in range(4) for bj in range(4, 12)]


def test_two_centres_propose_the_same_candidate():
    """A shift of (2, 2), (1, 1) at level 1: where the parents agree the centres are (0, 0) and (2, 2), whose +-1 neighbourhoods share (1, 1) --
    and the numpy form, which scores a vector once per centre, still equals the loops, which score it once."""
    H, W, B = 64, 96, 16
    cur, ref = oracle.translation_pair(H, W, 2, 2)
    counts = []
    winners = oracle.search(cur, ref, B, 1, 4, 1, 2, counts)
    # block (0, 0): no neighbour parents; 4 of the 9 around (0, 0) are inside the frame, 9 around (2, 2), (1, 1) in both.  Block (0, 1): the
    # neighbour parent (0, 1) agrees with the parent; 6 + 9 - 1
    assert counts[0] == 4 + 9 - 1 and counts[1] == 6 + 9 - 1 and winners[1][4:] == (2, 2, 0)
    assert _same(_numpy(cur, ref, B=B, Rt=4, r=1, lam=2, intra=255, levels=1), oracle.outputs(winners, 255))


def test_two_non_zero_candidates_tie():
    """Vertical stripes of period 4, cur one pixel left of ref: at level 1 cur is flat (every 2 x 2 mean is 120), every top-level candidate
    ties and (0, 0) wins, and level 0 refines around it with r = 3: dx = 1 and dx = -3 match with SAD 0 at every dy.  At lam = 0 the smallest
    dy, then the smallest dx wins -- (-3, -3) where the frame allows it; at lam = 1 the shortest, (1, 0)."""
    H, W, B = 32, 48, 8
    row = np.where(np.arange(W + 8) % 4 < 2, 40, 200).astype(np.uint8)
    ref = np.ascontiguousarray(np.broadcast_to(row[:W], (H, W)))
    cur = np.ascontiguousarray(np.broadcast_to(row[1:W + 1], (H, W)))
    assert (oracle.pyramid(cur, 1)[1] == 120).all()
    winners = oracle.search(cur, ref, B, 1, 2, 3, 0)
    by_xy = {(w[0], w[1]): w[4:] for w in winners}
    assert by_xy[(8, 8)] == (-3, -3, 0) and by_xy[(0, 0)] == (1, 0, 0) and by_xy[(8, 0)] == (-3, 0, 0)
    assert _same(_numpy(cur, ref, B=B, Rt=2, r=3, lam=0, intra=255, levels=1), oracle.outputs(winners, 255))
    with_lam = oracle.search(cur, ref, B, 1, 2, 3, 1)
    assert all(w[4:] == (1, 0, 0) for w in with_lam if w[0] + w[2] + 1 <= W)
    assert _same(_numpy(cur, ref, B=B, Rt=2, r=3, lam=1, intra=255, levels=1), oracle.outputs(with_lam, 255))


@pytest.mark.parametrize("fmt", bmo.FORMATS)
def test_every_format_and_pitched_views(fmt):
    """The pyramid and the search see the luma8 plane and nothing else of a format: junk in the ignored bits, views at a pitch, tensors."""
    import torch
    from arseg_amd import ingest

    H, W, B = 38, 54, 8
    cur, ref = bmo.format_planes(fmt, H, W)
    a, b = bmo.luma8(cur, fmt), bmo.luma8(ref, fmt)
    assert _same(ingest.luma_pyramid_numpy(cur, fmt, 2), oracle.pyramid(a, 2))
    want = oracle.outputs(oracle.search(a, b, B, 2, 2, 1, 2), 40)
    assert (want[0][:, 4:6] == (12, 8)).sum() >= 10 and want[1].max() > 0
    assert _same(_numpy(cur, ref, B=B, Rt=2, r=1, lam=2, intra=40, levels=2, src_format=fmt), want)
    wide_c, wide_r = (np.full((H, W + 9) + p.shape[2:], 171, p.dtype) for p in (cur, ref))
    wide_c[:, 4:4 + W], wide_r[:, 2:2 + W] = cur, ref
    assert _same(_numpy(wide_c[:, 4:4 + W], wide_r[:, 2:2 + W], B=B, Rt=2, r=1, lam=2, intra=40, levels=2, src_format=fmt), want)
    tc, tr = (torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p) for p in (cur, ref))
    assert _same(_numpy(tc[None], tr[None], B=B, Rt=2, r=1, lam=2, intra=40, levels=2, src_format=fmt), want)


def test_levels_0_is_the_full_search():
    from arseg_amd import ingest

    cur, ref = oracle.tiles_pair()
    for B, R in ((8, 5), (16, 7)):
        assert _same(_numpy(cur, ref, B=B, Rt=R, r=1, lam=2, intra=20, ref_index=3, levels=0), ingest.block_motion_numpy(cur, ref, B=B, R=R, lam=2, intra=20, ref_index=3))


@pytest.mark.parametrize("B", [8, 16])
def test_several_tiles_against_the_loops(B):
    cur, ref = oracle.tiles_pair()
    for L, Rt, r, lam in ((2, 4, 1, 2), (1, 7, 2, 0)):
        winners = oracle.tiles_winners(B, L, Rt, r, lam)
        want = oracle.outputs(winners, 20)
        assert 0 < want[2][0] < len(winners)                           # some blocks intra, not all
        assert sum(w[4:6] == (-11, 6) for w in winners) >= (10 if B == 16 else 40)
        assert _same(_numpy(cur, ref, B=B, Rt=Rt, r=r, lam=lam, intra=20, ref_index=2, levels=L), oracle.outputs(winners, 20, 2)), (L, Rt, r, lam)


def test_records_chain_with_intra_links_and_no_clamp():
    """The records go through records_to_dense and chain_records_numpy as the full search's do: intra blocks carry LINK_INTRA, nothing is
    clamped or uncovered, and the pan of (-12, 4) per frame -- beyond a full search of 8 -- is what the chain adds up."""
    from arseg_amd import ingest

    frames = oracle.gop_frames()
    H, W = frames[0].shape
    pushes, n_intra = [], 0
    for f in range(1, len(frames)):
        rec, _, st = _numpy(frames[f], frames[f - 1], B=16, Rt=4, r=1, lam=2, intra=20, levels=2)
        assert _same((rec,), oracle.outputs(oracle.search(frames[f], frames[f - 1], 16, 2, 4, 1, 2), 20))
        pushes.append((f, rec))
        dense = ingest.records_to_dense(rec, H, W)
        assert (dense[..., 2] >= 0).all()
        intra_px = dense[..., 2] == oracle.INTRA_REF
        assert not dense[intra_px][:, :2].any() and intra_px.sum() + st[3] == H * W
        n_intra += int(st[0])
        if f == 3:
            assert intra_px[32:80, 64:128].all()                       # the rectangle of fresh noise (its blocks lie inside it)
    assert n_intra > 0
    merged, link = ingest.chain_records_numpy(pushes, H, W, len(frames), 1, return_link=True)
    assert not (link[1:] & (ingest.LINK_CLAMPED | ingest.LINK_UNCOVERED)).any() and (link[3:] & ingest.LINK_INTRA).any()
    assert (merged[1][32:64, 96:160] == (-48, 16)).all() and (merged[2][32:64, 96:160] == (-96, 32)).all()


TRANSLATIONS = [(128, 192, 16, 2, 16, 1, 5, -3), (128, 192, 16, 2, 16, 1, 23, 17), (128, 192, 16, 2, 16, 1, -40, 9), (256, 384, 16, 3, 8, 2, 61, -38)]


@pytest.mark.parametrize("H,W,B,L,Rt,r,sx,sy", TRANSLATIONS)
def test_translation_is_recovered_on_interior_blocks(H, W, B, L, Rt, r, sx, sy):
    """cur[y][x] = ref[y + sy][x + sx] on uniform byte noise, lam = 2: every whole block whose level-L ancestor, displaced by the shift, lies
    inside the frame comes back with exactly the shift and SAD 0.  A property of these inputs, checked here on the host form; the GPU file
    holds the kernel to the same inputs."""
    cur, ref = oracle.translation_pair(H, W, sx, sy)
    rec, sad, st = _numpy(cur, ref, B=B, Rt=Rt, r=r, lam=2, intra=255, levels=L)
    idx = oracle.interior(H, W, B, L, sx, sy)
    assert len(idx) == (128 if H == 256 else 32) and oracle.recovered(rec, sad, idx, sx, sy) == len(idx)
    if max(abs(sx), abs(sy)) > 32:                                     # out of the full search's reach: none of its vectors can be the shift
        from arseg_amd import ingest

        full, fsad, _ = ingest.block_motion_numpy(cur, ref, B=B, R=32, lam=2, intra=255)
        assert oracle.recovered(full, fsad, idx, sx, sy) == 0 and (np.abs(full[:, 4:6].astype(np.int64)) <= 128).all()


def test_reach_and_bad_arguments():
    from arseg_amd import _lib, ingest

    a = np.zeros((16, 16), np.uint8)
    for kw in ({"levels": 4}, {"levels": -1}, {"r": 0}, {"r": 4}, {"B": 4}, {"Rt": 0}, {"Rt": 33}, {"lam": 256}, {"intra": -1}, {"ref_index": 16}, {"src_format": 9}):
        with pytest.raises(ValueError):
            ingest.block_motion_pyr_numpy(a, a, **kw)
    with pytest.raises(ValueError):
        ingest.block_motion_pyr_numpy(a, a[:8])
    with pytest.raises(ValueError):
        ingest.luma_pyramid_numpy(a, bmo.NV12, 4)
    with pytest.raises(ValueError):
        ingest.luma_pyramid_layout(0, 16, 1)
    # reach = search 2^L + refine (2^L - 1); the estimator itself needs a GPU, its arithmetic does not
    reach = ingest.MotionEstimator.reach.fget
    for L, Rt, r, want in ((0, 32, 1, 32), (2, 8, 1, 35), (2, 16, 1, 67), (3, 32, 3, 277), (1, 1, 1, 3)):
        est = ingest.MotionEstimator.__new__(ingest.MotionEstimator)
        est.levels, est.search, est.refine = L, Rt, r
        assert reach(est) == want
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(32, 48, levels=2, device="cpu")
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(32, 48, levels=4, device="cpu")
    with pytest.raises(_lib.ArsegError):
        ingest.LumaPyramid(32, 48, 2, device="cpu")


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Validation happens before any launch, so it is checkable without a GPU (the same cases run in tests/test_gpu_block_motion_pyr.py)."""
    from arseg_amd import _lib

    lib = _lib.load()
    assert lib.arseg_luma_pyramid_bytes(32, 48, 2) == 48 * 32 + 32 * 16 + 16 * 8 and lib.arseg_luma_pyramid_bytes(5, 7, 3) == 16 * (5 + 3 + 2 + 1)
    assert lib.arseg_luma_pyramid_bytes(1024, 2048, 2) == 2048 * 1024 + 1024 * 512 + 512 * 256
    assert lib.arseg_luma_pyramid_bytes(0, 7, 1) == 0 and lib.arseg_luma_pyramid_bytes(8, 8, 0) == 0 and lib.arseg_luma_pyramid_bytes(8, 8, 4) == 0
    assert lib.arseg_block_motion_pyr_workspace_bytes(32, 48, 16, 2) == 48 and lib.arseg_block_motion_pyr_workspace_bytes(37, 53, 8, 3) == 16 * (3 * 4 + 2 * 2 + 1)
    assert lib.arseg_block_motion_pyr_workspace_bytes(32, 48, 12, 2) == 0 and lib.arseg_block_motion_pyr_workspace_bytes(32, 48, 16, 0) == 0
    for name, fn, args, want in oracle.abi_cases():
        assert getattr(lib, fn)(*args) == want, (fn, name)
