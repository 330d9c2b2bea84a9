"""GPU checks of the hierarchical block search (csrc/block_motion_pyr.hip: arseg_luma_pyramid_fwd, arseg_block_motion_pyr_fwd; ops.luma_pyramid,
ops.block_motion_pyr, ingest.LumaPyramid, ingest.MotionEstimator(levels=...)) against the loop oracle of tests/block_motion_pyr_oracle.py and,
where the loops would take too long, against ingest.block_motion_pyr_numpy, which tests/test_block_motion_pyr.py holds to that oracle.
Integers in, integers out: every comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import block_motion_oracle as bmo
import block_motion_pyr_oracle as oracle
import mv_link_oracle

pytestmark = pytest.mark.gpu

GUARD16, GUARD = 0x5a5a, 0x5a


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _plane(p, dev):
    p = np.ascontiguousarray(p)
    return torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(dev)


def _pyramid(dev, plane, fmt, L):
    """ops.luma_pyramid of a device plane (taken as it is: a view keeps its pitch) into a buffer with guard bytes behind it; the guard and the
    plane stay as they were.  Returns the device buffer (exactly the pyramid's bytes) and the levels' pixels as numpy."""
    from arseg_amd import _lib, ops

    t = plane if torch.is_tensor(plane) else _plane(plane, dev)
    keep = t.clone()
    lead = t.dim() - (3 if fmt == bmo.RGB8 else 2)
    H, W = t.shape[lead], t.shape[lead + 1]
    n = _lib.load().arseg_luma_pyramid_bytes(H, W, L)
    assert n == oracle.layout(H, W, L)[1]
    buf = torch.full((n + 64,), GUARD, dtype=torch.uint8, device=dev)
    out = ops.luma_pyramid(t, fmt, L, out=buf[:n])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and bool((buf[n:] == GUARD).all()) and torch.equal(t, keep)
    return buf[:n], oracle.levels_of(buf[:n].cpu().numpy(), H, W, L)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("H,W", oracle.SIZES + ((100, 150),))
def test_pyramid_kernel_equals_the_loops(dev, H, W):
    """5 x 7 is one tile with H_3 = 1; 37 x 53 is odd at every level; 100 x 150 is 4 x 3 tiles, the last row and column of tiles cut by the
    frame at every level."""
    p0 = bmo.canvas(oracle.SEED + H, H, W)
    want = oracle.pyramid(p0, 3)
    for L in (1, 2, 3):
        assert _same(_pyramid(dev, p0, bmo.NV12, L)[1], want[:L + 1]), L


@pytest.mark.parametrize("fmt", bmo.FORMATS)
def test_pyramid_of_every_format_pitched_and_unaligned(dev, fmt):
    """Each format's plane, then the same plane as columns of a wider buffer at an odd sample offset (rows at a pitch, no 4-byte alignment for
    the 8-bit formats), the bytes around it untouched; a batch axis of one."""
    H, W = 38, 54
    cur, _ = bmo.format_planes(fmt, H, W)
    want = oracle.pyramid(bmo.luma8(cur, fmt), 2)
    assert _same(_pyramid(dev, cur, fmt, 2)[1], want)
    wide = np.full((H, W + 9) + cur.shape[2:], 171, cur.dtype)
    wide[:, 3:3 + W] = cur
    d = _plane(wide, dev)
    v = d[:, 3:3 + W]
    assert not v.is_contiguous() and v.data_ptr() % 4 != 0
    assert _same(_pyramid(dev, v, fmt, 2)[1], want) and _same(_pyramid(dev, v[None], fmt, 2)[1], want)
    assert np.array_equal(d.cpu().numpy().view(wide.dtype), wide)


def _run(dev, cur, ref, L, fmt=bmo.NV12, calls=1, stats_from=None, **kw):
    """The two pyramids, then ops.block_motion_pyr into buffers with guard words behind records, sad, stats and the workspace.  After the
    calls: every guard and both pyramids as they were.  Returns numpy (records, sad, stats)."""
    from arseg_amd import _lib, ops

    pc, pr = _pyramid(dev, cur, fmt, L)[0], _pyramid(dev, ref, fmt, L)[0]
    keep_c, keep_r = pc.clone(), pr.clone()
    t = cur if torch.is_tensor(cur) else np.asarray(cur)
    H, W, B = t.shape[0], t.shape[1], kw.get("B", 16)
    n = -(-H // B) * -(-W // B)
    nws = _lib.load().arseg_block_motion_pyr_workspace_bytes(H, W, B, L)
    rbuf = torch.full(((n + 2) * 8,), GUARD16, dtype=torch.int16, device=dev)
    sbuf = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    tbuf = torch.full((oracle.NSTATS + 2,), GUARD, dtype=torch.int64, device=dev)
    wbuf = torch.full((nws + 64,), GUARD, dtype=torch.uint8, device=dev)
    rec, sad, st = rbuf[:n * 8].view(n, 8), sbuf[:n], tbuf[:oracle.NSTATS]
    st.zero_()
    if stats_from is not None:
        st.copy_(torch.as_tensor(stats_from, dtype=torch.int64))
    for _ in range(calls):
        out = ops.block_motion_pyr(pc, pr, H, W, L, records=rec, sad=sad, stats=st, workspace=wbuf[:nws], **kw)
        assert out[0].data_ptr() == rec.data_ptr() and out[1].data_ptr() == sad.data_ptr() and out[2].data_ptr() == st.data_ptr()
    torch.cuda.synchronize()
    assert bool((rbuf[n * 8:] == GUARD16).all()) and bool((sbuf[n:] == GUARD).all()) and bool((tbuf[oracle.NSTATS:] == GUARD).all())
    assert bool((wbuf[nws:] == GUARD).all()) and torch.equal(pc, keep_c) and torch.equal(pr, keep_r)
    return rec.cpu().numpy(), sad.cpu().numpy().view(np.uint32), st.cpu().numpy()


CASES = list(dict.fromkeys(c[:5] for c in oracle.search_cases()))     # (kind, H, W, B, L); r and lam are looped over inside a test


@pytest.mark.parametrize("case", CASES, ids=oracle.case_id)
def test_search_equals_the_loop_oracle(dev, case):
    """The grid of tests/test_block_motion_pyr.py: 5 x 7 is one clipped block whose level 3 is one pixel; 37 x 53 has clipped blocks on both
    edges at every level and edge blocks without a neighbour parent."""
    kind, H, W, B, L = case
    cur, ref = oracle.content(kind, H, W)
    for r in oracle.REFINES:
        for lam in oracle.LAMS:
            winners = oracle.winners_of(kind, H, W, B, L, r, lam)
            for intra in oracle.INTRAS:
                assert _same(_run(dev, cur, ref, L, B=B, Rt=oracle.RT, r=r, lam=lam, intra=intra), oracle.outputs(winners, intra)), (r, lam, intra)


@pytest.mark.parametrize("B", [8, 16])
def test_several_tiles_against_the_loops_stats_accumulate_outputs_optional(dev, B):
    from arseg_amd import ops

    cur, ref = oracle.tiles_pair()
    for L, Rt, r, lam in ((2, 4, 1, 2), (1, 7, 2, 0)):
        want = oracle.outputs(oracle.tiles_winners(B, L, Rt, r, lam), 20, 2)
        assert 0 < want[2][0] < len(want[1])
        assert _same(_run(dev, cur, ref, L, B=B, Rt=Rt, r=r, lam=lam, intra=20, ref_index=2), want), (L, Rt, r, lam)
    rec, sad, st = _run(dev, cur, ref, 1, calls=2, stats_from=[5, 6, 7, 8], B=B, Rt=7, r=2, lam=0, intra=20, ref_index=2)
    assert np.array_equal(rec, want[0]) and np.array_equal(sad, want[1]) and np.array_equal(st, 2 * want[2] + np.array([5, 6, 7, 8]))
    H, W = cur.shape
    pc, pr = ops.luma_pyramid(_plane(cur, dev), bmo.NV12, 1), ops.luma_pyramid(_plane(ref, dev), bmo.NV12, 1)          # allocated
    r2, s2, t2 = ops.block_motion_pyr(pc, pr, H, W, 1, B, 7, 2, 0, 20, 2, sad=False, stats=False)                     # NULL sad and stats; the host layer's workspace
    assert s2 is None and t2 is None and np.array_equal(r2.cpu().numpy(), want[0])
    r3, s3, t3 = ops.block_motion_pyr(pc, pr, H, W, 1, B, 7, 2, 0, 20, 2)                                             # everything allocated, stats from zero
    assert np.array_equal(r3.cpu().numpy(), want[0]) and np.array_equal(s3.cpu().numpy().view(np.uint32), want[1]) and np.array_equal(t3.cpu().numpy(), want[2])


@pytest.mark.parametrize("B,L,Rt,r", [(16, 3, 32, 3), (8, 2, 13, 2), (16, 1, 5, 1)])
def test_several_tiles_against_the_numpy_form(dev, B, L, Rt, r):
    from arseg_amd import ingest

    cur, ref = oracle.tiles_pair()
    assert _same(_run(dev, cur, ref, L, B=B, Rt=Rt, r=r, lam=1, intra=30), ingest.block_motion_pyr_numpy(cur, ref, B=B, Rt=Rt, r=r, lam=1, intra=30, levels=L))


def test_360x480_against_the_numpy_form(dev):
    """CamVid's frame size: 23 x 30 blocks, the bottom row of blocks 8 pixels tall; a shift of (-26, 12), out of the full search's default reach."""
    from arseg_amd import ingest

    H, W = 360, 480
    cur, ref = (p.copy() for p in oracle.translation_pair(H, W, -26, 12, seed=oracle.SEED + 31))
    g = np.random.Generator(np.random.PCG64(oracle.SEED + 32))
    cur = np.clip(cur.astype(np.int64) + g.integers(-3, 4, cur.shape), 0, 255).astype(np.uint8)
    cur[100:180, 200:330] = g.integers(0, 256, (80, 130), dtype=np.uint8)
    want = ingest.block_motion_pyr_numpy(cur, ref, B=16, Rt=8, r=1, lam=2, intra=24, levels=2)
    assert want[0].shape == (23 * 30, 8) and 28 <= want[2][0] < 23 * 30 and (want[0][:, 4:6] == (-104, 48)).sum() > 400
    assert _same(_run(dev, cur, ref, 2, B=16, Rt=8, r=1, lam=2, intra=24), want)


@pytest.mark.parametrize("fmt", bmo.FORMATS)
def test_every_format_searches_its_luma8_plane(dev, fmt):
    H, W, B = 38, 54, 8
    cur, ref = bmo.format_planes(fmt, H, W)
    want = oracle.outputs(oracle.search(bmo.luma8(cur, fmt), bmo.luma8(ref, fmt), B, 2, 2, 1, 2), 40)
    assert _same(_run(dev, cur, ref, 2, fmt, B=B, Rt=2, r=1, lam=2, intra=40), want)


def test_translation_beyond_the_full_search(dev):
    """The capability: 128 x 192, B = 16, cur[y][x] = ref[y + 9][x - 40].  The hierarchical estimator with L = 2, Rt = 16, r = 1 returns exactly
    (-160, 36) quarter-pels with SAD 0 on every interior block (tests/test_block_motion_pyr.py: the host form does, on this input); the full
    search at R = 32 cannot return it for any of them."""
    from arseg_amd import ingest

    H, W, sx, sy = 128, 192, -40, 9
    cur, ref = oracle.translation_pair(H, W, sx, sy)
    idx = oracle.interior(H, W, 16, 2, sx, sy)
    assert len(idx) == 32
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    fc, fr = (ingest.DecodedFrames.nv12(_plane(p, dev), uv) for p in (cur, ref))
    est = ingest.MotionEstimator(H, W, block=16, search=16, lam=2, device=dev, with_sad=True, levels=2, refine=1)
    assert est.reach == 67
    rec = est.estimate(fc, fr).cpu().numpy()
    sad = est.sad.cpu().numpy().view(np.uint32)
    assert oracle.recovered(rec, sad, idx, sx, sy) == 32
    assert (rec[idx, 4:7] == (-160, 36, 0)).all() and not sad[idx].any()
    full = ingest.MotionEstimator(H, W, block=16, search=32, lam=2, device=dev, with_sad=True)
    assert full.reach == 32
    frec = full.estimate(fc, fr).cpu().numpy()
    assert oracle.recovered(frec, full.sad.cpu().numpy().view(np.uint32), idx, sx, sy) == 0 and (np.abs(frec[:, 4:6].astype(np.int64)) <= 128).all()
    for (sx2, sy2) in ((5, -3), (23, 17)):                             # the other shifts of the CPU file, built pyramids passed in
        c2, r2 = oracle.translation_pair(H, W, sx2, sy2)
        pa, pb = ingest.LumaPyramid(H, W, 2, dev), ingest.LumaPyramid(H, W, 2, dev)
        rec = est.estimate(pa.build(ingest.DecodedFrames.nv12(_plane(c2, dev), uv)), pb.build(ingest.DecodedFrames.nv12(_plane(r2, dev), uv))).cpu().numpy()
        i2 = oracle.interior(H, W, 16, 2, sx2, sy2)
        assert len(i2) == 32 and oracle.recovered(rec, est.sad.cpu().numpy().view(np.uint32), i2, sx2, sy2) == 32
        assert np.array_equal(pa.level(2).cpu().numpy(), oracle.pyramid(c2, 2)[2]) and tuple(pa.level(1).shape) == (64, 96)


def _frames(planes, dev):
    from arseg_amd import ingest

    H, W = planes[0].shape
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(_plane(p, dev), uv) for p in planes]


def test_estimator_feeds_the_chain_over_a_gop(dev):
    """Five frames of a canvas panned by (-12, 4), a rectangle of fresh noise in frame 3: MotionEstimator(levels=2) + MotionChain(track_links=True)
    leave the merged field, link bytes and link counts that chain_records_numpy gives on the host records.  Every frame is built once: two
    LumaPyramids alternate."""
    from arseg_amd import ingest

    planes = oracle.gop_frames()
    H, W, gop = planes[0].shape[0], planes[0].shape[1], len(planes)
    frames = _frames(planes, dev)
    est = ingest.MotionEstimator(H, W, block=16, search=4, lam=2, intra=20, device=dev, with_sad=True, levels=2, refine=1)
    chain = ingest.MotionChain(H, W, gop=gop, max_ref=1, device=dev, track_links=True)
    pyr = [ingest.LumaPyramid(H, W, 2, dev), ingest.LumaPyramid(H, W, 2, dev)]
    pyr[0].build(frames[0])
    pushes, total = [], np.zeros(oracle.NSTATS, np.int64)
    for f in range(1, gop):
        want = ingest.block_motion_pyr_numpy(planes[f], planes[f - 1], B=16, Rt=4, r=1, lam=2, intra=20, levels=2)
        rec = est.estimate(pyr[f & 1].build(frames[f]), pyr[(f - 1) & 1])
        assert rec.data_ptr() == est.records.data_ptr()
        chain.push(rec)
        total += want[2]
        assert np.array_equal(rec.cpu().numpy(), want[0]) and np.array_equal(est.sad.cpu().numpy().view(np.uint32), want[1])
        assert np.array_equal(est.stats_row().cpu().numpy(), total)
        assert torch.equal(est.estimate(frames[f], frames[f - 1]), rec)                      # frames: built into the estimator's own pyramids
        total += want[2]
        pushes.append((f, want[0]))
    assert total[0] > 0
    merged, link = ingest.chain_records_numpy(pushes, H, W, gop, 1, return_link=True)
    assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
    assert np.array_equal(chain.link_stats().cpu().numpy()[1:], mv_link_oracle.stats(link)[1:])
    assert (link[3:] & ingest.LINK_INTRA).any() and not (link & (ingest.LINK_CLAMPED | ingest.LINK_UNCOVERED)).any()
    assert (merged[2][32:64, 96:160] == (-96, 32)).all()


def test_graph_replays_builds_search_and_push_on_new_frames(dev):
    """reset + two pyramid builds + search + push over two static frame buffers in one torch.cuda.graph (a linear chain of launches); the
    buffers are refilled with other frame pairs and the graph replayed."""
    from arseg_amd import ingest

    planes = oracle.gop_frames()
    H, W = planes[0].shape
    prev, cur = _frames([np.zeros_like(planes[0]), np.zeros_like(planes[0])], dev)
    est = ingest.MotionEstimator(H, W, block=16, search=4, lam=2, intra=20, device=dev, levels=2)
    chain = ingest.MotionChain(H, W, gop=2, max_ref=1, device=dev, track_links=True)

    def step():
        est.reset_stats()
        chain.reset()
        return chain.push(est.estimate(cur, prev))

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for f in (1, 3, 4, 1):
        prev.planes[0].copy_(_plane(planes[f - 1], dev)[None])
        cur.planes[0].copy_(_plane(planes[f], dev)[None])
        est.records.fill_(GUARD16)
        graph.replay()
        torch.cuda.synchronize()
        replayed = (est.records.clone(), out.clone(), chain.link().clone(), chain.link_stats().clone(), est.stats_row().clone())
        want = ingest.block_motion_pyr_numpy(planes[f], planes[f - 1], B=16, Rt=4, r=1, lam=2, intra=20, levels=2)
        assert np.array_equal(replayed[0].cpu().numpy(), want[0]) and np.array_equal(replayed[4].cpu().numpy(), want[2])
        eager = step()
        torch.cuda.synchronize()
        assert torch.equal(est.records, replayed[0]) and torch.equal(eager, replayed[1]) and torch.equal(chain.link(), replayed[2])
        assert torch.equal(chain.link_stats(), replayed[3]) and torch.equal(est.stats_row(), replayed[4])


def test_levels_0_is_the_full_search_and_wrappers_refuse(dev):
    from arseg_amd import _lib, ingest, ops

    planes = bmo.gop_frames()
    H, W = planes[0].shape
    fc, fr = _frames(planes[1:3], dev)
    a, b = ingest.MotionEstimator(H, W, search=8, intra=20, device=dev), ingest.MotionEstimator(H, W, search=8, intra=20, device=dev, levels=0, refine=1)
    assert torch.equal(a.estimate(fc, fr), b.estimate(fc, fr)) and torch.equal(a.stats_row(), b.stats_row()) and b.reach == 8
    pyr = torch.zeros(_lib.load().arseg_luma_pyramid_bytes(32, 48, 2), dtype=torch.uint8, device=dev)
    for kw in ({"B": 12}, {"Rt": 0}, {"Rt": 33}, {"r": 0}, {"r": 4}, {"lam": 256}, {"intra": -1}, {"ref_index": 16}):
        with pytest.raises(_lib.ArsegError):
            ops.block_motion_pyr(pyr, pyr, 32, 48, 2, **kw)
    with pytest.raises(_lib.ArsegError):
        ops.block_motion_pyr(pyr, pyr, 32, 48, 3)                      # a pyramid of two levels is too short for three
    with pytest.raises(_lib.ArsegError):
        ops.block_motion_pyr(pyr, pyr[16:], 32, 48, 2)
    with pytest.raises(_lib.ArsegError):
        ops.block_motion_pyr(pyr, pyr, 32, 48, 2, workspace=torch.zeros(47, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.ArsegError):
        ops.luma_pyramid(torch.zeros((32, 48), dtype=torch.uint8, device=dev), bmo.NV12, 4)
    with pytest.raises(_lib.ArsegError):
        ops.luma_pyramid(torch.zeros((32, 48), dtype=torch.uint8, device=dev), bmo.NV12, 2, out=pyr[1:])
    with pytest.raises(_lib.ArsegError):
        ops.luma_pyramid(torch.zeros((32, 48), dtype=torch.uint8), bmo.NV12, 2)
    est = ingest.MotionEstimator(32, 48, device=dev, levels=2)
    with pytest.raises(_lib.ArsegError):
        est.estimate(ingest.LumaPyramid(32, 48, 1, dev), ingest.LumaPyramid(32, 48, 2, dev))
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(32, 48, device=dev, levels=2, refine=4)


def test_c_abi_refuses_bad_arguments(dev):
    from arseg_amd import _lib

    lib = _lib.load()
    for name, fn, args, want in oracle.abi_cases():
        assert getattr(lib, fn)(*args) == want, (fn, name)
