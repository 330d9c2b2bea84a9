"""GPU checks of block motion estimation (csrc/block_motion.hip: arseg_block_motion_fwd; ops.block_motion, ingest.MotionEstimator) against the
loop oracle of tests/block_motion_oracle.py and, where the loops would take too long, against ingest.block_motion_numpy, which
tests/test_block_motion.py holds to that oracle.  Integers in, integers out: every comparison is np.array_equal / torch.equal."""
import functools

import numpy as np
import pytest
import torch

import block_motion_oracle as oracle
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


def _run(dev, cur, ref, fmt=oracle.NV12, calls=1, stats_from=None, **kw):
    """ops.block_motion on device copies of the planes (tensors are taken as they are: views keep their pitch), into buffers with guard
    words behind records, sad and stats.  After the calls: every guard and both planes as they were.  Returns numpy (records, sad, stats)."""
    from arseg_amd import ops

    tc, tr = (p if torch.is_tensor(p) else _plane(p, dev) for p in (cur, ref))
    keep_c, keep_r = tc.clone(), tr.clone()
    lead = tc.dim() - (3 if fmt == oracle.RGB8 else 2)                 # a batch axis of one
    H, W, B = tc.shape[lead], tc.shape[lead + 1], kw.get("B", 16)
    n = -(-H // B) * -(-W // B)
    rbuf = torch.full(((n + 2) * 8,), GUARD16, dtype=torch.int16, device=dev)
    sbuf = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    tbuf = torch.full((oracle.NSTATS + 2,), GUARD, dtype=torch.int64, device=dev)
    rec, sad, st = rbuf[:n * 8].view(n, 8), sbuf[:n], tbuf[:oracle.NSTATS]
    st.zero_()
    if stats_from is not None:
        st.copy_(torch.as_tensor(stats_from, dtype=torch.int64))
    for _ in range(calls):
        out = ops.block_motion(tc, tr, fmt, records=rec, sad=sad, stats=st, **kw)
        assert out[0].data_ptr() == rec.data_ptr() and out[1].data_ptr() == sad.data_ptr() and out[2].data_ptr() == st.data_ptr()
    torch.cuda.synchronize()
    assert bool((rbuf[n * 8:] == GUARD16).all()) and bool((sbuf[n:] == GUARD).all()) and bool((tbuf[oracle.NSTATS:] == GUARD).all())
    assert torch.equal(tc, keep_c) and torch.equal(tr, keep_r)
    return rec.cpu().numpy(), sad.cpu().numpy().view(np.uint32), st.cpu().numpy()


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("case", oracle.search_cases(), ids=oracle.case_id)
def test_kernel_equals_the_loop_oracle(dev, case):
    """5 x 7 and 16 x 16 are one block (B = 16) or a few; 37 x 53 has clipped blocks on both edges; R = 32 is larger than every frame here."""
    kind, H, W, B, R, lam = case
    cur, ref = oracle.content(kind, H, W)
    winners = oracle.winners_of(*case)
    for intra in oracle.INTRAS:
        assert _same(_run(dev, cur, ref, B=B, R=R, lam=lam, intra=intra), oracle.outputs(winners, intra)), intra


def test_translation_intra_and_tie_cases_of_the_cpu_file(dev):
    """The other cases of tests/test_block_motion.py: the four translations (every block whose displacement is a candidate comes back with it
    and SAD 0), independent noise (all intra), the intra bound at and one above intra w h, two equal costs decided by the rank."""
    H, W = 37, 53
    for sy, sx in ((3, -5), (-6, 6), (0, 1), (5, 0)):
        cur, ref = oracle.shifted_pair(H, W, sx, sy)
        rec, sad, st = _run(dev, cur, ref, B=8, R=6, lam=2, intra=255)
        assert _same((rec, sad, st), oracle.outputs(oracle.search(cur, ref, 8, 6, 2), 255))
        r = rec.astype(np.int64)
        inside = (r[:, 0] + sx >= 0) & (r[:, 0] + r[:, 2] + sx <= W) & (r[:, 1] + sy >= 0) & (r[:, 1] + r[:, 3] + sy <= H)
        assert inside.sum() >= 20 and (r[inside, 4:7] == (4 * sx, 4 * sy, 0)).all() and not sad[inside].any()
    cur, ref = oracle.canvas(oracle.SEED + 1, H, W), oracle.canvas(oracle.SEED + 2, H, W)
    for B in (8, 16):
        rec, sad, st = _run(dev, cur, ref, B=B, R=8, lam=2, intra=20)
        assert (rec[:, 6] == oracle.INTRA_REF).all() and st.tolist() == [rec.shape[0], 0, 0, 0]
        assert _same((rec, sad, st), oracle.outputs(oracle.search(cur, ref, B, 8, 2), 20))
    ref = np.full((8, 8), 100, np.uint8)
    cur = np.full((8, 8), 107, np.uint8)
    assert [a.tolist() for a in _run(dev, cur, ref, B=8, R=2, lam=1, intra=7)] == [[[0, 0, 8, 8, 0, 0, 0, 0]], [448], [0, 1, 448, 64]]
    cur[3, 4] = 108
    assert [a.tolist() for a in _run(dev, cur, ref, B=8, R=2, lam=1, intra=7)] == [[[0, 0, 8, 8, 0, 0, oracle.INTRA_REF, 0]], [449], [1, 0, 0, 0]]
    row = np.where(np.arange(40) % 4 < 2, 40, 200).astype(np.uint8)
    ref = np.ascontiguousarray(np.broadcast_to(row[:32], (16, 32)))
    cur = np.ascontiguousarray(np.broadcast_to(row[1:33], (16, 32)))
    for lam in (0, 1):                                                 # lam = 0: rank decides, (-3, -6) at the inner block; lam = 1: the shortest, (1, 0)
        assert _same(_run(dev, cur, ref, B=8, R=6, lam=lam, intra=255), oracle.outputs(oracle.search(cur, ref, 8, 6, lam), 255))


@functools.lru_cache(maxsize=None)
def _tiles_pair():
    """100 x 150: 4 x 3 tiles of 64 x 32, the last row and column of tiles cut by the frame, clipped blocks at both edges for B = 8 and 16.
    Shifted noise with a rectangle of fresh noise (intra at a moderate bound) over smooth texture in the lower half (near-ties)."""
    H, W = 100, 150
    cur, ref = (p.copy() for p in oracle.shifted_pair(H, W, -5, 3, seed=oracle.SEED + 21))
    tc, tr = oracle.content("texture", 50, W)
    cur[50:], ref[50:] = tc, tr
    cur[20:45, 70:110] = oracle.canvas(oracle.SEED + 22, 25, 40)
    return cur, ref


@functools.lru_cache(maxsize=None)
def _tiles_winners(B, R, lam):
    cur, ref = _tiles_pair()
    return tuple(oracle.search(cur, ref, B, R, lam))


@pytest.mark.parametrize("B", [8, 16])
def test_several_tiles_against_the_loop_oracle(dev, B):
    cur, ref = _tiles_pair()
    for R, lam in ((7, 2), (4, 0)):
        winners = _tiles_winners(B, R, lam)
        want = oracle.outputs(winners, 20)
        assert 0 < want[2][0] < len(winners)                           # some blocks intra, not all
        assert _same(_run(dev, cur, ref, B=B, R=R, lam=lam, intra=20), want), (R, lam)


@pytest.mark.parametrize("B,R", [(8, 32), (16, 32), (16, 13), (8, 18)])
def test_several_tiles_large_radii_against_the_numpy_form(dev, B, R):
    """The window of R = 32 (the largest LDS image) and radii that are no multiple of 4, on several tiles."""
    from arseg_amd import ingest

    cur, ref = _tiles_pair()
    assert _same(_run(dev, cur, ref, B=B, R=R, lam=1, intra=30), ingest.block_motion_numpy(cur, ref, B=B, R=R, lam=1, intra=30))


def test_360x480_against_the_numpy_form(dev):
    """CamVid's frame size at the defaults: 23 x 30 blocks, the bottom row of blocks 8 pixels tall."""
    from arseg_amd import ingest

    H, W = 360, 480
    cur, ref = (p.copy() for p in oracle.shifted_pair(H, W, 9, -4, seed=oracle.SEED + 31))
    g = np.random.Generator(np.random.PCG64(oracle.SEED + 32))
    cur = np.clip(cur.astype(np.int64) + g.integers(-3, 4, cur.shape), 0, 255).astype(np.uint8)
    cur[100:180, 200:330] = g.integers(0, 256, (80, 130), dtype=np.uint8)
    want = ingest.block_motion_numpy(cur, ref, B=16, R=16, lam=2, intra=24)
    assert want[0].shape == (23 * 30, 8) and 28 <= want[2][0] < 23 * 30 and (want[0][:, 4:6] == (36, -16)).sum() > 400
    assert _same(_run(dev, cur, ref, B=16, R=16, lam=2, intra=24), want)


def test_stats_accumulate_and_outputs_are_optional(dev):
    from arseg_amd import ops

    cur, ref = _tiles_pair()
    want = oracle.outputs(_tiles_winners(16, 7, 2), 20)
    rec, sad, st = _run(dev, cur, ref, calls=2, stats_from=[5, 6, 7, 8], B=16, R=7, lam=2, intra=20)
    assert np.array_equal(rec, want[0]) and np.array_equal(sad, want[1]) and np.array_equal(st, 2 * want[2] + np.array([5, 6, 7, 8]))
    tc, tr = _plane(cur, dev), _plane(ref, dev)
    r2, s2, t2 = ops.block_motion(tc, tr, oracle.NV12, 16, 7, 2, 20, sad=False, stats=False)          # NULL sad, NULL stats; records allocated
    assert s2 is None and t2 is None and np.array_equal(r2.cpu().numpy(), want[0])
    r3, s3, t3 = ops.block_motion(tc, tr, oracle.NV12, 16, 7, 2, 20)                                    # everything allocated, stats from zero
    assert np.array_equal(r3.cpu().numpy(), want[0]) and np.array_equal(s3.cpu().numpy().view(np.uint32), want[1]) and np.array_equal(t3.cpu().numpy(), want[2])


@pytest.mark.parametrize("fmt", oracle.FORMATS)
def test_every_format_and_pitched_views(dev, fmt):
    """Each format's planes searched as their luma8 planes are; then the same planes as columns of wider buffers at an odd sample offset (rows
    at a pitch, no 4-byte alignment for the 8-bit formats), the bytes around them untouched."""
    H, W, B, R = 38, 54, 8, 4
    cur, ref = oracle.format_planes(fmt, H, W)
    want = oracle.outputs(oracle.search(oracle.luma8(cur, fmt), oracle.luma8(ref, fmt), B, R, 2), 40)
    assert _same(_run(dev, cur, ref, fmt, B=B, R=R, lam=2, intra=40), want)
    wide_c, wide_r = (np.full((H, W + 9) + p.shape[2:], 171, p.dtype) for p in (cur, ref))
    wide_c[:, 3:3 + W], wide_r[:, 5:5 + W] = cur, ref
    dc, dr = _plane(wide_c, dev), _plane(wide_r, dev)
    vc, vr = dc[:, 3:3 + W], dr[:, 5:5 + W]
    assert not vc.is_contiguous() and vc.data_ptr() % 4 != 0
    assert _same(_run(dev, vc, vr, fmt, B=B, R=R, lam=2, intra=40), want)
    assert np.array_equal(dc.cpu().numpy().view(wide_c.dtype), wide_c) and np.array_equal(dr.cpu().numpy().view(wide_r.dtype), wide_r)
    assert _same(_run(dev, vc[None], vr[None], fmt, B=16, R=R, lam=2, intra=40)[:1],
                 oracle.outputs(oracle.search(oracle.luma8(cur, fmt), oracle.luma8(ref, fmt), 16, R, 2), 40)[:1])          # a batch axis of one


def test_ref_index_is_written_through(dev):
    cur, ref = _tiles_pair()
    winners = _tiles_winners(16, 7, 2)
    for ref_index in (1, 15):
        want = oracle.outputs(winners, 20, ref_index)
        assert set(want[0][:, 6].tolist()) == {ref_index, oracle.INTRA_REF}
        assert _same(_run(dev, cur, ref, B=16, R=7, lam=2, intra=20, ref_index=ref_index), want)


def test_wrapper_refuses_what_the_header_refuses(dev):
    from arseg_amd import _lib, ingest, ops

    a = torch.zeros((32, 48), dtype=torch.uint8, device=dev)
    for kw in ({"B": 12}, {"R": 0}, {"R": 33}, {"lam": 256}, {"intra": -1}, {"ref_index": 16}):
        with pytest.raises(_lib.ArsegError):
            ops.block_motion(a, a, oracle.NV12, **kw)
    with pytest.raises(_lib.ArsegError):
        ops.block_motion(a, a[:16], oracle.NV12)
    with pytest.raises(_lib.ArsegError):
        ops.block_motion(a, a, oracle.P010)                            # uint8 samples for a 16-bit format
    with pytest.raises(_lib.ArsegError):
        ops.block_motion(a.cpu(), a.cpu(), oracle.NV12)
    with pytest.raises(_lib.ArsegError):
        ops.block_motion(a, a, oracle.NV12, records=torch.zeros((5, 8), dtype=torch.int16, device=dev))
    with pytest.raises(_lib.ArsegError):
        ops.block_motion(a.t(), a.t(), oracle.NV12)                    # columns are not rows
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(32, 48, block=4, device=dev)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(32, 48, device="cpu")


def test_c_abi_refuses_bad_arguments(dev):
    """Every ARSEG_EINVAL of the header through the C ABI, before any launch (the pointers are never dereferenced).  The workspace need is 0
    for every shape, so ARSEG_EWORKSPACE cannot arise; a NULL workspace of 0 bytes is what every launch of this file passes."""
    from arseg_amd import _lib

    lib = _lib.load()
    for shape in ((720, 960, 16, 16), (1024, 2048, 8, 32), (0, 0, 16, 16)):
        assert lib.arseg_block_motion_workspace_bytes(*shape) == 0
    for name, args, want in oracle.abi_cases():
        assert lib.arseg_block_motion_fwd(*args) == want, name


def _frames(planes, dev):
    """One-frame NV12 DecodedFrames over static luma buffers (chroma is never read by the search)."""
    from arseg_amd import ingest

    H, W = planes[0].shape
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(_plane(p, dev), uv) for p in planes]


def test_estimator_feeds_the_chain_over_a_gop(dev):
    """Five frames of a panned canvas, a rectangle of fresh noise in frame 3: MotionEstimator + MotionChain(track_links=True) leave the
    merged field, link bytes and link counts that chain_records_numpy gives on the oracle's records."""
    from arseg_amd import ingest

    planes = oracle.gop_frames()
    H, W, gop = planes[0].shape[0], planes[0].shape[1], len(planes)
    frames = _frames(planes, dev)
    est = ingest.MotionEstimator(H, W, block=16, search=8, lam=2, intra=20, device=dev, with_sad=True)
    chain = ingest.MotionChain(H, W, gop=gop, max_ref=1, device=dev, track_links=True)
    assert est.records.shape == (24, 8) and est.sad.shape == (24,) and not bool(est.stats_row().any())
    pushes, total = [], np.zeros(oracle.NSTATS, np.int64)
    for f in range(1, gop):
        want = oracle.outputs(oracle.search(planes[f], planes[f - 1], 16, 8, 2), 20)
        rec = est.estimate(frames[f], frames[f - 1])
        assert rec.data_ptr() == est.records.data_ptr()
        chain.push(rec)
        total += want[2]
        assert np.array_equal(rec.cpu().numpy(), want[0]) and np.array_equal(est.sad.cpu().numpy().view(np.uint32), want[1])
        assert np.array_equal(est.stats_row().cpu().numpy(), total)
        pushes.append((f, want[0]))
    assert total[0] > 0
    merged, link = ingest.chain_records_numpy(pushes, H, W, gop, 1, return_link=True)
    assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
    assert np.array_equal(chain.link_stats().cpu().numpy()[1:], mv_link_oracle.stats(link)[1:])
    assert (link[3:] & ingest.LINK_INTRA).any() and not (link & (ingest.LINK_CLAMPED | ingest.LINK_UNCOVERED)).any()
    est.reset_stats()
    assert not bool(est.stats_row().any())
    with pytest.raises(Exception):
        est.estimate(frames[1][0:1], ingest.DecodedFrames.rgb8(torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)))          # two formats


def test_graph_replays_estimate_and_push_on_new_frames(dev):
    """reset + estimate + push over two static frame buffers in one torch.cuda.graph (a linear chain of launches); the buffers are refilled
    with other frame pairs and the graph replayed: records, merged, link bytes and counts are those of the frames in the buffers."""
    from arseg_amd import ingest

    planes = oracle.gop_frames()
    H, W = planes[0].shape
    prev, cur = _frames([np.zeros_like(planes[0]), np.zeros_like(planes[0])], dev)
    est = ingest.MotionEstimator(H, W, block=16, search=8, lam=2, intra=20, device=dev)
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
        want = oracle.outputs(oracle.search(planes[f], planes[f - 1], 16, 8, 2), 20)
        assert np.array_equal(replayed[0].cpu().numpy(), want[0]) and np.array_equal(replayed[4].cpu().numpy(), want[2])
        eager = step()
        torch.cuda.synchronize()
        assert torch.equal(est.records, replayed[0]) and torch.equal(eager, replayed[1]) and torch.equal(chain.link(), replayed[2])
        assert torch.equal(chain.link_stats(), replayed[3]) and torch.equal(est.stats_row(), replayed[4])
