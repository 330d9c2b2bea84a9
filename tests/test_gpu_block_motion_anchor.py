"""GPU checks of the keyframe anchoring (csrc/block_motion_anchor.hip: arseg_block_motion_anchor_fwd; ops.block_motion_anchor,
ingest.MotionEstimator(anchor_refine=...)) against the loop oracle of tests/block_motion_anchor_oracle.py and, where the loops would take too
long, against ingest.block_motion_anchor_numpy, which tests/test_block_motion_anchor.py holds to that oracle.  Integers in, integers out:
every comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import block_motion_anchor_oracle as oracle
import mv_link_oracle

pytestmark = pytest.mark.gpu

GUARD16, GUARD = 0x5a5a, 0x5a
SAD0 = 0x01020304                                                      # what sad holds before a call: entries of blocks kept on their hop stay so


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plane(a, dev):
    """A luma plane on the device as the anchor takes it: rows (W + 3) & ~3 bytes apart (the bytes beyond W are not pixels), the base aligned."""
    H, W = a.shape
    buf = torch.full((H, (W + 3) & ~3), 0xa5, dtype=torch.uint8, device=dev)
    buf[:, :W] = _dev(a, dev)
    return buf[:, :W]


def _run(dev, cur, key, records, mp, f, B, r, lam, intra, calls=1, stats_from=None, planes=None):
    """ops.block_motion_anchor into buffers with guard words behind out, sad and stats.  After the calls: every guard and every input as they
    were.  ``planes``: device planes to use instead of uploads of cur and key.  Returns numpy (out, sad_of_anchored, stats) in the oracle's form."""
    from arseg_amd import ops

    pc, pk = planes if planes is not None else (_plane(cur, dev), _plane(key, dev))
    rin, mpd = _dev(records, dev), None if mp is None else _dev(mp, dev)
    keep = [t.clone() for t in (pc, pk, rin)] + [None if mpd is None else mpd.clone()]
    n = len(records)
    rbuf = torch.full(((n + 2) * 8,), GUARD16, dtype=torch.int16, device=dev)
    sbuf = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    tbuf = torch.full((oracle.NSTATS + 2,), GUARD, dtype=torch.int64, device=dev)
    out, sad, st = rbuf[:n * 8].view(n, 8), sbuf[:n], tbuf[:oracle.NSTATS]
    sad.fill_(SAD0)
    st.zero_()
    if stats_from is not None:
        st.copy_(torch.as_tensor(stats_from, dtype=torch.int64))
    for _ in range(calls):
        got = ops.block_motion_anchor(pc, pk, rin, mpd, f, B, r, lam, intra, out=out, sad=sad, stats=st)
        assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == sad.data_ptr() and got[2].data_ptr() == st.data_ptr()
    torch.cuda.synchronize()
    assert bool((rbuf[n * 8:] == GUARD16).all()) and bool((sbuf[n:] == GUARD).all()) and bool((tbuf[oracle.NSTATS:] == GUARD).all())
    assert torch.equal(pc, keep[0]) and torch.equal(pk, keep[1]) and torch.equal(rin, keep[2]) and (mpd is None or torch.equal(mpd, keep[3]))
    s = sad.cpu().numpy().astype(np.int64)
    return out.cpu().numpy(), np.where(s == SAD0, -1, s), st.cpu().numpy()


def _run_case(dev, c, **kw):
    c = dict(c, **kw)
    return _run(dev, c["cur"], c["key"], c["records"], c["mp"], c["f"], c["B"], c["r"], c["lam"], c["intra"])


@pytest.mark.parametrize("case", oracle.grid_cases(), ids=oracle.case_id)
def test_kernel_equals_the_loop_oracle(dev, case):
    """The grid of tests/test_block_motion_anchor.py: every r (a template instance each, with B), lam, intra and f."""
    kind, H, W, B = case
    cur, key, rec, mp = oracle.case(*case)
    pc, pk = _plane(cur, dev), _plane(key, dev)
    for r in oracle.REFINES:
        for lam in oracle.LAMS:
            win = oracle.winners_of(kind, H, W, B, r, lam)
            for intra in oracle.INTRAS:
                for f in oracle.FRAMES:
                    assert oracle.same(_run(dev, cur, key, rec, mp, f, B, r, lam, intra, planes=(pc, pk)), oracle.outputs(win, rec, f, intra, H, W, B)), (r, lam, intra, f)


@pytest.mark.parametrize("name", sorted(oracle.hand_cases()))
def test_hand_built_cases_equal_the_loops(dev, name):
    c = oracle.hand_cases()[name]
    assert oracle.same(_run_case(dev, c), oracle.anchor(c["cur"], c["key"], c["records"], c["mp"], c["f"], c["B"], c["r"], c["lam"], c["intra"]))


def test_f_1_copies_through_and_touches_nothing_else(dev):
    from arseg_amd import ops

    cur, key, rec, mp = oracle.case("noise", 37, 53, 16)
    out, sad, st = _run(dev, cur, key, rec, None, 1, 16, 2, 2, 255, stats_from=[5, 6, 7, 8])
    assert np.array_equal(out, rec) and (sad == -1).all() and np.array_equal(st, [5, 6, 7, 8])
    out, sad, st = _run(dev, cur, key, rec, mp, 1, 16, 2, 2, 255)                                                   # merged_prev given: still not read
    assert np.array_equal(out, rec) and (sad == -1).all() and not st.any()
    o2, s2, t2 = ops.block_motion_anchor(_plane(cur, dev), _plane(key, dev), _dev(rec, dev), None, 1, 16, 2, 2, 255, sad=False, stats=False)
    assert s2 is None and t2 is None and np.array_equal(o2.cpu().numpy(), rec)


def test_acceptance_bound_at_and_one_above(dev):
    at, above = oracle.bound_case(0), oracle.bound_case(1)
    out, sad, st = _run_case(dev, at)
    assert tuple(out[0]) == (0, 0, 16, 16, 0, 0, 1, 0) and sad[0] == 3 * 256 and tuple(st) == (1, 0, 0, 4)
    out, sad, st = _run_case(dev, above)
    assert np.array_equal(out, above["records"]) and sad[0] == -1 and tuple(st) == (0, 0, 1, 0)
    out, sad, st = _run_case(dev, above, intra=4)
    assert out[0, 6] == 1 and sad[0] == 3 * 256 + 1


@pytest.mark.parametrize("B,r", [(16, 2), (8, 3), (16, 1)])
def test_100x150_against_the_numpy_form_stats_accumulate_outputs_optional(dev, B, r):
    """7 x 10 or 13 x 19 blocks: several waves and, at B = 8, several workgroups; clipped blocks on both edges."""
    from arseg_amd import ingest, ops

    cur, key, rec, mp = oracle.tiles_case(B=B)
    want = ingest.block_motion_anchor_numpy(cur, key, rec, mp, 4, B=B, r=r, lam=2, intra=20)
    assert 0 < want[2][2] and 0 < want[2][1] < want[2][0] and want[2][3] > 0
    assert oracle.same(_run(dev, cur, key, rec, mp, 4, B, r, 2, 20), want)
    out, sad, st = _run(dev, cur, key, rec, mp, 4, B, r, 2, 20, calls=2, stats_from=[5, 6, 7, 8])
    assert np.array_equal(out, want[0]) and np.array_equal(sad, want[1]) and np.array_equal(st, 2 * want[2] + np.array([5, 6, 7, 8]))
    args = (_plane(cur, dev), _plane(key, dev), _dev(rec, dev), _dev(mp, dev), 4, B, r, 2, 20)
    o2, s2, t2 = ops.block_motion_anchor(*args, sad=False, stats=False)                                              # NULL sad and stats
    assert s2 is None and t2 is None and np.array_equal(o2.cpu().numpy(), want[0])
    o3, s3, t3 = ops.block_motion_anchor(*args)                                                                      # everything allocated: sad and stats from zero
    assert np.array_equal(o3.cpu().numpy(), want[0]) and np.array_equal(t3.cpu().numpy(), want[2])
    assert np.array_equal(s3.cpu().numpy().astype(np.int64), np.where(want[1] < 0, 0, want[1]))


def test_360x480_against_the_numpy_form(dev):
    """CamVid's frame size: 23 x 30 blocks, more than two workgroups per compute unit would take at once: the grid's stride is walked."""
    from arseg_amd import ingest

    cur, key, rec, mp = oracle.tiles_case(360, 480, 16, oracle.SEED + 33)
    want = ingest.block_motion_anchor_numpy(cur, key, rec, mp, 7, B=16, r=2, lam=2, intra=24)
    assert want[0].shape == (23 * 30, 8) and 400 < want[2][0] < 23 * 30 and want[2][1] > 20
    assert oracle.same(_run(dev, cur, key, rec, mp, 7, 16, 2, 2, 24), want)


def test_pitched_planes_and_level_0_of_a_pyramid(dev):
    """The planes as columns of wider buffers (a pitch above the row, a base 4 bytes in, other bytes around them untouched and never read as
    pixels: W = 53 leaves three bytes of the last dword to the neighbour), and as level 0 of a LumaPyramid."""
    from arseg_amd import ingest

    H, W, B = 37, 53, 8
    cur, key, rec, mp = oracle.case("noise", H, W, B)
    want = oracle.outputs(oracle.winners_of("noise", H, W, B, 2, 3), rec, 5, 20, H, W, B)
    wide = []
    for p, pad, fill in ((cur, 64, 171), (key, 72, 33)):
        wbuf = np.full((H, pad), fill, np.uint8)
        wbuf[:, 4:4 + W] = p
        wide.append(_dev(wbuf, dev))
    views = tuple(t[:, 4:4 + W] for t in wide)
    assert not views[0].is_contiguous() and views[0].data_ptr() % 4 == 0 and views[1].stride(0) == 72
    assert oracle.same(_run(dev, cur, key, rec, mp, 5, B, 2, 3, 20, planes=views), want)
    grey = lambda p: ingest.DecodedFrames.rgb8(_dev(np.repeat(p[..., None], 3, axis=2), dev))            # luma8 of (v, v, v) is v; 4:2:0 needs even sizes
    pyr = [ingest.LumaPyramid(H, W, 1, dev).build(grey(p)) for p in (cur, key)]
    assert pyr[0].level(0).stride(0) == 64
    assert oracle.same(_run(dev, cur, key, rec, mp, 5, B, 2, 3, 20, planes=(pyr[0].level(0), pyr[1].level(0))), want)


def _frames(planes, dev):
    from arseg_amd import ingest

    H, W = planes[0].shape
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(_dev(p, dev), uv) for p in planes]


@pytest.mark.parametrize("levels", [0, 2])
def test_estimator_anchors_the_chain_over_the_capability_gop(dev, levels):
    """The panned GOP with an occluder in frame 2 (tests/test_block_motion_anchor.py establishes what anchoring does on it) through
    MotionEstimator + MotionChain(max_ref=16, track_links=True): records, merged, link bytes, link counts and anchor counts equal the host chain
    over the host forms.  levels=0 reads the frames' own luma planes; levels=2 searches hierarchically and anchors on level 0 of its pyramids."""
    from arseg_amd import ingest

    cap = oracle.CAP
    planes = oracle.gop_frames()
    H, W = planes[0].shape
    search = cap["R"] if levels == 0 else 2
    if levels:
        hop = lambda c, p: ingest.block_motion_pyr_numpy(c, p, B=cap["B"], Rt=search, r=1, lam=cap["lam"], intra=cap["intra"], levels=levels)[0]
    else:
        hop = lambda c, p: ingest.block_motion_numpy(c, p, B=cap["B"], R=search, lam=cap["lam"], intra=cap["intra"])[0]
    anchor = lambda c, k, rec, mp, f: ingest.block_motion_anchor_numpy(c, k, rec, mp, f, B=cap["B"], r=cap["r"], lam=cap["lam"], intra=cap["intra"])
    merged, link, pushes, stats = oracle.run_gop(hop, anchor)
    frames = _frames(planes, dev)
    est = ingest.MotionEstimator(H, W, block=cap["B"], search=search, lam=cap["lam"], intra=cap["intra"], device=dev, with_sad=True, levels=levels, refine=1,
                                 anchor_refine=cap["r"], anchor_intra=cap["intra"])
    chain = ingest.MotionChain(H, W, gop=oracle.GOP, max_ref=cap["max_ref"], device=dev, track_links=True)
    est.set_key(frames[0])
    total = np.zeros(oracle.NSTATS, np.int64)
    for f in range(1, oracle.GOP):
        rec = est.estimate_anchored(frames[f], frames[f - 1], chain)
        assert rec.data_ptr() == est.anchored.data_ptr() and rec.data_ptr() != est.records.data_ptr()
        assert np.array_equal(rec.cpu().numpy(), pushes[f - 1][1]), f
        chain.push(rec)
        total += stats[f]
        assert np.array_equal(est.anchor_stats_row().cpu().numpy(), total)
    assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
    assert np.array_equal(chain.link_stats().cpu().numpy()[1:], mv_link_oracle.stats(link)[1:])
    if levels == 0:                                                    # the capability itself, on the device's own output
        got, lk = chain.mv_q().cpu().numpy(), chain.link().cpu().numpy()
        for f in (3, 4, 5):
            assert oracle.off_truth(got[f], f) == 0 and np.array_equal(lk[f] & 7 != 0, oracle.leaves_frame(f))
    est.reset_stats()
    assert not est.anchor_stats_row().any() and not est.stats_row().any()


def test_graph_replays_estimate_anchor_and_push_on_new_frames(dev):
    """Frame 3 of the capability GOP: the chain holds frames 1 and 2; estimate + anchor + push for the fixed f = 3 in one torch.cuda.graph over
    static frame buffers, replayed on other frame pairs (the chain is wound back to f = 2 on the host between replays: push itself is
    launches only)."""
    from arseg_amd import ingest

    cap = oracle.CAP
    planes = oracle.gop_frames()
    H, W = planes[0].shape
    frames = _frames(planes, dev)
    prev, cur = _frames([np.zeros_like(planes[0]), np.zeros_like(planes[0])], dev)
    est = ingest.MotionEstimator(H, W, block=cap["B"], search=cap["R"], lam=cap["lam"], intra=cap["intra"], device=dev, anchor_refine=cap["r"], anchor_intra=cap["intra"])
    chain = ingest.MotionChain(H, W, gop=oracle.GOP, max_ref=cap["max_ref"], device=dev, track_links=True)
    est.set_key(frames[0])
    for f in (1, 2):
        chain.push(est.estimate_anchored(frames[f], frames[f - 1], chain))
    merged2 = chain.merged[2].cpu().numpy()

    def step():
        chain.f = 2
        est.reset_stats()
        return chain.push(est.estimate_anchored(cur, prev, chain))

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for a, b in ((3, 2), (4, 3), (2, 1), (3, 2)):
        prev.planes[0].copy_(_dev(planes[b], dev)[None])
        cur.planes[0].copy_(_dev(planes[a], dev)[None])
        est.anchored.fill_(GUARD16)
        graph.replay()
        torch.cuda.synchronize()
        replayed = (est.anchored.clone(), out.clone(), chain.link()[3].clone(), est.anchor_stats_row().clone())
        hop = ingest.block_motion_numpy(planes[a], planes[b], B=cap["B"], R=cap["R"], lam=cap["lam"], intra=cap["intra"])[0]
        want = ingest.block_motion_anchor_numpy(planes[a], planes[0], hop, merged2, 3, B=cap["B"], r=cap["r"], lam=cap["lam"], intra=cap["intra"])
        assert np.array_equal(replayed[0].cpu().numpy(), want[0]) and np.array_equal(replayed[3].cpu().numpy(), want[2])
        eager = step()
        torch.cuda.synchronize()
        assert torch.equal(est.anchored, replayed[0]) and torch.equal(eager, replayed[1]) and torch.equal(chain.link()[3], replayed[2])
        assert torch.equal(est.anchor_stats_row(), replayed[3])


def test_anchor_refine_0_is_the_estimator_as_it_was(dev):
    from arseg_amd import _lib, ingest

    planes = oracle.gop_frames()
    H, W = planes[0].shape
    frames = _frames(planes[:3], dev)
    a = ingest.MotionEstimator(H, W, search=8, intra=20, device=dev)
    b = ingest.MotionEstimator(H, W, search=8, intra=20, device=dev, anchor_refine=2, anchor_intra=20)
    assert torch.equal(a.estimate(frames[2], frames[1]), b.estimate(frames[2], frames[1])) and torch.equal(a.stats_row(), b.stats_row())
    assert not hasattr(a, "anchored") and not hasattr(a, "anchor_stats")
    chain = ingest.MotionChain(H, W, gop=4, max_ref=16, device=dev)
    for fn in (lambda: a.set_key(frames[0]), lambda: a.estimate_anchored(frames[1], frames[0], chain), lambda: a.anchor_stats_row()):
        with pytest.raises(_lib.ArsegError):
            fn()


def test_wrappers_refuse(dev):
    from arseg_amd import _lib, ingest, ops

    H, W, B = 37, 53, 16
    cur, key, rec, mp = oracle.case("noise", H, W, B)
    cur, key, rec, mp = _plane(cur, dev), _plane(key, dev), _dev(rec, dev), _dev(mp, dev)
    ok = dict(f=2, B=B, r=2, lam=2, intra=20)
    for kw in (dict(B=12), dict(r=0), dict(r=4), dict(lam=256), dict(intra=-1), dict(f=0), dict(f=17)):
        with pytest.raises(_lib.ArsegError):
            ops.block_motion_anchor(cur, key, rec, mp, **dict(ok, **kw))
    wide = torch.zeros((H, 64), dtype=torch.uint8, device=dev)
    bad = [lambda: ops.block_motion_anchor(cur, key, rec, None, **ok),                              # merged_prev missing at f = 2
           lambda: ops.block_motion_anchor(cur, key, rec, mp, out=rec, **ok),                        # in place
           lambda: ops.block_motion_anchor(cur, key, rec[:-1], mp, **ok),                            # one record short of the grid
           lambda: ops.block_motion_anchor(wide[:, 1:1 + W], key, rec, mp, **ok),                    # base not 4-byte aligned
           lambda: ops.block_motion_anchor(cur, torch.zeros((H, W + 1), dtype=torch.uint8, device=dev)[:, :W], rec, mp, **ok),     # pitch 54
           lambda: ops.block_motion_anchor(cur, key[:-1], rec, mp, **ok),
           lambda: ops.block_motion_anchor(cur.cpu(), key, rec, mp, **ok),
           lambda: ops.block_motion_anchor(cur, key, rec, mp[..., :1], **ok),
           lambda: ops.block_motion_anchor(cur, key, rec, mp.to(torch.int32), **ok),
           lambda: ops.block_motion_anchor(cur, key, rec, mp, stats=torch.zeros(3, dtype=torch.int64, device=dev), **ok)]
    for fn in bad:
        with pytest.raises(_lib.ArsegError):
            fn()
    both = torch.zeros((2 * len(rec) - 1, 8), dtype=torch.int16, device=dev)                          # two views that share one record
    with pytest.raises(_lib.ArsegError):
        ops.block_motion_anchor(cur, key, both[:len(rec)], mp, out=both[len(rec) - 1:], **ok)
    # the estimator
    planes = oracle.gop_frames()
    H, W = planes[0].shape
    frames = _frames(planes[:3], dev)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(H, W, device=dev, anchor_refine=4)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionEstimator(H, W, device=dev, anchor_refine=1, anchor_intra=256)
    est = ingest.MotionEstimator(H, W, search=4, device=dev, anchor_refine=1)
    chain = ingest.MotionChain(H, W, gop=4, max_ref=16, device=dev)
    with pytest.raises(_lib.ArsegError):                                                            # before set_key
        est.estimate_anchored(frames[1], frames[0], chain)
    rgb = ingest.DecodedFrames.rgb8(torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.ArsegError, match="levels >= 1"):                                       # levels=0 reads the frame's own luma plane
        est.set_key(rgb)
    odd = torch.zeros((1, H, W + 4), dtype=torch.uint8, device=dev)[:, :, 1:1 + W]
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.ArsegError, match="levels >= 1"):
        est.set_key(ingest.DecodedFrames.nv12(odd, uv))
    est.set_key(frames[0])
    for bad_chain in (ingest.MotionChain(H, W, gop=4, max_ref=16, device=dev, bidirectional=True), ingest.MotionChain(H + 16, W, gop=4, max_ref=16, device=dev)):
        with pytest.raises(_lib.ArsegError):
            est.estimate_anchored(frames[1], frames[0], bad_chain)
    short = ingest.MotionChain(H, W, gop=4, max_ref=1, device=dev)
    short.push(est.estimate_anchored(frames[1], frames[0], short))                                  # f = 1 <= max_ref
    with pytest.raises(_lib.ArsegError):                                                            # f = 2 > max_ref = 1: ref = 1 would be unusable
        est.estimate_anchored(frames[2], frames[1], short)
    est2 = ingest.MotionEstimator(H, W, search=2, device=dev, levels=1, anchor_refine=1)
    est2.set_key(rgb)                                                                               # with a pyramid any format anchors
    est2.set_key(ingest.LumaPyramid(H, W, 2, dev).build(frames[0]))
    with pytest.raises(_lib.ArsegError):
        est2.set_key(ingest.LumaPyramid(H + 2, W, 1, dev))


def test_c_abi_refuses_bad_arguments(dev):
    from arseg_amd import _lib

    lib = _lib.load()
    for name, args, want in oracle.abi_cases():
        assert lib.arseg_block_motion_anchor_fwd(*args) == want, name
