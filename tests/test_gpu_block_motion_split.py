"""GPU checks of the quad-tree split (csrc/block_motion_split.hip: arseg_block_motion_split_fwd; ops.block_motion_split,
ingest.MotionEstimator(split_refine=...)) against the loop oracle of tests/block_motion_split_oracle.py and, where the loops would take too
long, against ingest.block_motion_split_numpy, which tests/test_block_motion_split.py holds to that oracle.  Integers in, integers out: every
comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import block_motion_split_oracle as oracle
import mv_link_oracle

pytestmark = pytest.mark.gpu

GUARD16, GUARD = 0x5a5a, 0x5a


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plane(a, dev):
    """A luma plane on the device as the split takes it: rows (W + 3) & ~3 bytes apart (the bytes beyond W are not pixels), the base aligned."""
    H, W = a.shape
    buf = torch.full((H, (W + 3) & ~3), 0xa5, dtype=torch.uint8, device=dev)
    buf[:, :W] = _dev(a, dev)
    return buf[:, :W]


def _run(dev, cur, ref, records, r, lam, intra, gain, ref_index=0, calls=1, stats_from=None, planes=None):
    """ops.block_motion_split into buffers with guard words behind children, sad and stats, all three filled with the guard before the call (so
    a row that is not written shows).  After the calls: every guard and every input as they were.  Returns numpy (children, sad, stats)."""
    from arseg_amd import ops

    pc, pr = planes if planes is not None else (_plane(cur, dev), _plane(ref, dev))
    rin = _dev(records, dev)
    keep = [t.clone() for t in (pc, pr, rin)]
    n = 4 * len(records)
    rbuf = torch.full(((n + 2) * 8,), GUARD16, dtype=torch.int16, device=dev)
    sbuf = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    tbuf = torch.full((oracle.NSTATS + 2,), GUARD, dtype=torch.int64, device=dev)
    out, sad, st = rbuf[:n * 8].view(n, 8), sbuf[:n], tbuf[:oracle.NSTATS]
    st.zero_()
    if stats_from is not None:
        st.copy_(torch.as_tensor(stats_from, dtype=torch.int64))
    for _ in range(calls):
        got = ops.block_motion_split(pc, pr, rin, r, lam, intra, gain, ref_index, children=out, sad=sad, stats=st)
        assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == sad.data_ptr() and got[2].data_ptr() == st.data_ptr()
    torch.cuda.synchronize()
    assert bool((rbuf[n * 8:] == GUARD16).all()) and bool((sbuf[n:] == GUARD).all()) and bool((tbuf[oracle.NSTATS:] == GUARD).all())
    assert torch.equal(pc, keep[0]) and torch.equal(pr, keep[1]) and torch.equal(rin, keep[2])
    return out.cpu().numpy(), sad.cpu().numpy().view(np.uint32), st.cpu().numpy()


@pytest.mark.parametrize("case", oracle.grid_cases(), ids=oracle.case_id)
def test_kernel_equals_the_loop_oracle(dev, case):
    """The grid of tests/test_block_motion_split.py: every r (a template instance each), lam, intra and split_gain."""
    cur, ref, rec = oracle.grid_case(*case)
    planes = (_plane(cur, dev), _plane(ref, dev))
    for r in oracle.REFINES:
        for lam in oracle.LAMS:
            found = oracle.grid_found(*case, r, lam)
            for intra in oracle.INTRAS:
                for gain in oracle.GAINS:
                    assert oracle.same(_run(dev, cur, ref, rec, r, lam, intra, gain, planes=planes), oracle.outputs(found, lam, intra, gain)), (r, lam, intra, gain)


@pytest.mark.parametrize("case", oracle.noise_cases(), ids=oracle.case_id)
def test_seeded_noise_cases_equal_the_loops_stats_accumulate_runs_repeat(dev, case):
    """37 x 53, 48 x 64 and 100 x 150 (70 parents: five workgroups' worth of waves) with hand-planted records: unusable refs, vectors of 500 and
    501 pixels, parents that leave the frame.  tests/test_block_motion_split.py asserts their spread."""
    H, W = case
    cur, ref, rec = oracle.noise_case(H, W)
    n = oracle.NOMINAL
    for r, lam in ((n["r"], n["lam"]), (3, 0), (1, 3)):
        want = oracle.outputs(oracle.noise_found(H, W, r, lam), lam, n["intra"], n["split_gain"])
        first = _run(dev, cur, ref, rec, r, lam, n["intra"], n["split_gain"])
        assert oracle.same(first, want), (r, lam)
        again = _run(dev, cur, ref, rec, r, lam, n["intra"], n["split_gain"], calls=2, stats_from=[5, 6, 7, 8, 9, 10])
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
        assert np.array_equal(again[2], 2 * want[2] + np.array([5, 6, 7, 8, 9, 10]))


@pytest.mark.parametrize("name", sorted(oracle.rank_cases()))
def test_rank_rule_on_constant_and_striped_images(dev, name):
    cur, ref, rec, r, lam = oracle.rank_cases()[name]
    assert oracle.same(_run(dev, cur, ref, rec, r, lam, 255, 0), oracle.outputs(oracle.search(cur, ref, rec, r, lam), lam, 255, 0))


def test_ref_index_3(dev):
    cur, ref, rec = oracle.noise_case(48, 64)
    rec = rec.copy()
    rec[rec[:, 6] == 0, 6] = 3
    rec[5, 6] = 0
    assert oracle.same(_run(dev, cur, ref, rec, 2, 3, 20, 32, ref_index=3), oracle.outputs(oracle.search(cur, ref, rec, 2, 3, 3), 3, 20, 32, 3))


def test_360x480_against_the_numpy_form(dev):
    """CamVid's frame size: 23 x 30 parents, more than 43 workgroups of 16 waves."""
    from arseg_amd import ingest

    H, W = 360, 480
    g = np.random.Generator(np.random.PCG64(oracle.SEED + 33))
    ref, cur = oracle.two_layer_frames(H, W, 248, 2, oracle.SEED + 34)
    cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    cur[100:140, 300:360] = g.integers(0, 256, (40, 60), dtype=np.uint8)
    rec = oracle.grid_records(H, W, 4 * oracle.LEFT[0], 4 * oracle.LEFT[1])
    rec[g.integers(0, 10, len(rec)) == 0, 4:7] = (0, 0, oracle.INTRA_REF)
    want = ingest.block_motion_split_numpy(cur, ref, rec, 2, 2, 20, 32)
    assert want[0].shape == (4 * 23 * 30, 8) and 100 < want[2][0] < 23 * 30 and want[2][1] > 20 and want[2][3] > 0
    assert oracle.same(_run(dev, cur, ref, rec, 2, 2, 20, 32), want)


def test_pitched_planes_level_0_of_a_pyramid_and_optional_outputs(dev):
    """The planes as columns of wider buffers (a pitch above the row, a base 4 bytes in; W = 53 leaves three bytes of the last dword to the
    neighbour), as level 0 of a LumaPyramid, and the call with sad and stats left out or allocated."""
    from arseg_amd import ingest, ops

    H, W = 37, 53
    cur, ref, rec = oracle.noise_case(H, W)
    want = oracle.outputs(oracle.noise_found(H, W, 2, 3), 3, 20, 32)
    wide = []
    for p, pad, fill in ((cur, 64, 171), (ref, 72, 33)):
        wbuf = np.full((H, pad), fill, np.uint8)
        wbuf[:, 4:4 + W] = p
        wide.append(_dev(wbuf, dev))
    views = tuple(t[:, 4:4 + W] for t in wide)
    assert not views[0].is_contiguous() and views[0].data_ptr() % 4 == 0 and views[1].stride(0) == 72
    assert oracle.same(_run(dev, cur, ref, rec, 2, 3, 20, 32, planes=views), want)
    grey = lambda p: ingest.DecodedFrames.rgb8(_dev(np.repeat(p[..., None], 3, axis=2), dev))            # luma8 of (v, v, v) is v
    pyr = [ingest.LumaPyramid(H, W, 1, dev).build(grey(p)) for p in (cur, ref)]
    assert pyr[0].level(0).stride(0) == 64
    assert oracle.same(_run(dev, cur, ref, rec, 2, 3, 20, 32, planes=(pyr[0].level(0), pyr[1].level(0))), want)
    args = (_plane(cur, dev), _plane(ref, dev), _dev(rec, dev), 2, 3, 20, 32)
    c2, s2, t2 = ops.block_motion_split(*args, sad=False, stats=False)                                  # NULL sad and stats
    assert s2 is None and t2 is None and np.array_equal(c2.cpu().numpy(), want[0])
    c3, s3, t3 = ops.block_motion_split(*args)                                                          # everything allocated: stats from zero
    assert np.array_equal(c3.cpu().numpy(), want[0]) and np.array_equal(s3.cpu().numpy().view(np.uint32), want[1]) and np.array_equal(t3.cpu().numpy(), want[2])


def test_wrapper_refuses(dev):
    from arseg_amd import _lib, ops

    H, W = 37, 53
    cur, ref, rec = oracle.noise_case(H, W)
    cur, ref, rec = _plane(cur, dev), _plane(ref, dev), _dev(rec, dev)
    n = len(rec)
    for kw in (dict(r=0), dict(r=4), dict(lam=256), dict(intra=-1), dict(split_gain=65536), dict(split_gain=-1), dict(ref_index=16)):
        with pytest.raises(_lib.ArsegError):
            ops.block_motion_split(cur, ref, rec, **kw)
    both = torch.zeros((5 * n - 1, 8), dtype=torch.int16, device=dev)                                # two views that share one record
    wide = torch.zeros((H, 64), dtype=torch.uint8, device=dev)
    bad = [lambda: ops.block_motion_split(cur, ref, both[:n], children=both[n - 1:]),                  # the overlap refusal
           lambda: ops.block_motion_split(cur, ref, both[4 * n - 1:], children=both[:4 * n]),
           lambda: ops.block_motion_split(cur, ref, rec[:-1]),                                         # one record short of the grid
           lambda: ops.block_motion_split(cur, ref, rec, children=torch.zeros((n, 8), dtype=torch.int16, device=dev)),
           lambda: ops.block_motion_split(wide[:, 1:1 + W], ref, rec),                                 # base not 4-byte aligned
           lambda: ops.block_motion_split(cur, torch.zeros((H, W + 1), dtype=torch.uint8, device=dev)[:, :W], rec),      # pitch 54
           lambda: ops.block_motion_split(cur, ref[:-1], rec),
           lambda: ops.block_motion_split(cur.cpu(), ref, rec),
           lambda: ops.block_motion_split(cur, ref, rec, sad=torch.zeros(n, dtype=torch.int32, device=dev)),
           lambda: ops.block_motion_split(cur, ref, rec, stats=torch.zeros(4, dtype=torch.int64, device=dev))]
    for fn in bad:
        with pytest.raises(_lib.ArsegError):
            fn()
    ok = torch.zeros((5 * n, 8), dtype=torch.int16, device=dev)                                       # the estimator's layout: children right behind
    ok[:n] = rec
    ops.block_motion_split(cur, ref, ok[:n], children=ok[n:])
    torch.cuda.synchronize()


# ---- the estimator and the chain ----
GOP = dict(H=80, W=112, border=56, n=5, R=6, lam=2, intra=20, r=2, gain=32)


def _gop_planes():
    return oracle.two_layer_frames(GOP["H"], GOP["W"], GOP["border"], GOP["n"], oracle.SEED + 60)


def _frames(planes, dev):
    from arseg_amd import ingest

    H, W = planes[0].shape
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(_dev(p, dev), uv) for p in planes]


def _host_hop(levels, split):
    from arseg_amd import ingest

    def hop(c, p):
        if levels:
            rec = ingest.block_motion_pyr_numpy(c, p, B=16, Rt=2, r=1, lam=GOP["lam"], intra=GOP["intra"], levels=levels)[0]
        else:
            rec = ingest.block_motion_numpy(c, p, B=16, R=GOP["R"], lam=GOP["lam"], intra=GOP["intra"])[0]
        if not split:
            return rec, None
        children, _, st = ingest.block_motion_split_numpy(c, p, rec, GOP["r"], GOP["lam"], GOP["intra"], GOP["gain"])
        return np.concatenate([rec, children]), st
    return hop


def _exact_pixels(merged):
    """Pixels of frames 1 .. n - 1 whose composed vector is the layer's true one to the keyframe."""
    return sum(int((merged[f] == oracle.true_field(GOP["H"], GOP["W"], GOP["border"], hops=f)).all(axis=-1).sum()) for f in range(1, GOP["n"]))


@pytest.mark.parametrize("levels", [0, 2])
def test_estimator_feeds_the_chain_over_a_two_layer_gop(dev, levels):
    """Five frames of the two-layer scene through MotionEstimator(split_refine=2) + MotionChain(track_links=True): the list pushed, merged, link
    bytes, link counts and split counts equal the host chain over the host forms; more pixels carry the exact vector than with split_refine=0.
    levels=0 reads the frames' own luma planes; levels=2 searches hierarchically and splits on level 0 of its pyramids."""
    from arseg_amd import ingest

    planes = _gop_planes()
    H, W, n = GOP["H"], GOP["W"], GOP["n"]
    frames = _frames(planes, dev)
    search = 2 if levels else GOP["R"]
    results = {}
    for split in (2, 0):
        hop = _host_hop(levels, split)
        est = ingest.MotionEstimator(H, W, search=search, lam=GOP["lam"], intra=GOP["intra"], device=dev, with_sad=True, levels=levels, refine=1, split_refine=split,
                                     split_gain=GOP["gain"])
        chain = ingest.MotionChain(H, W, gop=n, max_ref=1, device=dev, track_links=True)
        pushes, total = [], np.zeros(oracle.NSTATS, np.int64)
        for f in range(1, n):
            rec = est.estimate(frames[f], frames[f - 1])
            want, st = hop(planes[f], planes[f - 1])
            assert np.array_equal(rec.cpu().numpy(), want), (split, f)
            if split:
                assert rec.data_ptr() == est.records_all.data_ptr() == est.records.data_ptr() and rec.shape == (5 * est.n_blocks, 8)
                assert est.children.data_ptr() == rec.data_ptr() + 16 * est.n_blocks and est.child_sad.shape == (4 * est.n_blocks,)
                total += st
                assert np.array_equal(est.split_stats_row().cpu().numpy(), total)
            chain.push(rec)
            pushes.append((f, want))
        merged, link = ingest.chain_records_numpy(pushes, H, W, n, 1, return_link=True)
        assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
        assert np.array_equal(chain.link_stats().cpu().numpy()[1:], mv_link_oracle.stats(link)[1:])
        results[split] = _exact_pixels(chain.mv_q().cpu().numpy())
        if split:
            assert total[0] > 0
            est.reset_stats()
            assert not est.split_stats_row().any() and not est.stats_row().any()
    assert results[2] > results[0], results


def test_graph_replays_estimate_and_push_on_new_frames(dev):
    """estimate (search + split) + push for the fixed f = 2 in one torch.cuda.graph over static frame buffers, replayed on other frame pairs: the
    list has 5 n_blocks records whatever was split (the chain is wound back to f = 1 on the host between replays: push itself is launches only)."""
    from arseg_amd import ingest

    planes = _gop_planes()
    H, W, n = GOP["H"], GOP["W"], GOP["n"]
    frames = _frames(planes, dev)
    prev, cur = _frames([np.zeros_like(planes[0]), np.zeros_like(planes[0])], dev)
    est = ingest.MotionEstimator(H, W, search=GOP["R"], lam=GOP["lam"], intra=GOP["intra"], device=dev, split_refine=GOP["r"], split_gain=GOP["gain"])
    chain = ingest.MotionChain(H, W, gop=n, max_ref=1, device=dev, track_links=True)
    chain.push(est.estimate(frames[1], frames[0]))
    hop = _host_hop(0, True)

    def step():
        chain.f = 1
        est.reset_stats()
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
    for a, b in ((2, 1), (3, 2), (1, 0), (2, 1)):
        prev.planes[0].copy_(_dev(planes[b], dev)[None])
        cur.planes[0].copy_(_dev(planes[a], dev)[None])
        est.records_all.fill_(GUARD16)
        graph.replay()
        torch.cuda.synchronize()
        replayed = (est.records_all.clone(), out.clone(), chain.link()[2].clone(), est.split_stats_row().clone())
        want, st = hop(planes[a], planes[b])
        assert np.array_equal(replayed[0].cpu().numpy(), want) and np.array_equal(replayed[3].cpu().numpy(), st) and st[0] > 0
        eager = step()
        torch.cuda.synchronize()
        assert torch.equal(est.records_all, replayed[0]) and torch.equal(eager, replayed[1]) and torch.equal(chain.link()[2], replayed[2])
        assert torch.equal(est.split_stats_row(), replayed[3])


@pytest.mark.parametrize("levels", [0, 1])
def test_split_refine_0_is_the_estimator_as_it_was(dev, levels):
    from arseg_amd import _lib, ingest

    planes = _gop_planes()
    H, W = GOP["H"], GOP["W"]
    frames = _frames(planes[:3], dev)
    kw = dict(search=2 if levels else GOP["R"], intra=GOP["intra"], device=dev, levels=levels, with_sad=True)
    a, b = ingest.MotionEstimator(H, W, **kw), ingest.MotionEstimator(H, W, split_refine=2, **kw)
    ra, rb = a.estimate(frames[2], frames[1]), b.estimate(frames[2], frames[1])
    want = _host_hop(levels, False)(planes[2], planes[1])[0] if not levels else \
        ingest.block_motion_pyr_numpy(planes[2], planes[1], B=16, Rt=2, r=1, lam=2, intra=GOP["intra"], levels=1)[0]
    assert ra.data_ptr() == a.records.data_ptr() and tuple(ra.shape) == tuple(a.records.shape) == (a.n_blocks, 8) and a.records.is_contiguous()
    assert np.array_equal(ra.cpu().numpy(), want) and torch.equal(ra, b.records) and torch.equal(rb[:b.n_blocks], ra)
    assert torch.equal(a.stats_row(), b.stats_row()) and torch.equal(a.sad, b.sad) and tuple(a.sad.shape) == (a.n_blocks,)
    for name in ("records_all", "children", "split_stats", "child_sad"):
        assert not hasattr(a, name), name
    with pytest.raises(_lib.ArsegError):
        a.split_stats_row()
    a.reset_stats()
    assert not a.stats_row().any()


def test_estimator_refuses_frames_it_cannot_read_in_place(dev):
    from arseg_amd import _lib, ingest

    H, W = GOP["H"], GOP["W"]
    frames = _frames(_gop_planes()[:2], dev)
    est = ingest.MotionEstimator(H, W, search=4, device=dev, split_refine=1)
    rgb = ingest.DecodedFrames.rgb8(torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.ArsegError, match="levels >= 1"):          # levels=0 reads the frame's own luma plane
        est.estimate(rgb, rgb)
    est.estimate(frames[1], frames[0])
    est1 = ingest.MotionEstimator(H, W, search=2, device=dev, levels=1, split_refine=1)
    assert tuple(est1.estimate(rgb, rgb).shape) == (5 * est1.n_blocks, 8)                              # with a pyramid any format splits
    torch.cuda.synchronize()
