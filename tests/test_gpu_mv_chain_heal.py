"""GPU checks of the chain healing (csrc/mv_chain_heal.hip: arseg_mv_chain_heal_fwd; ops.mv_chain_heal, ingest.ChainHealer) against the loop
oracle of tests/mv_chain_heal_oracle.py and, where the loops would take too long, against ingest.mv_chain_heal_numpy, which
tests/test_mv_chain_heal.py holds to that oracle.  Integers in, integers out: every comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import block_motion_anchor_oracle as bma
import mv_chain_heal_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0x5a
SAD0 = 0x01020304                                                      # what sad holds before a call: the entries of skipped blocks stay so


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plane(a, dev):
    """A luma plane on the device as the entry takes it: rows (W + 3) & ~3 bytes apart (the bytes beyond W are not pixels), the base aligned."""
    H, W = a.shape
    buf = torch.full((H, (W + 3) & ~3), 0xa5, dtype=torch.uint8, device=dev)
    buf[:, :W] = _dev(a, dev)
    return buf[:, :W]


class _Bench(object):
    """The device side of one case: the planes and pristine copies of merged, link and row uploaded once; per call the in-place buffers are
    restored on the device, and every output comes back in one copy.  Guard bytes behind every output."""

    def __init__(self, dev, cur, key, merged, link, row, B, planes=None):
        self.H, self.W = link.shape
        self.n = -(-self.H // B) * -(-self.W // B)
        self.B, self.dev = B, dev
        self.pc, self.pk = planes if planes is not None else (_plane(cur, dev), _plane(key, dev))
        self.keep = (self.pc.clone(), self.pk.clone())
        sizes = (4 * self.H * self.W, self.H * self.W, 16 * self.n, 4 * self.n, 8 * oracle.NSTATS, 8 * oracle.LINK_NSTATS)
        self.off = [0]
        for s in sizes:
            self.off.append(self.off[-1] + ((s + 16 + 15) & ~15))                 # at least 16 guard bytes behind each, every start 16-byte aligned
        self.sizes = sizes
        self.buf = torch.empty(self.off[-1], dtype=torch.uint8, device=dev)
        self.init = torch.full((self.off[-1],), GUARD, dtype=torch.uint8, device=dev)
        part = lambda t, i: t[self.off[i]:self.off[i] + sizes[i]]
        part(self.init, 0).copy_(_dev(merged, dev).view(torch.uint8).flatten())
        part(self.init, 1).copy_(_dev(link, dev).flatten())
        part(self.init, 3).copy_(torch.full((self.n,), SAD0, dtype=torch.int32, device=dev).view(torch.uint8))
        part(self.init, 4).zero_()
        part(self.init, 5).copy_(_dev(np.asarray(row, dtype=np.int64), dev).view(torch.uint8))
        self.merged = part(self.buf, 0).view(torch.int16).view(self.H, self.W, 2)
        self.link = part(self.buf, 1).view(self.H, self.W)
        self.dec = part(self.buf, 2).view(torch.int16).view(self.n, 8)
        self.sad = part(self.buf, 3).view(torch.int32)
        self.stats = part(self.buf, 4).view(torch.int64)
        self.row = part(self.buf, 5).view(torch.int64)

    def run(self, r, lam, intra, mask, mf, calls=1, sad=True, stats=True, row=True):
        """The oracle's tuple; after the calls every guard byte and both planes are as they were."""
        from arseg_amd import ops

        self.buf.copy_(self.init)
        for _ in range(calls):
            got = ops.mv_chain_heal(self.pc, self.pk, self.merged, self.link, self.B, r, lam, intra, mask, mf, decisions=self.dec, sad=self.sad if sad else False,
                                    stats=self.stats if stats else False, link_stats_row=self.row if row else None)
            assert got[0].data_ptr() == self.dec.data_ptr() and (got[1] is None) == (not sad) and (got[2] is None) == (not stats)
        host = self.buf.cpu().numpy()
        assert torch.equal(self.pc, self.keep[0]) and torch.equal(self.pk, self.keep[1])
        out = []
        for i, (s, dt) in enumerate(zip(self.sizes, (np.int16, np.uint8, np.int16, np.int32, np.int64, np.int64))):
            assert (host[self.off[i] + s:self.off[i + 1]] == GUARD).all(), i
            out.append(host[self.off[i]:self.off[i] + s].view(dt))
        s = out[3].astype(np.int64)
        return out[0].reshape(self.H, self.W, 2), out[1].reshape(self.H, self.W), out[2].reshape(self.n, 8), np.where(s == SAD0, -1, s), out[4], out[5]


@pytest.mark.parametrize("case", oracle.grid_cases(), ids=oracle.case_id)
def test_kernels_equal_the_loop_oracle(dev, case):
    """The grid of tests/test_mv_chain_heal.py: every r (a template instance each, with B), lam, intra, flag_mask and min_flagged."""
    cur, key, m, l, row = oracle.case(*case)
    bench = _Bench(dev, cur, key, m, l, row, case[3])
    for r, lam, intra, mask, mf in oracle.grid_params():
        want = oracle.outputs(oracle.winners_of(*case, r, lam, mask), m, l, case[3], intra, mask, mf, row)
        assert oracle.same(bench.run(r, lam, intra, mask, mf), want), (r, lam, intra, mask, mf)


@pytest.mark.parametrize("name", sorted(oracle.hand_cases()) + ["bound", "bound + 1"])
def test_hand_built_cases_equal_the_loops(dev, name):
    c = oracle.bound_case(name == "bound + 1") if name.startswith("bound") else oracle.hand_cases()[name]
    row = oracle.recount(c["link"]) + 7
    bench = _Bench(dev, c["cur"], c["key"], c["merged"], c["link"], row, c["B"])
    got = bench.run(c["r"], c["lam"], c["intra"], c["mask"], c["min_flagged"])
    assert oracle.same(got, oracle.run_case(oracle.heal, c, row))
    if name.startswith("bound"):
        assert got[2][0, 6] == (name == "bound + 1") and got[3][0] == 30 + (name == "bound + 1")


@pytest.mark.parametrize("B,r", [(16, 2), (8, 3), (16, 1)])
def test_100x150_against_the_numpy_form_stats_accumulate_outputs_optional(dev, B, r):
    """7 x 10 or 13 x 19 blocks: several waves and, at B = 8, several workgroups; clipped blocks on both edges."""
    from arseg_amd import ingest, ops

    cur, key, m, l, row = oracle.tiles_case(B=B)
    want = ingest.mv_chain_heal_numpy(cur, key, m, l, B, r, 2, 20, 3, 1, row)
    assert 0 < want[4][1] < want[4][0] and want[4][5] > 0 and (want[2][:, 6] == 2).any()
    bench = _Bench(dev, cur, key, m, l, row, B)
    assert oracle.same(bench.run(r, 2, 20, 3, 1), want)
    again = ingest.mv_chain_heal_numpy(cur, key, want[0], want[1], B, r, 2, 20, 3, 1, want[5])        # the second call sees the first one's planes
    got = bench.run(r, 2, 20, 3, 1, calls=2)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2])
    assert np.array_equal(got[4], want[4] + again[4]) and np.array_equal(got[5], again[5]) and np.array_equal(got[5], oracle.recount(got[1]))
    bare = bench.run(r, 2, 20, 3, 1, sad=False, stats=False, row=False)                                 # NULL sad, stats and link_stats_row
    assert oracle.same(bare[:3], want[:3]) and (bare[3] == -1).all() and not bare[4].any() and np.array_equal(bare[5], row)
    md, ld = _dev(m, dev), _dev(l, dev)
    dec, sad, st = ops.mv_chain_heal(bench.pc, bench.pk, md, ld, B, r, 2, 20, 3, 1)                      # everything allocated: sad and stats from zero
    assert np.array_equal(dec.cpu().numpy(), want[2]) and np.array_equal(st.cpu().numpy(), want[4]) and np.array_equal(md.cpu().numpy(), want[0])
    assert np.array_equal(sad.cpu().numpy().astype(np.int64), np.where(want[3] < 0, 0, want[3])) and np.array_equal(ld.cpu().numpy(), want[1])


def test_360x480_against_the_numpy_form(dev):
    from arseg_amd import ingest

    cur, key, m, l, row = oracle.tiles_case(360, 480, 16, oracle.SEED + 33)
    want = ingest.mv_chain_heal_numpy(cur, key, m, l, 16, 2, 2, 24, 3, 1, row)
    assert want[2].shape == (23 * 30, 8) and 100 < want[4][1] < want[4][0] < 23 * 30
    assert oracle.same(_Bench(dev, cur, key, m, l, row, 16).run(2, 2, 24, 3, 1), want)


def test_768x768_blocks_of_8_walk_the_grid_stride(dev):
    """9,216 blocks, above 16 waves x 2 workgroups x 256 compute units: some waves take a second block.  About 5 % of the blocks carry flags."""
    from arseg_amd import ingest

    cur, key, m, l, row = oracle.tiles_case(768, 768, 8, oracle.SEED + 34, share=0.05)
    want = ingest.mv_chain_heal_numpy(cur, key, m, l, 8, 2, 2, 20, 3, 8, row)
    assert want[2].shape == (9216, 8) and 300 < want[4][0] < 700 and want[4][1] > 100 and want[4][4] > 0
    assert oracle.same(_Bench(dev, cur, key, m, l, row, 8).run(2, 2, 20, 3, 8), want)


def test_pitched_planes_and_level_0_of_a_pyramid(dev):
    """The planes as columns of wider buffers (a pitch above the row, a base 4 bytes in; W = 53 leaves three bytes of the last dword to the
    neighbour) and as level 0 of a LumaPyramid."""
    from arseg_amd import ingest

    case = ("noise", 37, 53, 8, "rects")
    cur, key, m, l, row = oracle.case(*case)
    want = oracle.outputs(oracle.winners_of(*case, 2, 3, 3), m, l, 8, 20, 3, 1, row)
    wide = []
    for p, pad, fill in ((cur, 64, 171), (key, 72, 33)):
        wbuf = np.full((37, pad), fill, np.uint8)
        wbuf[:, 4:4 + 53] = p
        wide.append(_dev(wbuf, dev))
    views = tuple(t[:, 4:4 + 53] for t in wide)
    assert not views[0].is_contiguous() and views[0].data_ptr() % 4 == 0 and views[1].stride(0) == 72
    assert oracle.same(_Bench(dev, cur, key, m, l, row, 8, planes=views).run(2, 3, 20, 3, 1), want)
    grey = lambda p: ingest.DecodedFrames.rgb8(_dev(np.repeat(p[..., None], 3, axis=2), dev))            # luma8 of (v, v, v) is v
    pyr = [ingest.LumaPyramid(37, 53, 1, dev).build(grey(p)) for p in (cur, key)]
    assert oracle.same(_Bench(dev, cur, key, m, l, row, 8, planes=(pyr[0].level(0), pyr[1].level(0))).run(2, 3, 20, 3, 1), want)


# ---- end to end ----
def _frames(planes, dev):
    from arseg_amd import ingest

    H, W = planes[0].shape
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(_dev(p, dev), uv) for p in planes]


def _healer(dev, H, W, **kw):
    from arseg_amd import ingest

    cap = oracle.CAP
    return ingest.ChainHealer(H, W, block=cap["B"], refine=cap["r"], lam=cap["lam"], intra=cap["intra"], flags=cap["mask"], min_flagged=cap["min_flagged"],
                              device=dev, **kw)


def _host(pushes, frames, gop, max_ref, bidirectional=False):
    from arseg_amd import ingest

    return oracle.run_chain(pushes, frames, gop, max_ref, oracle.cap_heal(ingest.mv_chain_heal_numpy), bidirectional)


@pytest.mark.parametrize("source", ["records", "estimator"])
def test_scene_1_through_chain_and_healer(dev, source):
    """The panned GOP with an occluder in frame 2 as plain hop records (uploaded, or estimated on the device) through MotionChain + ChainHealer:
    merged, link bytes, link counts and heal counts equal the host chain over the host form, and the capability holds on the device's output."""
    from arseg_amd import ingest

    planes, pushes = bma.gop_frames(), list(oracle.scene1_pushes())
    H, W = planes[0].shape
    merged, link, stats, rows = _host(pushes, planes, bma.GOP, oracle.CAP["max_ref"])
    frames = _frames(planes, dev)
    chain = ingest.MotionChain(H, W, gop=bma.GOP, max_ref=oracle.CAP["max_ref"], device=dev, track_links=True)
    healer = _healer(dev, H, W, with_sad=True)
    est = ingest.MotionEstimator(H, W, block=oracle.CAP["B"], search=oracle.CAP["R"], lam=oracle.CAP["lam"], intra=oracle.CAP["intra"], device=dev)
    healer.set_key(frames[0])
    total = np.zeros(oracle.NSTATS, np.int64)
    for f, rec in pushes:
        chain.push(est.estimate(frames[f], frames[f - 1]) if source == "estimator" else _dev(rec, dev))
        out = healer.heal(chain, frames[f])
        assert out.data_ptr() == chain.merged[f].data_ptr()
        total += stats[f]
        assert np.array_equal(healer.heal_stats_row().cpu().numpy(), total), f
    assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
    got = chain.link_stats().cpu().numpy()
    assert all(np.array_equal(got[f], rows[f]) and np.array_equal(got[f], oracle.recount(link[f])) for f in range(1, bma.GOP))
    lk, mv = chain.link().cpu().numpy(), chain.mv_q().cpu().numpy()
    for f in (3, 4, 5):
        leaves = oracle.leaves_frame(f, H, W)
        assert np.array_equal(lk[f] & 7 != 0, leaves) and oracle.off_truth(mv[f], f, ~leaves) == 0
    healer.reset_stats()
    assert not healer.heal_stats_row().any()


def test_scene_2_bidirectional_chain_of_20_frames(dev):
    """Off-grid decoder records with intra units, a B-frame in decode order, frames beyond 16: bit-equal to the host chain over the host form."""
    from arseg_amd import ingest

    planes, pushes = oracle.scene2_frames(), list(oracle.scene2_pushes())
    H, W = planes[0].shape
    merged, link, stats, rows = _host(pushes, planes, oracle.GOP2, oracle.MAX_REF2, True)
    frames = _frames(planes, dev)
    chain = ingest.MotionChain(H, W, gop=oracle.GOP2, max_ref=oracle.MAX_REF2, device=dev, bidirectional=True, track_links=True)
    healer = _healer(dev, H, W)
    healer.set_key(frames[0])
    for f, rec in pushes:
        chain.push(_dev(rec, dev), at=f)
        healer.heal(chain, frames[f])                                  # at = None: the frame just pushed
    assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
    got = chain.link_stats().cpu().numpy()
    assert all(np.array_equal(got[f], rows[f]) for f in range(1, oracle.GOP2))
    assert np.array_equal(healer.heal_stats_row().cpu().numpy(), sum(stats[f] for f in range(1, oracle.GOP2)))
    for f in (17, 18, 19):
        stays = ~oracle.leaves_frame(f, H, W)
        assert not ((link[f] & 7 != 0) & stays).any() and oracle.off_truth(merged[f], f, stays) == 0 and stats[f][1] > 0


def test_graph_replays_push_and_heal_on_new_frames_and_records(dev):
    """Frame 3 of scene 1: the chain holds the healed frames 1 and 2; push + heal for f = 3 in one torch.cuda.graph over a static record buffer
    and a static frame, replayed on other records and frames (the chain is wound back to f = 2 on the host: push and heal are launches only)."""
    from arseg_amd import ingest

    planes, pushes = bma.gop_frames(), list(oracle.scene1_pushes())
    H, W = planes[0].shape
    frames = _frames(planes, dev)
    cur = _frames([np.zeros_like(planes[0])], dev)[0]
    records = torch.zeros_like(_dev(pushes[0][1], dev))
    chain = ingest.MotionChain(H, W, gop=bma.GOP, max_ref=oracle.CAP["max_ref"], device=dev, track_links=True)
    healer = _healer(dev, H, W)
    healer.set_key(frames[0])
    for f in (1, 2):
        chain.push(_dev(pushes[f - 1][1], dev))
        healer.heal(chain, frames[f])

    def step():
        chain.f = chain.last = 2
        chain.link_counts[3].zero_()
        healer.reset_stats()
        chain.push(records)
        return healer.heal(chain, cur)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for k in (3, 4, 2, 3):
        records.copy_(_dev(pushes[k - 1][1], dev))
        cur.planes[0].copy_(_dev(planes[k], dev)[None])
        graph.replay()
        torch.cuda.synchronize()
        replayed = (out.clone(), chain.link_bytes[3].clone(), chain.link_counts[3].clone(), healer.heal_stats_row().clone(), healer.decisions.clone())
        merged, link, stats, rows = _host(pushes[:2] + [(3, pushes[k - 1][1])], planes[:3] + (planes[k],), bma.GOP, oracle.CAP["max_ref"])
        assert np.array_equal(replayed[0].cpu().numpy(), merged[3]) and np.array_equal(replayed[1].cpu().numpy(), link[3])
        assert np.array_equal(replayed[2].cpu().numpy(), rows[3]) and np.array_equal(replayed[3].cpu().numpy(), stats[3])
        eager = step()
        torch.cuda.synchronize()
        assert torch.equal(eager, replayed[0]) and torch.equal(chain.link_bytes[3], replayed[1]) and torch.equal(chain.link_counts[3], replayed[2])
        assert torch.equal(healer.heal_stats_row(), replayed[3]) and torch.equal(healer.decisions, replayed[4])


def test_a_chain_never_healed_is_as_it_was(dev):
    from arseg_amd import ingest

    planes, pushes = bma.gop_frames(), list(oracle.scene1_pushes())
    H, W = planes[0].shape
    merged, link, _, _ = oracle.run_chain(pushes, planes, bma.GOP, oracle.CAP["max_ref"])
    chain = ingest.MotionChain(H, W, gop=bma.GOP, max_ref=oracle.CAP["max_ref"], device=dev, track_links=True)
    healer = _healer(dev, H, W)
    healer.set_key(_frames(planes[:1], dev)[0])                         # a healer that is never asked to heal changes nothing
    for f, rec in pushes:
        chain.push(_dev(rec, dev))
        assert chain.last == chain.f == f
    assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(chain.link().cpu().numpy(), link)
    got = chain.link_stats().cpu().numpy()
    assert all(np.array_equal(got[f], oracle.recount(link[f])) for f in range(1, bma.GOP))
    assert not healer.heal_stats_row().any() and not healer.decisions.any()


def test_wrappers_refuse(dev):
    from arseg_amd import _lib, ingest, ops

    case = ("noise", 37, 53, 16, "rects")
    cur, key, m, l, row = oracle.case(*case)
    H, W = 37, 53
    cur, key, m, l, row = _plane(cur, dev), _plane(key, dev), _dev(m, dev), _dev(l, dev), _dev(row, dev)
    ok = dict(B=16, r=2, lam=2, intra=20, flag_mask=3, min_flagged=1)
    for kw in (dict(B=12), dict(r=0), dict(r=4), dict(lam=256), dict(intra=-1), dict(flag_mask=0), dict(flag_mask=8), dict(min_flagged=0), dict(min_flagged=65)):
        with pytest.raises(_lib.ArsegError):
            ops.mv_chain_heal(cur, key, m, l, **dict(ok, **kw))
    wide = torch.zeros((H, 64), dtype=torch.uint8, device=dev)
    bad = [lambda: ops.mv_chain_heal(wide[:, 1:1 + W], key, m, l, **ok),                                      # base not 4-byte aligned
           lambda: ops.mv_chain_heal(cur, torch.zeros((H, W + 1), dtype=torch.uint8, device=dev)[:, :W], m, l, **ok),      # pitch 54
           lambda: ops.mv_chain_heal(cur, key[:-1], m, l, **ok),
           lambda: ops.mv_chain_heal(cur.cpu(), key, m, l, **ok),
           lambda: ops.mv_chain_heal(cur, key, m[..., :1], l, **ok),
           lambda: ops.mv_chain_heal(cur, key, m.to(torch.int32), l, **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l[:, :-1], **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l.to(torch.int16), **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l, decisions=torch.zeros((11, 8), dtype=torch.int16, device=dev), **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l, sad=torch.zeros(11, dtype=torch.int32, device=dev), **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l, stats=torch.zeros(4, dtype=torch.int64, device=dev), **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l, link_stats_row=row[:-1], **ok),
           lambda: ops.mv_chain_heal(cur, key, m, l, link_stats_row=row.to(torch.int32), **ok)]
    for fn in bad:
        with pytest.raises(_lib.ArsegError):
            fn()
    assert torch.equal(m, _dev(oracle.case(*case)[2], dev)) and torch.equal(l, _dev(oracle.case(*case)[3], dev))      # a refused call touches nothing
    # the healer
    planes = bma.gop_frames()
    H, W = planes[0].shape
    frames = _frames(planes[:3], dev)
    for kw in (dict(block=12), dict(refine=0), dict(refine=4), dict(lam=256), dict(intra=256), dict(flags=0), dict(flags=8), dict(min_flagged=0), dict(min_flagged=65)):
        with pytest.raises(_lib.ArsegError):
            ingest.ChainHealer(H, W, device=dev, **kw)
    with pytest.raises(_lib.ArsegError):
        ingest.ChainHealer(H, W, device="cpu")
    healer = ingest.ChainHealer(H, W, device=dev)
    chain = ingest.MotionChain(H, W, gop=4, max_ref=16, device=dev, track_links=True)
    chain.push(_dev(oracle.scene1_pushes()[0][1], dev))
    with pytest.raises(_lib.ArsegError, match="set_key"):                                                   # before set_key
        healer.heal(chain, frames[1])
    rgb = ingest.DecodedFrames.rgb8(torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.ArsegError, match="levels >= 1"):                                               # the estimator's rule, the estimator's words
        healer.set_key(rgb)
    odd = torch.zeros((1, H, W + 4), dtype=torch.uint8, device=dev)[:, :, 1:1 + W]
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.ArsegError, match="levels >= 1"):
        healer.set_key(ingest.DecodedFrames.nv12(odd, uv))
    with pytest.raises(_lib.ArsegError):
        healer.set_key(ingest.LumaPyramid(H + 2, W, 1, dev))
    healer.set_key(ingest.LumaPyramid(H, W, 2, dev).build(frames[0]))
    healer.set_key(frames[0])
    healer.heal(chain, frames[1])
    healer.heal(chain, ingest.LumaPyramid(H, W, 1, dev).build(frames[1]), at=1)
    for bad_chain in (ingest.MotionChain(H, W, gop=4, max_ref=16, device=dev), ingest.MotionChain(H + 16, W, gop=4, max_ref=16, device=dev, track_links=True)):
        with pytest.raises(_lib.ArsegError):
            healer.heal(bad_chain, frames[1])
    for at in (0, 2, 4, -1):                                                                                # the keyframe, a frame not pushed, outside the GOP
        with pytest.raises(_lib.ArsegError):
            healer.heal(chain, frames[1], at=at)
    with pytest.raises(_lib.ArsegError):
        healer.heal(ingest.MotionChain(H, W, gop=4, max_ref=16, device=dev, track_links=True), frames[1])   # nothing pushed yet
    with pytest.raises(_lib.ArsegError):
        healer.heal(chain, rgb)
    bi = ingest.MotionChain(H, W, gop=6, max_ref=3, device=dev, bidirectional=True, track_links=True)
    bi.push(_dev(oracle.scene1_pushes()[0][1], dev), at=2)
    with pytest.raises(_lib.ArsegError):
        healer.heal(bi, frames[1], at=1)
    healer.heal(bi, frames[2])


def test_c_abi_refuses_bad_arguments(dev):
    from arseg_amd import _lib

    lib = _lib.load()
    for name, args, want in oracle.abi_cases():
        assert lib.arseg_mv_chain_heal_fwd(*args) == want, name
