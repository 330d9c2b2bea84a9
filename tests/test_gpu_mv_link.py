"""GPU checks of the link bytes along the motion chain (csrc/mv_records.hip: arseg_mv_link_reset, arseg_mv_records_step_link_fwd,
arseg_mv_records_bi_step_link_fwd; ingest.MotionChain(track_links=True)) and of the consistency form they gate (csrc/consistency.hip:
arseg_labels_consistency_linked_fwd) against the plain-Python oracles of tests/mv_link_oracle.py.  Integers in, integers out: every comparison
is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import consistency_oracle as tc_oracle
import mv_link_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0x5a
ORDER_IDS = ["".join(map(str, o)) for o in oracle.ORDERS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _dev(rec, dev):
    return torch.from_numpy(np.ascontiguousarray(rec, dtype=np.int16)).to(dev)


def _run(dev, pushes, H, W, gop, max_ref, policy, bi=True, with_stats=True):
    """reset + one link step per push on buffers with guard bytes behind link, guard words behind link_stats, merged and the index map(s).
    After every step: the maps all -1, every guard and the records as they were, merged[f] torch.equal to the plain entry's on the same
    records.  Returns (merged, link, link_stats) as numpy; all three are zeroed beforehand, so frames never pushed read 0."""
    from arseg_amd import _lib, ops

    hw, maps_n, NS = H * W, 2 if bi else 1, _lib.LINK_NSTATS
    mbuf = torch.zeros(gop * hw * 2 + 16, dtype=torch.int16, device=dev)
    mbuf[gop * hw * 2:] = 0x5a5a
    wbuf = torch.full((maps_n * hw + 8,), 0x5a5a, dtype=torch.int32, device=dev)
    lbuf = torch.full((gop * hw + 16,), GUARD, dtype=torch.uint8, device=dev)
    sbuf = torch.full((gop * NS + 4,), GUARD, dtype=torch.int64, device=dev)
    merged, maps = mbuf[:gop * hw * 2].view(gop, H, W, 2), wbuf[:maps_n * hw]
    link, st = lbuf[:gop * hw].view(gop, H, W), sbuf[:gop * NS].view(gop, NS)
    link[1:] = 0
    plain, pmaps = torch.zeros_like(merged), torch.empty_like(maps)
    (ops.mv_records_bi_reset if bi else ops.mv_records_reset)(merged, maps)
    (ops.mv_records_bi_reset if bi else ops.mv_records_reset)(plain, pmaps)
    ops.mv_link_reset(link, st if with_stats else None)
    assert not bool(link[0].any()) and (not with_stats or not bool(st.any()))
    done = 1
    for f, rec in pushes:
        r = _dev(rec, dev)
        if bi:
            out, lk = ops.mv_records_bi_step_link(r, merged, f, done, maps, link, st if with_stats else None, max_ref, policy)
            ops.mv_records_bi_step(r, plain, f, done, pmaps, max_ref, policy)
        else:
            out, lk = ops.mv_records_step_link(r, merged, f, maps, link, st if with_stats else None, max_ref)
            ops.mv_records_step(r, plain, f, pmaps, max_ref)
        done |= 1 << f
        assert out.data_ptr() == merged[f].data_ptr() and lk.data_ptr() == link[f].data_ptr() and lk.shape == (H, W)
        assert torch.equal(merged[f], plain[f])
        assert bool((maps == -1).all())
        assert bool((mbuf[gop * hw * 2:] == 0x5a5a).all()) and bool((wbuf[maps_n * hw:] == 0x5a5a).all())
        assert bool((lbuf[gop * hw:] == GUARD).all()) and bool((sbuf[gop * NS:] == GUARD).all())
        assert np.array_equal(r.cpu().numpy(), rec)
    return merged.cpu().numpy(), link.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("case", oracle.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(dev, case):
    _, max_ref, gop, pushes, expected = case
    for policy in oracle.POLICIES:
        want = oracle.hand_expected(expected[policy], gop)
        _, link, st = _run(dev, pushes, 8, 8, gop, max_ref, policy)
        assert np.array_equal(link, want), policy
        assert np.array_equal(st, oracle.stats(want) * (np.arange(gop) > 0)[:, None])          # row 0 is never added to
    if oracle.is_p_case(pushes):
        want = oracle.hand_expected(expected["list0"], gop)
        _, link, st = _run(dev, pushes, 8, 8, gop, max_ref, None, bi=False)
        assert np.array_equal(link, want) and np.array_equal(st[1:], oracle.stats(want)[1:]) and not st[0].any()


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("order", oracle.ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("H,W", oracle.SHAPES)
def test_generated_gops_bi_entry(dev, H, W, order, max_ref):
    """37x53 (H W odd) takes the per-pixel kernel, 8x8 and 24x40 the four-pixel one."""
    from arseg_amd import ingest

    for policy in oracle.POLICIES:
        pushes, want = oracle.generated(H, W, order, max_ref, policy)
        merged, link, st = _run(dev, pushes, H, W, oracle.GOP, max_ref, policy)
        assert np.array_equal(link, want), policy
        assert np.array_equal(st[1:], oracle.stats(want)[1:]) and not st[0].any()
        assert np.array_equal(merged, ingest.chain_records_numpy(pushes, H, W, oracle.GOP, max_ref, policy))
    _, link, st = _run(dev, pushes, H, W, oracle.GOP, max_ref, "mean", with_stats=False)           # link_stats = NULL
    assert np.array_equal(link, want) and bool((st == GUARD).all())


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("H,W", oracle.SHAPES)
def test_generated_gops_p_entry_and_bi_in_order(dev, H, W, max_ref):
    pushes, _ = oracle.generated(H, W, oracle.ORDERS[0], max_ref, "list0", False)
    want = oracle.chain_p([r for _, r in pushes], H, W, oracle.GOP, max_ref)
    merged, link, st = _run(dev, pushes, H, W, oracle.GOP, max_ref, None, bi=False)
    assert np.array_equal(link, want) and np.array_equal(st[1:], oracle.stats(want)[1:]) and not st[0].any()
    for policy in oracle.POLICIES:                                     # every record in list 0, in order: the bi entry's bytes are the P entry's
        m2, l2, s2 = _run(dev, pushes, H, W, oracle.GOP, max_ref, policy)
        assert np.array_equal(l2, link) and np.array_equal(s2, st) and np.array_equal(m2, merged), policy
    _, link, st = _run(dev, pushes, H, W, oracle.GOP, max_ref, None, bi=False, with_stats=False)
    assert np.array_equal(link, want) and bool((st == GUARD).all())


def test_across_the_scatter_band(dev):
    """One GOP of four frames at 300x200: two scatter bands, a frame-sized record first in every frame."""
    pushes, want = oracle.generated_banded(3)
    H, W = oracle.BANDED
    merged, link, st = _run(dev, pushes, H, W, 4, 3, None, bi=False)
    assert np.array_equal(link, want) and np.array_equal(st[1:], oracle.stats(want)[1:])
    _, l2, s2 = _run(dev, pushes, H, W, 4, 3, "near")
    assert np.array_equal(l2, want) and np.array_equal(s2, st)


def test_two_pushes_of_one_frame_count_twice(dev):
    """link_stats is accumulated into: the same frame stepped twice into a fresh row leaves twice its counts (and the same bytes)."""
    from arseg_amd import ops

    H, W = 24, 40
    pushes, want = oracle.generated(H, W, oracle.ORDERS[0], 3, "list0", False)
    merged = torch.zeros((oracle.GOP, H, W, 2), dtype=torch.int16, device=dev)
    maps = torch.empty(H * W, dtype=torch.int32, device=dev)
    link = torch.zeros((oracle.GOP, H, W), dtype=torch.uint8, device=dev)
    st = torch.ones((oracle.GOP, 20), dtype=torch.int64, device=dev)
    ops.mv_records_reset(merged, maps)
    ops.mv_link_reset(link, st)
    r = _dev(pushes[0][1], dev)
    for _ in range(2):
        ops.mv_records_step_link(r, merged, 1, maps, link, st)
    row = np.array(oracle.stats_row(want[1]), dtype=np.int64)
    assert np.array_equal(st[1].cpu().numpy(), 2 * row) and np.array_equal(link[1].cpu().numpy(), want[1]) and not bool(st[2:].any())


@pytest.mark.parametrize("bi", [False, True], ids=["p", "bi"])
def test_motion_chain_two_gops_padded_and_host_records(dev, bi):
    """Two GOPs through one MotionChain(track_links=True) with reset() between them; padded device buffers and host records give the same."""
    from arseg_amd import ingest

    H, W, max_ref = 37, 53, 3
    order = oracle.ORDERS[1] if bi else oracle.ORDERS[0]
    a, want_a = oracle.generated(H, W, order, max_ref, "near", bi)
    b = oracle.make_gop(oracle.SEED + 1, H, W, order, max_ref, bi)
    want_b = oracle.chain(b, H, W, oracle.GOP, max_ref, "near")
    assert not np.array_equal(want_a, want_b)
    chain = ingest.MotionChain(H, W, gop=oracle.GOP, max_ref=max_ref, device=dev, bidirectional=bi, bipred="near", track_links=True)
    assert chain.link_bytes.shape == (oracle.GOP, H, W) and chain.link_stats().shape == (oracle.GOP, 20)
    cap = max(r.shape[0] for _, r in a + b) + 7
    for pushes, want, padded in ((a, want_a, True), (b, want_b, False), (a, want_a, False)):
        chain.reset()
        assert not bool(chain.link_stats().any()) and tuple(chain.link().shape) == (1, H, W)
        for f, r in pushes:
            chain.push(_dev(ingest.pad_records(r, cap), dev) if padded else r, at=f if bi else None)
        assert tuple(chain.link().shape) == (oracle.GOP, H, W) and chain.link().data_ptr() == chain.link_bytes.data_ptr()
        assert np.array_equal(chain.link().cpu().numpy(), want)
        assert np.array_equal(chain.link_stats().cpu().numpy()[1:], oracle.stats(want)[1:])
        assert np.array_equal(ingest.link_hops(chain.link()).cpu().numpy(), want >> 4)
        merged, link = ingest.chain_records_numpy(pushes, H, W, oracle.GOP, max_ref, "near", return_link=True)
        assert np.array_equal(chain.mv_q().cpu().numpy(), merged) and np.array_equal(link, want)
    mon = ingest.LinkMonitor(0.3, mask=7)
    rows = chain.link_stats().cpu().numpy()
    assert [mon.update(rows[f], H * W) for f in range(1, oracle.GOP)] == [bool(((want_a[f] & 7) != 0).sum() > 0.3 * H * W) for f in range(1, oracle.GOP)]
    if bi:                                                               # link() follows mv_q()'s prefix rule
        chain.reset()
        chain.push(a[0][1], at=a[0][0])                                  # frame 3 first: not a prefix
        with pytest.raises(Exception):
            chain.link()


def test_track_links_false_allocates_nothing_and_is_the_plain_chain(dev):
    from arseg_amd import _lib, ingest

    H, W = 24, 40
    pushes, _ = oracle.generated(H, W, oracle.ORDERS[0], 3, "list0", False)
    plain = ingest.MotionChain(H, W, gop=oracle.GOP, device=dev)
    assert plain.track_links is False and plain.link_bytes is None and plain.link_counts is None
    with pytest.raises(_lib.ArsegError):
        plain.link()
    with pytest.raises(_lib.ArsegError):
        plain.link_stats()
    linked = ingest.MotionChain(H, W, gop=oracle.GOP, device=dev, track_links=True)
    recs = [_dev(r, dev) for _, r in pushes]
    assert torch.equal(plain.push_gop(recs), linked.push_gop(recs))


def test_graph_replays_reset_and_pushes_on_refilled_records(dev):
    """reset + seven pushes of a track_links chain over static padded record buffers in one torch.cuda.graph; the buffers are refilled in
    place with a GOP of another fill level and the graph replayed: bytes and counts are those of the records in the buffers."""
    from arseg_amd import ingest

    H, W, max_ref = 24, 40, 3
    a, want_a = oracle.generated(H, W, oracle.ORDERS[0], max_ref, "list0", False)
    b = [(f, r[: r.shape[0] // 2]) for f, r in oracle.make_gop(oracle.SEED + 2, H, W, oracle.ORDERS[0], max_ref, False)]          # half the records: more holes
    want_b = oracle.chain_p([r for _, r in b], H, W, oracle.GOP, max_ref)
    assert not np.array_equal(want_a, want_b) and (want_b[-1] & oracle.UNCOVERED).sum() > (want_a[-1] & oracle.UNCOVERED).sum()
    cap = max(r.shape[0] for _, r in a + b) + 5
    static = [_dev(ingest.pad_records(r, cap), dev) for _, r in a]
    chain = ingest.MotionChain(H, W, gop=oracle.GOP, max_ref=max_ref, device=dev, track_links=True)

    def step():
        chain.reset()
        for s in static:
            chain.push(s)
        return chain.link()

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for gop_, want in ((a, want_a), (b, want_b), (a, want_a)):
        for s, (_, r) in zip(static, gop_):
            s.copy_(_dev(ingest.pad_records(r, cap), dev))
        chain.link_bytes.fill_(GUARD)
        chain.link_counts.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert out.data_ptr() == chain.link_bytes.data_ptr() and np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(chain.link_stats().cpu().numpy()[1:], oracle.stats(want)[1:]) and not bool(chain.link_stats()[0].any())


# ---- the consistency form the bytes gate ----
@pytest.fixture(scope="module")
def tc(dev):
    """consistency_oracle's 2 x 12 x 24 x 40 case with the link planes of frames 6 and 7 of a generated GOP of that size."""
    case = tc_oracle.CASES[0]
    assert case[2:4] == (2, 12) and case[6:8] == (24, 40)
    b = tc_oracle.build(case)
    link = oracle.generated(24, 40, oracle.ORDERS[1], 3, "mean")[1][6:8].copy()
    labels = b["labels"].astype(np.uint8)
    labels[0, 3:6, 10:20] = 255                                          # void source labels
    return {"labels": labels, "ref": b["ref"], "mv": b["mv"], "link": link, "n_cls": 12,
            "t": {k: torch.from_numpy(v).to(dev) for k, v in (("labels", labels), ("ref", b["ref"]), ("mv", b["mv"]), ("link", link))}}


@pytest.mark.parametrize("mask", [0, 1, 2, 4, 3, 7, 0x30, 0xff])
def test_linked_consistency_against_the_oracle(dev, tc, mask):
    from arseg_amd import _lib, ops

    t, N, H, W = tc["t"], 2, 24, 40
    change = torch.full((N, H, W), 77, dtype=torch.uint8, device=dev)
    st = torch.zeros((N, _lib.TC_NSTATS), dtype=torch.int64, device=dev)
    unl = torch.zeros(N, dtype=torch.int64, device=dev)
    ops.labels_consistency_linked(t["labels"], t["ref"], t["mv"], 12, t["link"], mask, change_out=change, stats=st, unlinked=unl)
    want_c, want_s, want_u = oracle.consistency_linked(tc["labels"], tc["ref"], tc["mv"], 12, tc["link"], mask)
    assert np.array_equal(change.cpu().numpy(), want_c) and np.array_equal(st.cpu().numpy(), want_s) and np.array_equal(unl.cpu().numpy(), want_u)
    assert ((st[:, :3].sum(dim=1) + unl) == H * W).all()                 # compared + outside + void + unlinked = H W
    assert np.array_equal(want_u, ((tc["link"] & mask) != 0).sum(axis=(1, 2)))
    if mask in (1, 2, 4):
        assert 0 < want_u.min() and want_u.max() < H * W                 # each single bit gates some pixels and not all
    if mask == 0:                                                        # the plain form, bit for bit
        c0 = torch.full_like(change, 77)
        s0 = torch.zeros_like(st)
        ops.labels_consistency(t["labels"], t["ref"], t["mv"], 12, change_out=c0, stats=s0)
        assert torch.equal(change, c0) and torch.equal(st, s0) and not bool(unl.any())
    if mask == 0xff:                                                     # every pixel of frames 6 and 7 has hops: all unlinked
        assert bool((change == 128).all()) and not bool(st.any()) and unl.tolist() == [H * W, H * W]
    ops.labels_consistency_linked(t["labels"], t["ref"], t["mv"], 12, t["link"], mask, stats=st, unlinked=unl)          # accumulated into; no plane
    assert np.array_equal(st.cpu().numpy(), 2 * want_s) and np.array_equal(unl.cpu().numpy(), 2 * want_u)
    c2 = torch.full_like(change, 77)
    ops.labels_consistency_linked(t["labels"], t["ref"], t["mv"], 12, t["link"], mask, change_out=c2)                   # unlinked = NULL, stats = NULL
    assert torch.equal(c2, change)


def test_linked_consistency_pitched_link_plane_and_a_frame_slice(dev, tc):
    """The link plane as rows of a wider buffer (guard bytes between the rows) and as frames [1:3] of a four-frame tensor; through
    egress.consistency_of_planes, which allocates the outputs."""
    from arseg_amd import egress

    t, N, H, W = tc["t"], 2, 24, 40
    wide = torch.full((4, H, W + 13), GUARD | 7, dtype=torch.uint8, device=dev)
    wide[1:3, :, :W] = t["link"]
    view = wide[1:3, :, :W]
    assert not view.is_contiguous()
    want_c, want_s, want_u = oracle.consistency_linked(tc["labels"], tc["ref"], tc["mv"], 12, tc["link"], 3)
    change, st, unl = egress.consistency_of_planes(t["labels"], t["ref"], t["mv"], 12, change_out=True, link=view, unlinked=True)
    assert np.array_equal(change.cpu().numpy(), want_c) and np.array_equal(st.cpu().numpy(), want_s) and np.array_equal(unl.cpu().numpy(), want_u)
    assert bool((wide[:, :, W:] == (GUARD | 7)).all()) and bool((wide[0] == (GUARD | 7)).all())
    plain = egress.consistency_of_planes(t["labels"], t["ref"], t["mv"], 12, change_out=True)          # link=None: today's path, two results
    assert len(plain) == 2
    c0, s0, u0 = egress.consistency_of_planes(t["labels"], t["ref"], t["mv"], 12, change_out=True, link=view, link_mask=0, unlinked=True)
    assert torch.equal(c0, plain[0]) and torch.equal(s0, plain[1]) and not bool(u0.any())
    table = egress.tc_table(st, 12)                                      # the stats layout is unchanged: the table and the monitor work as they are
    assert np.isfinite(table["agreement"]).all() and egress.ConsistencyMonitor(0.0, 0.0).update(st[0].cpu().numpy(), H * W) is False


def test_alter_res_batch_consistency_linked(dev, manifest):
    """The small PSPNet (fp32) fed by a track_links chain: the labels are alter_res_batch_consistency's, change8 / statistics / unlinked equal
    the oracle fed those labels and the chain's link planes; link_mask = 0 gives alter_res_batch_consistency's outputs."""
    import test_gpu_ingest_formats as tf
    from arseg_amd import egress, ingest, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop = 64, 96, 4
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    chain = ingest.MotionChain(H, W, gop=gop, device=dev, track_links=True)
    recs = synth.make_link_chain(31, H, W, gop - 1, intra=0.1, holes=0.1)
    mvs = chain.push_gop([_dev(r, dev) for r in recs])[1:]
    link = chain.link()[1:]
    assert np.array_equal(link.cpu().numpy(), oracle.chain_p(recs, H, W, gop, 3)[1:])
    with torch.no_grad():
        key_logits, feat_k = hr.forward_keyframe(frames[0:1])
        key_labels = egress.labels8(key_logits.float(), H, W)
        refs = [feat_k[0]] * (gop - 1)
        c0, l0, s0 = ev.alter_res_batch_consistency(lr, refs, frames[1:gop], mvs, key_labels, 0.5)
        change, labels, stats, unl = ev.alter_res_batch_consistency_linked(lr, refs, frames[1:gop], mvs, key_labels, 0.5, link=link)
        cz, lz, sz, uz = ev.alter_res_batch_consistency_linked(lr, refs, frames[1:gop], mvs, key_labels, 0.5, link=link, link_mask=0)
    n_cls = key_logits.shape[1]
    assert torch.equal(labels, l0) and torch.equal(lz, l0)
    assert torch.equal(cz, c0) and torch.equal(sz, s0) and not bool(uz.any())
    want_c, want_s, want_u = oracle.consistency_linked(labels.cpu().numpy(), key_labels.cpu().numpy(), mvs.cpu().numpy(), n_cls, link.cpu().numpy(), 3)
    assert np.array_equal(change.cpu().numpy(), want_c) and np.array_equal(stats.cpu().numpy(), want_s) and np.array_equal(unl.cpu().numpy(), want_u)
    assert 0 < int(unl.min()) and int(unl.max()) < H * W and ((stats[:, :3].sum(dim=1) + unl) == H * W).all()
    print(f"\nunlinked {unl.tolist()} of {H * W}; compared plain {s0[:, 0].tolist()} -> linked {stats[:, 0].tolist()}")
