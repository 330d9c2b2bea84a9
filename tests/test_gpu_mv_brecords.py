"""GPU checks of the two-list (B-frame) record chain (csrc/mv_records.hip, arseg_mv_records_bi_*; ingest.MotionChain(bidirectional=True))
against the plain-Python oracle (tests/mv_brecords_oracle.py): hand cases, generated GOPs in four decode orders under the three policies,
the P-frame equivalence, padded and host record buffers, a larger gop buffer, graph replay of one decode order, mv_q()'s prefix rule, and
the fast path fed from a B-frame chain.  Integers in, integers out: every comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import mv_brecords_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0x5a5a
ORDER_IDS = ["".join(map(str, o)) for o in oracle.ORDERS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _dev(rec, dev):
    return torch.from_numpy(np.ascontiguousarray(rec, dtype=np.int16)).to(dev)


def _run(dev, pushes, H, W, gop, max_ref, policy):
    """reset + one ops.mv_records_bi_step per push on buffers with guard words behind merged and behind the two index maps.  After every
    step: both maps all -1, the guards and the records as they were.  Returns merged (zeroed beforehand, so frames never pushed read 0)."""
    from arseg_amd import ops

    hw = H * W
    mbuf = torch.zeros(gop * hw * 2 + 16, dtype=torch.int16, device=dev)
    mbuf[gop * hw * 2:] = GUARD
    wbuf = torch.full((2 * hw + 8,), GUARD, dtype=torch.int32, device=dev)
    merged, maps = mbuf[:gop * hw * 2].view(gop, H, W, 2), wbuf[:2 * hw]
    ops.mv_records_bi_reset(merged, maps)
    assert bool((maps == -1).all()) and bool((merged[0] == -1).all()) and not bool(merged[1:].any())
    done = 1
    for f, rec in pushes:
        r = _dev(rec, dev)
        out = ops.mv_records_bi_step(r, merged, f, done, maps, max_ref, policy)
        done |= 1 << f
        assert out.data_ptr() == merged[f].data_ptr() and out.shape == (H, W, 2)
        assert bool((maps == -1).all())
        assert bool((mbuf[gop * hw * 2:] == GUARD).all()) and bool((wbuf[2 * hw:] == GUARD).all())
        assert np.array_equal(r.cpu().numpy(), rec)
    return merged.cpu().numpy()


@pytest.mark.parametrize("case", oracle.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(dev, case):
    _, max_ref, pushes, expected = case
    for policy in oracle.POLICIES:
        want = oracle.hand_expected(expected[policy])
        assert np.array_equal(oracle.chain(pushes, 8, 8, 4, max_ref, policy), want)
        assert np.array_equal(_run(dev, pushes, 8, 8, 4, max_ref, policy), want), policy


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("order", oracle.ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("H,W", [(24, 40), (37, 53), (8, 8)])
def test_generated_gops(dev, H, W, order, max_ref):
    """24x40: four pixels per lane; 37x53: H W % 4 != 0, one pixel per lane; 8x8: one block."""
    for policy in oracle.POLICIES:
        pushes, want, _ = oracle.generated(H, W, order, max_ref, policy)
        assert np.array_equal(_run(dev, pushes, H, W, oracle.GOP, max_ref, policy), want), policy


@pytest.mark.parametrize("policy", oracle.POLICIES)
@pytest.mark.parametrize("order", oracle.ORDERS, ids=ORDER_IDS)
def test_generated_gops_across_the_scatter_band(dev, order, policy):
    """300x200: two scatter bands, a frame-sized record in each list under the blocks; the whole GOP in every decode order under every policy."""
    H, W = oracle.BANDED
    pushes, want, st = oracle.generated(H, W, order, 3, policy)
    assert len(pushes) == oracle.GOP - 1 and st["both"] > 0 and st["only_list1"] > 0 and st["neither_under_winner"] > 0
    assert np.array_equal(_run(dev, pushes, H, W, oracle.GOP, 3, policy), want)


@pytest.mark.parametrize("H,W,F_", [(37, 53, 11), (64, 96, 3)])
def test_p_only_records_in_order_equal_the_p_frame_chain(dev, H, W, F_):
    """The anchor: P-only records pushed in order through the two-list entry give MotionChain(bidirectional=False)'s merged bit for bit,
    under every policy (and that equals cpu_ref.merge_motion: tests/test_gpu_mv_records.py)."""
    from arseg_amd import _lib, ingest, synth

    recs = [_dev(r, dev) for r in synth.make_record_chain(21 + F_, H, W, F_)]
    want = ingest.MotionChain(H, W, gop=F_ + 1, device=dev).push_gop(recs).clone()
    for policy in oracle.POLICIES:
        chain = ingest.MotionChain(H, W, gop=F_ + 1, device=dev, bidirectional=True, bipred=policy)
        got = chain.push_gop(recs)
        assert got.shape == (F_ + 1, H, W, 2) and got.data_ptr() == chain.merged.data_ptr()
        assert torch.equal(got, want), policy
        assert chain.frames_done() == tuple(range(F_ + 1)) and bool((chain.index_map == -1).all())
        with pytest.raises(_lib.ArsegError):                  # the GOP is full
            chain.push(recs[0])


def test_padded_buffers_host_records_and_a_larger_gop_buffer(dev):
    """One generated GOP three more ways through MotionChain: records padded to a fixed capacity, records handed over as numpy arrays, and a
    gop-16 chain holding the 8-frame GOP (a forward target in 8..15 is a frame not pushed, not a frame outside the buffer: equally
    unusable).  reset() between GOPs leaves nothing behind."""
    from arseg_amd import ingest

    H, W, order, max_ref = 24, 40, oracle.ORDERS[2], 3
    for policy in oracle.POLICIES:
        pushes, want, _ = oracle.generated(H, W, order, max_ref, policy)
        cap = max(r.shape[0] for _, r in pushes) + 9
        chain = ingest.MotionChain(H, W, gop=oracle.GOP, max_ref=max_ref, device=dev, bidirectional=True, bipred=policy)
        got = chain.push_gop([_dev(ingest.pad_records(r, cap), dev) for _, r in pushes], order=[f for f, _ in pushes])
        assert np.array_equal(got.cpu().numpy(), want)
        got = chain.push_gop([r for _, r in pushes], order=order)               # host records, the same chain again
        assert np.array_equal(got.cpu().numpy(), want)
        big = ingest.MotionChain(H, W, gop=16, max_ref=max_ref, device=dev, bidirectional=True, bipred=policy)
        got = big.push_gop([_dev(r, dev) for _, r in pushes], order=order)
        assert got.shape == (oracle.GOP, H, W, 2) and np.array_equal(got.cpu().numpy(), want)
        assert big.frames_done() == tuple(range(oracle.GOP))


def test_push_order_rules_and_mv_q_prefix(dev):
    """push refuses an index outside [1, gop) and a frame pushed twice; `at` defaults to the lowest index not pushed; mv_q() raises while the
    frames pushed are not 1..k and returns once they are."""
    from arseg_amd import _lib, ingest

    H, W, order = 8, 8, oracle.ORDERS[1]
    pushes, want, _ = oracle.generated(H, W, order, 3, "near")
    chain = ingest.MotionChain(H, W, gop=oracle.GOP, device=dev, bidirectional=True, bipred="near")
    assert chain.frames_done() == (0,) and chain.mv_q().shape[0] == 1
    by_frame = dict(pushes)
    for at in (0, -1, oracle.GOP, 64):
        with pytest.raises(_lib.ArsegError):
            chain.push(by_frame[3], at=at)
    out = chain.push(by_frame[3], at=3)
    assert out.data_ptr() == chain.merged[3].data_ptr() and chain.frames_done() == (0, 3)
    with pytest.raises(_lib.ArsegError):
        chain.push(by_frame[3], at=3)
    with pytest.raises(_lib.ArsegError):
        chain.mv_q()
    chain.push(by_frame[1])                                    # at = None: frame 1
    assert chain.frames_done() == (0, 1, 3)
    with pytest.raises(_lib.ArsegError):
        chain.mv_q()
    chain.push(by_frame[2])                                    # at = None: frame 2
    assert chain.mv_q().shape[0] == 4 and np.array_equal(chain.mv_q().cpu().numpy(), want[:4])
    for f in order[3:]:
        chain.push(by_frame[f], at=f)
    assert np.array_equal(chain.mv_q().cpu().numpy(), want)
    with pytest.raises(_lib.ArsegError):                       # every frame is in
        chain.push(by_frame[1])
    plain = ingest.MotionChain(H, W, gop=oracle.GOP, device=dev)
    with pytest.raises(_lib.ArsegError):                       # an in-order chain takes frame 1 first
        plain.push(by_frame[3], at=3)
    assert plain.frames_done() == (0,)


def test_graph_replays_one_decode_order_on_refilled_records(dev):
    """reset + seven pushes in order [3,1,2,6,4,5,7] over static padded record buffers captured in one torch.cuda.graph (done_mask is a
    kernel argument, so the graph holds this decode order); the buffers are refilled in place with a second GOP and the graph replayed."""
    from arseg_amd import ingest

    H, W, order, max_ref, policy = 37, 53, oracle.ORDERS[1], 3, "mean"
    a, want_a, _ = oracle.generated(H, W, order, max_ref, policy)
    b = oracle.make_gop(oracle.SEED + 1, H, W, order, max_ref)
    want_b = oracle.chain(b, H, W, oracle.GOP, max_ref, policy)
    assert not np.array_equal(want_a, want_b)
    cap = max(r.shape[0] for _, r in a + b) + 5
    static = [_dev(ingest.pad_records(r, cap), dev) for _, r in a]
    chain = ingest.MotionChain(H, W, gop=oracle.GOP, max_ref=max_ref, device=dev, bidirectional=True, bipred=policy)

    def step():
        chain.reset()
        for s, f in zip(static, order):
            chain.push(s, at=f)
        return chain.mv_q()

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
        chain.merged[1:].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert out.data_ptr() == chain.merged.data_ptr() and np.array_equal(out.cpu().numpy(), want)


def test_end_to_end_fast_path(dev, manifest):
    """CamVid PSPNet fp32, manifest weights: alter_res_batch_fast fed the completed B-frame chain's mv_q()[1:] gives torch.equal logits to
    the same call fed ingest.chain_records_numpy's field."""
    import test_gpu_models as tm
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, synth

    hr, lr = tm._psp(manifest, dev, False), tm._psp(manifest, dev, True)
    H, W, gop, order = 64, 96, 4, (2, 1, 3)
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    pushes = oracle.make_gop(oracle.SEED, H, W, order, 3, gop=gop)
    chain = ingest.MotionChain(H, W, gop=gop, device=dev, bidirectional=True, bipred="near")
    mv_chain = chain.push_gop([_dev(r, dev) for _, r in pushes], order=order)
    mv_host = torch.from_numpy(ingest.chain_records_numpy(pushes, H, W, gop, 3, "near")).to(dev)
    assert torch.equal(mv_chain, mv_host) and bool((mv_chain[1:] != 0).any())
    with torch.no_grad():
        _, feat = hr.forward_keyframe(frames[0:1])
        out_c, _ = ev.alter_res_batch_fast(lr, [feat[0]] * (gop - 1), frames[1:], mv_chain[1:], 0.5)
        out_h, _ = ev.alter_res_batch_fast(lr, [feat[0]] * (gop - 1), frames[1:], mv_host[1:], 0.5)
        out_0, _ = ev.alter_res_batch_fast(lr, [feat[0]] * (gop - 1), frames[1:], torch.zeros_like(mv_host[1:]), 0.5)
    assert out_c.shape == out_h.shape and bool(torch.isfinite(out_c).all())
    assert torch.equal(out_c, out_h)
    assert not torch.equal(out_c, out_0)                      # the motion reaches the logits
