"""GPU checks of the motion-vector record path (csrc/mv_records.hip, arseg_mv_records_*; ingest.MotionChain): rasterisation against the
numpy oracle (tests/mv_records_oracle.py), the chain against the CPU mergeMotion oracle and against ops.merge_motion, streaming, graph
replay over refilled record buffers, and the fast path fed from a MotionChain.  Everything is bit-exact: integers in, integers out, no
tolerance anywhere."""
import numpy as np
import pytest
import torch

import mv_records_oracle as oracle

pytestmark = pytest.mark.gpu

SHAPES = [(720, 960, 4), (37, 53, 11), (8, 8, 1)]           # the three shapes of test_merge_motion (tests/test_gpu_ops.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _dev(rec, dev):
    return torch.from_numpy(np.ascontiguousarray(rec, dtype=np.int16)).to(dev)


def _want_merged(flows, max_ref=3):
    """cpu_ref.merge_motion as the int16 [F+1,H,W,2] the .bin files hold.  max_ref < 3: the oracle's intra rule is `ref < 0 or ref >= 3`,
    so every ref >= max_ref is rewritten to -1 first -- the same rule in the oracle's terms."""
    from oracle import cpu_ref

    d = np.array(flows, copy=True)
    assert max_ref <= 3
    d[..., 2][d[..., 2] >= max_ref] = -1
    return cpu_ref.merge_motion(d).transpose(2, 0, 1, 3).astype(np.int16)


@pytest.mark.parametrize("H,W,F_", SHAPES)
def test_rasterize_record_chain_frames(dev, H, W, F_):
    """ops.mv_records_rasterize of every make_record_chain frame == the oracle == the make_mv_chain field the records came from."""
    from arseg_amd import ops, synth

    flows = synth.make_mv_chain(21 + F_, H, W, F_)
    for f, rec in enumerate(synth.make_record_chain(21 + F_, H, W, F_), start=1):
        got = ops.mv_records_rasterize(_dev(rec, dev), H, W).cpu().numpy()
        assert got.shape == (H, W, 3) and got.dtype == np.int16
        assert np.array_equal(got, flows[f])
        if H * W <= 64 * 64 or f == 1:                       # the per-row python oracle on the large frame once
            assert np.array_equal(got, oracle.rasterize(rec, H, W))


@pytest.mark.parametrize("case", oracle.adversarial_cases(), ids=lambda c: c[0])
def test_rasterize_adversarial(dev, case):
    """Overlaps in both index orders, records partly and wholly off-frame, 1x1 and odd offsets, zero and negative sizes, the empty list,
    padded buffers, every kind of reference index, a set reserved field: the dense field equals the oracle's; twice, so that the second run
    sees the index map the first one left."""
    from arseg_amd import ops

    _, H, W, rec = case
    want = oracle.rasterize(rec, H, W)
    r = _dev(rec, dev)
    for _ in range(2):
        got = ops.mv_records_rasterize(r, H, W).cpu().numpy()
        assert np.array_equal(got, want)


@pytest.mark.parametrize("case", oracle.adversarial_cases(), ids=lambda c: c[0])
def test_chain_adversarial(dev, case):
    """The same lists through MotionChain (three frames of the same records: the third reaches two frames back where ref allows) ==
    cpu_ref.merge_motion of the oracle's dense fields."""
    from arseg_amd import ingest

    _, H, W, rec = case
    dense = oracle.rasterize(rec, H, W)
    flows = np.stack([np.zeros_like(dense), dense, dense, dense])
    chain = ingest.MotionChain(H, W, gop=4, device=dev)
    got = chain.push_gop([_dev(rec, dev)] * 3).cpu().numpy()
    assert np.array_equal(got, _want_merged(flows))


@pytest.mark.parametrize("H,W,F_", SHAPES)
def test_chain_equals_merge_motion(dev, H, W, F_):
    """MotionChain.push_gop(records) == cpu_ref.merge_motion(dense) as int16 == ops.merge_motion of the GPU-rasterised dense fields,
    the whole tensor (frame 0 = -1 included)."""
    from arseg_amd import ingest, ops, synth

    flows = synth.make_mv_chain(21 + F_, H, W, F_)
    recs = [_dev(r, dev) for r in synth.make_record_chain(21 + F_, H, W, F_)]
    chain = ingest.MotionChain(H, W, gop=F_ + 1, device=dev)
    got = chain.push_gop(recs)
    assert got.shape == (F_ + 1, H, W, 2) and got.dtype == torch.int16 and got.data_ptr() == chain.merged.data_ptr()
    assert np.array_equal(got.cpu().numpy(), _want_merged(flows))
    dense = torch.stack([torch.zeros((H, W, 3), dtype=torch.int16, device=dev)] + [ops.mv_records_rasterize(r, H, W) for r in recs])
    assert torch.equal(got, ops.merge_motion(dense))
    with pytest.raises(Exception):                            # the GOP is full
        chain.push(recs[0])


def test_chain_max_ref_1(dev):
    """max_ref = 1: reference indices 1 and 2 of make_mv_chain become intra."""
    from arseg_amd import ingest, synth

    H, W, F_ = 37, 53, 11
    flows = synth.make_mv_chain(21 + F_, H, W, F_)
    assert (flows[..., 2] >= 1).any()
    recs = [_dev(r, dev) for r in synth.make_record_chain(21 + F_, H, W, F_)]
    got = ingest.MotionChain(H, W, gop=F_ + 1, max_ref=1, device=dev).push_gop(recs).cpu().numpy()
    want = _want_merged(flows, max_ref=1)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, _want_merged(flows))      # the argument matters on this input


def test_chain_larger_gop_buffer_and_host_records(dev):
    """A chain with room for more frames than were pushed (gop = 12, 4 pushed) and records handed over as numpy arrays."""
    from arseg_amd import ingest, synth

    H, W, F_ = 40, 56, 4
    flows = synth.make_mv_chain(5, H, W, F_)
    chain = ingest.MotionChain(H, W, gop=12, device=dev)
    got = chain.push_gop(synth.make_record_chain(5, H, W, F_))
    assert got.shape == (F_ + 1, H, W, 2) and np.array_equal(got.cpu().numpy(), _want_merged(flows))


def test_streaming(dev):
    """Each push returns what the batch form holds for that frame, and two different GOPs pushed through ONE MotionChain with reset()
    between them each equal a fresh chain (the index map is left clean, nothing of the first GOP survives)."""
    from arseg_amd import ingest, synth

    H, W, F_ = 72, 104, 11
    gops = [synth.make_record_chain(s, H, W, F_) for s in (3, 4)]
    flows = [synth.make_mv_chain(s, H, W, F_) for s in (3, 4)]
    fresh = [ingest.MotionChain(H, W, gop=F_ + 1, device=dev).push_gop([_dev(r, dev) for r in g]).clone() for g in gops]
    assert not torch.equal(fresh[0], fresh[1])
    chain = ingest.MotionChain(H, W, gop=F_ + 1, device=dev)
    for g, want, fl in zip(gops, fresh, flows):
        chain.reset()
        assert chain.mv_q().shape[0] == 1
        for f, r in enumerate(g, start=1):
            out = chain.push(_dev(r, dev))
            assert out.shape == (H, W, 2) and out.data_ptr() == chain.merged[f].data_ptr()
            assert torch.equal(out, want[f])
            assert chain.mv_q().shape[0] == f + 1
        assert torch.equal(chain.mv_q(), want)
        assert np.array_equal(want.cpu().numpy(), _want_merged(fl))
        assert bool((chain.index_map == -1).all())


def test_graph_capture_replays_refilled_records(dev):
    """reset + eleven pushes over static padded record buffers captured on one stream (executor.GopGraph, one lane); the buffers are
    refilled in place with a second chain and the graph replayed: the result equals the eager result on the second chain."""
    from arseg_amd import ingest, synth
    from arseg_amd.executor import GopGraph

    H, W, F_ = 64, 96, 11
    a = synth.make_record_chain(12, H, W, F_)
    flows_b = synth.make_mv_chain(13, H, W, F_)
    flows_b[:, :32, 32:] = (8, -12, 0)                                   # a calm area: fewer, larger records than chain a holds
    b = [ingest.mv_to_records(d) for d in flows_b[1:]]
    cap = max(r.shape[0] for r in a + b) + 7
    assert all(r.shape[0] != s.shape[0] for r, s in zip(a, b))          # the fill level differs: the padding is what makes the replay valid
    want = [ingest.MotionChain(H, W, gop=F_ + 1, device=dev).push_gop([_dev(r, dev) for r in g]).clone() for g in (a, b)]
    assert not torch.equal(want[0], want[1])
    static = [_dev(ingest.pad_records(r, cap), dev) for r in a]
    chain = ingest.MotionChain(H, W, gop=F_ + 1, device=dev)

    def step():
        chain.reset()
        for s in static:
            chain.push(s)
        return chain.mv_q()

    graph = GopGraph([step], warmup=1, independent=True)
    out = graph.replay()[0]
    torch.cuda.synchronize()
    assert out.data_ptr() == chain.merged.data_ptr() and torch.equal(out, want[0])
    for s, r in zip(static, b):
        s.copy_(_dev(ingest.pad_records(r, cap), dev))
    out = graph.replay()[0]
    torch.cuda.synchronize()
    assert torch.equal(out, want[1])
    for s, r in zip(static, a):                                          # and back
        s.copy_(_dev(ingest.pad_records(r, cap), dev))
    out = graph.replay()[0]
    torch.cuda.synchronize()
    assert torch.equal(out, want[0])


def test_end_to_end_fast_path(dev, manifest):
    """CamVid PSPNet fp32, manifest weights, a synth.make_clip-shaped GOP: alter_res_batch_fast fed chain.mv_q()[1:] built from the records
    of a make_mv_chain GOP gives torch.equal logits to the same call fed ops.merge_motion(dense)[1:]."""
    import test_gpu_models as tm
    from arseg_amd import evaluation as ev
    from arseg_amd import ingest, ops, synth

    hr, lr = tm._psp(manifest, dev, False), tm._psp(manifest, dev, True)
    H, W, gop = 64, 96, 4
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    flows = synth.make_mv_chain(31, H, W, gop - 1)
    chain = ingest.MotionChain(H, W, gop=gop, device=dev)
    mv_chain = chain.push_gop([_dev(r, dev) for r in synth.make_record_chain(31, H, W, gop - 1)])
    mv_dense = ops.merge_motion(torch.from_numpy(flows).to(dev))
    assert torch.equal(mv_chain, mv_dense) and bool((mv_chain[1:] != 0).any())
    with torch.no_grad():
        _, feat = hr.forward_keyframe(frames[0:1])
        out_c, _ = ev.alter_res_batch_fast(lr, [feat[0]] * (gop - 1), frames[1:], mv_chain[1:], 0.5)
        out_d, _ = ev.alter_res_batch_fast(lr, [feat[0]] * (gop - 1), frames[1:], mv_dense[1:], 0.5)
        out_0, _ = ev.alter_res_batch_fast(lr, [feat[0]] * (gop - 1), frames[1:], torch.zeros_like(mv_dense[1:]), 0.5)
    assert out_c.shape == out_d.shape and bool(torch.isfinite(out_c).all())
    assert torch.equal(out_c, out_d)
    assert not torch.equal(out_c, out_0)                      # the motion reaches the logits
