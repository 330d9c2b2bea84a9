"""GPU checks of the links between the regions of two frames (csrc/links.hip, arseg_region_links_fwd; arseg_amd.egress.links): n_pairs, links
and back against the oracle written from the contract (tests/links_oracle.py).  The stand-alone tests feed run codes and region numbers
made by the oracles on the host, so only links.hip runs; the end-to-end tests run the whole chain from logits.  Every output is an integer:
every comparison is np.array_equal.  Nothing here provokes a fault: malformed inputs are exercised only through the argument checks on the
CPU (tests/test_links.py)."""
import numpy as np
import pytest
import torch

import consistency_oracle
import links_oracle as oracle
import regions_oracle
import rle_oracle

pytestmark = pytest.mark.gpu

G32 = np.int32(oracle.GUARD_I32)
G64 = np.int64(oracle.GUARD_I64)
EXTRA = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _guarded(dev, n, guard, dtype):
    return torch.from_numpy(np.full(n, guard, dtype=dtype)).to(dev)


def _up(dev, arrays):
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in arrays]


def _run(dev, cur, ref, mv_q=None, cap=None, ref_cap=None, rcap=None, kcap=None, pcap=None, with_links=True, with_back=True, workspace=None,
         spoil=None):
    """ops.region_links on inputs the oracles made (room for every run and region unless told otherwise), into 0x5A-filled buffers with
    EXTRA guard rows behind them -> the numpy copies (n_pairs [N], links [N,rcap,6], back [N,kcap,4]) after checking them against
    oracle.expected: n_pairs exact, the rows below the region counts exact and intact above, a frame that cannot be linked or has too many
    pairs intact, the guards behind every buffer intact.  spoil: (side, frame) whose n_regions is set to -1 before the call."""
    from arseg_amd import ops

    N, H, W = cur.shape
    want = oracle.link_planes(cur, ref, mv_q)
    a, b = list(oracle.device_inputs(cur, cap)), list(oracle.device_inputs(ref, ref_cap))
    if spoil is not None:
        (a if spoil[0] == "cur" else b)[2][spoil[1]] = -1
    rcap = max(len(w[1]) for w in want) + 2 if rcap is None else rcap
    kcap = max(len(w[2]) for w in want) + 2 if kcap is None else kcap
    pcap = 4 * a[1].shape[1] if pcap is None else pcap
    n_back = _guarded(dev, N + EXTRA, G32, np.int32)
    l_back = _guarded(dev, (N * rcap + EXTRA) * 6, G64, np.int64)
    b_back = _guarded(dev, (N * kcap + EXTRA) * 4, G64, np.int64)
    links = l_back[:N * rcap * 6].view(N, rcap, 6) if with_links else None
    back = b_back[:N * kcap * 4].view(N, kcap, 4) if with_back else None
    ops.region_links(*_up(dev, a), *_up(dev, b), H, W, n_back[:N], links, back, mv_q=None if mv_q is None else torch.from_numpy(mv_q).to(dev),
                     pair_capacity=pcap, workspace=workspace)
    n_got, l_got, b_got = n_back.cpu().numpy(), l_back.cpu().numpy(), b_back.cpu().numpy()
    assert (n_got[N:] == G32).all()
    assert (l_got[N * rcap * 6:] == G64).all() if with_links else (l_got == G64).all()
    assert (b_got[N * kcap * 4:] == G64).all() if with_back else (b_got == G64).all()
    l_all, b_all = l_got[:N * rcap * 6].reshape(N, rcap, 6), b_got[:N * kcap * 4].reshape(N, kcap, 4)
    for n in range(N):
        m = n if ref.shape[0] > 1 else 0
        linkable = a[2][n] >= 0 and b[2][m] >= 0
        e_pairs, e_links, e_back = oracle.expected(want[n], linkable, rcap if with_links else 0, kcap if with_back else 0, pcap,
                                                   np.full((rcap, 6), G64), np.full((kcap, 4), G64))
        assert n_got[n] == e_pairs, (n, int(n_got[n]), e_pairs)
        assert np.array_equal(l_all[n], e_links), n
        assert np.array_equal(b_all[n], e_back), n
    return n_got[:N], l_all, b_all


@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_hand_made_cases(dev, name):
    """Against the oracle, and against the answers written out by hand."""
    cur, ref, mv_q, answers = oracle.HAND[name]
    n_got, l_got, b_got = _run(dev, cur, ref, mv_q)
    for n, (n_pairs, links, back) in enumerate(answers):
        assert n_got[n] == n_pairs
        assert l_got[n, :len(links)].tolist() == [list(r) for r in links] and b_got[n, :len(back)].tolist() == [list(r) for r in back]


@pytest.mark.parametrize("shape", oracle.EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_shapes_with_block_motion(dev, shape):
    """Widths around a wave at H = 3 and small heights at W = 16, random block motion up to +-W pixels: both ends of the two binary searches,
    blocks that leave the frame entirely, stretches of one pair across the 64-pixel passes; with and without motion, shared and
    per-frame references."""
    H, W = shape
    for seed, make in ((700, regions_oracle.noise_planes), (800, regions_oracle.dense_noise)):
        cur, ref = make(seed + H * W, 2, H, W), make(seed + 50 + H * W, 2, H, W)
        ref[1, :, W // 2:] = cur[1, :, W // 2:]                                                 # something to find
        _run(dev, cur, ref, oracle.block_motion(seed + W, 2, H, W, block=4))
        _run(dev, cur, ref[1:2], oracle.block_motion(seed + 1 + W, 2, H, W, block=4, amp=2))
        _run(dev, cur, ref[1:2])


@pytest.fixture(scope="module")
def dense():
    seed, N, H, W = oracle.DENSE
    cur, ref = regions_oracle.dense_noise(seed, N, H, W), regions_oracle.dense_noise(seed + 1, N, H, W)
    mv_q = oracle.block_motion(seed + 2, N, H, W, block=8, amp=3)
    return cur, ref, mv_q, oracle.link_planes(cur, ref, mv_q)


def test_pair_capacities(dev, dense):
    """More than 256 distinct pairs per frame; pcap = the distinct pairs of the busier frame (it fits exactly), one fewer (that frame gets
    -2 and its rows stay untouched, the other frame of the call is exact: _run checks both) and four times as many."""
    cur, ref, mv_q, want = dense
    distinct = [w[0] for w in want]
    assert min(distinct) > 256 and distinct[0] != distinct[1]
    busy = int(np.argmax(distinct))
    n_got, _, _ = _run(dev, cur, ref, mv_q, pcap=max(distinct))
    assert n_got.tolist() == distinct
    n_got, l_got, b_got = _run(dev, cur, ref, mv_q, pcap=max(distinct) - 1)
    assert n_got[busy] == -2 and n_got[1 - busy] == distinct[1 - busy] and (l_got[busy] == G64).all() and (b_got[busy] == G64).all()
    n_got, _, _ = _run(dev, cur, ref, mv_q, pcap=4 * max(distinct))
    assert n_got.tolist() == distinct
    n_got, _, _ = _run(dev, cur, ref, mv_q, pcap=1)
    assert n_got.tolist() == [-2, -2]


def test_record_capacities(dev, dense):
    """rcap / kcap = R, R - 1 and 0 with NULL: the rows below the capacity exact, the 0x5A rows from there on intact, mutual exact without
    back (_run checks all of it)."""
    cur, ref, mv_q, want = dense
    R, K = max(len(w[1]) for w in want), max(len(w[2]) for w in want)
    _run(dev, cur, ref, mv_q, rcap=R, kcap=K)
    _run(dev, cur, ref, mv_q, rcap=R - 1, kcap=K - 1)
    _, l_got, _ = _run(dev, cur, ref, mv_q, with_back=False)
    assert l_got[0, :len(want[0][1]), 4].sum() > 0                                              # mutual links exist, and were found
    _run(dev, cur, ref, mv_q, with_links=False)
    _run(dev, cur, ref, mv_q, with_links=False, with_back=False)
    _run(dev, cur, ref, mv_q, rcap=0, kcap=0, with_links=False, with_back=False)


def test_frames_that_cannot_be_linked(dev):
    """A current frame whose run code overflowed, a reference whose run code overflowed, and n_regions == -1 on either side: n_pairs == -1
    and the frame's rows stay untouched; the other frames of the call are linked as usual."""
    planes = rle_oracle.build(rle_oracle.CASES[1])
    need = [len(r) for r in rle_oracle.encode(planes)[1]]
    worst = int(np.argmax(need))
    mv_q = oracle.block_motion(5, 3, planes.shape[1], planes.shape[2], amp=4)
    ref = np.roll(planes, 1, axis=0)
    n_got, l_got, _ = _run(dev, planes, ref, mv_q, cap=max(need) - 1)
    assert n_got[worst] == -1 and (l_got[worst] == G64).all() and sum(int(k) >= 0 for k in n_got) == 2
    n_got, _, _ = _run(dev, planes, ref, mv_q, ref_cap=max(need) - 1)
    assert n_got[(worst + 1) % 3] == -1 and sum(int(k) >= 0 for k in n_got) == 2
    n_got, _, _ = _run(dev, planes, planes[worst:worst + 1], mv_q, ref_cap=max(need) - 1)       # the shared reference: no frame has links
    assert n_got.tolist() == [-1, -1, -1]
    n_got, _, _ = _run(dev, planes, ref, mv_q, spoil=("cur", 1))
    assert n_got[1] == -1 and n_got[0] >= 0 and n_got[2] >= 0
    n_got, _, _ = _run(dev, planes, ref, mv_q, spoil=("ref", 2))
    assert n_got[2] == -1 and n_got[0] >= 0 and n_got[1] >= 0


def test_own_workspace_and_bit_equality(dev, dense):
    """Two runs of the same call are bit-equal (integer atomics, a table whose outcome does not depend on the order); a caller's workspace
    of exactly the size asked for serves, with guards behind it."""
    from arseg_amd import _lib

    cur, ref, mv_q, want = dense
    first, second = _run(dev, cur, ref, mv_q), _run(dev, cur, ref, mv_q)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    pcap = 2 * max(w[0] for w in want)
    nbytes = _lib.load().arseg_region_links_workspace_bytes(2, pcap)
    assert nbytes == 2 * (32 * pcap + 8)
    ws_back = _guarded(dev, nbytes // 8 + EXTRA, G64, np.int64)
    own = _run(dev, cur, ref, mv_q, pcap=pcap, workspace=ws_back[:nbytes // 8])
    assert (ws_back[nbytes // 8:].cpu().numpy() == G64).all()
    for a, b in zip(first, own):
        assert np.array_equal(a, b)
    with pytest.raises(_lib.ArsegError):
        _run(dev, cur, ref, mv_q, pcap=pcap, workspace=ws_back[:nbytes // 8 - 1])


def _check_frames(found, cur_planes, ref_planes, mv_q):
    """A LinkFrames against the oracle applied to label planes."""
    want = oracle.link_planes(cur_planes.astype(np.uint8), ref_planes.astype(np.uint8), mv_q)
    assert found.needed().cpu().tolist() == [w[0] for w in want]
    host = found.to_host()
    for n, (n_pairs, links, back) in enumerate(want):
        assert np.array_equal(found.links[n, :len(links)].cpu().numpy(), links) and np.array_equal(found.back[n, :len(back)].cpu().numpy(), back)
        for k, name in enumerate(oracle.LINK_FIELDS):
            assert np.array_equal(host[n][0][name], links[:, k]), name
        for k, name in enumerate(oracle.BACK_FIELDS):
            assert np.array_equal(host[n][1][name], back[:, k]), name
    return want


@pytest.mark.parametrize("case", [consistency_oracle.CASES[0], consistency_oracle.CASES[1]], ids=lambda c: c[0])
def test_full_chain_from_logits(dev, case):
    """egress.links(egress.regions(egress.rle(logits, ...)), key_regions, mv_q) equals the oracle applied to ops.argmax_confusion's pred
    and the case's reference planes; links_numpy gives the same from the run codes brought to the host."""
    from arseg_amd import egress, ops

    _, _, N, n_cls, h, w, H, W, align, shared = case
    built = consistency_oracle.build(case)
    logits = torch.from_numpy(built["logits"]).to(dev)
    ref, mv_q = built["ref"], built["mv"]
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=align)[0].cpu().numpy()
    cur = egress.regions(egress.rle(logits, H, W, H * W, align_corners=align), 1024)
    key = egress.regions(egress.rle_of_planes(torch.from_numpy(ref).to(dev), H * W), 1024)
    found = egress.links(cur, key, torch.from_numpy(mv_q).to(dev))
    assert isinstance(found, egress.LinkFrames) and found.cur is cur and found.ref is key and found.pair_capacity == 4 * H * W
    want = _check_frames(found, pred, ref, mv_q)
    assert sum(w[0] for w in want) > 0
    cur_code, key_code = cur.frames.to_host(), key.frames.to_host()
    cur_rr, key_rr = cur.run_region.cpu().numpy(), key.run_region.cpu().numpy()
    for n in range(N):
        m = n if key.N > 1 else 0
        links, back = egress.links_numpy(cur_code[n][0], cur_code[n][1], cur_rr[n], key_code[m][0], key_code[m][1], key_rr[m], H, W, mv_q[n])
        assert np.array_equal(np.stack([links[f] for f in oracle.LINK_FIELDS], axis=1), want[n][1])
        assert np.array_equal(np.stack([back[f] for f in oracle.BACK_FIELDS], axis=1), want[n][2])
    _check_frames(egress.links(cur, key), pred, ref, None)                                      # zero motion


def test_chain_in_one_graph(dev):
    """labels8 + encode + regions + links captured once (every buffer given: nothing is allocated); logits and motion are refilled in
    place; each replay equals the oracle for its own inputs."""
    from arseg_amd import egress, ops

    case = consistency_oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align, _ = case
    built = consistency_oracle.build(case)
    logits = torch.from_numpy(built["logits"]).to(dev)
    mv_q = torch.from_numpy(built["mv"]).to(dev)
    ref = built["ref"][:1]
    key = egress.regions(egress.rle_of_planes(torch.from_numpy(ref).to(dev), H * W), 256)
    cap, rcap = H * W // 2, 256
    labels = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    coded = egress.RleFrames(torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev), H, W)
    found = egress.RegionFrames(torch.zeros((N,), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev),
                                torch.zeros((N, rcap, 8), dtype=torch.int64, device=dev), coded, 8,
                                torch.zeros((N, cap), dtype=torch.int32, device=dev))
    linked = egress.links(found, key, mv_q, pair_capacity=2048)                                 # allocates the buffers the capture reuses

    def chain():
        egress.links(egress.regions(egress.rle(logits, H, W, cap, labels_out=labels, out=coded, align_corners=align), rcap, out=found), key,
                     mv_q, out=linked)

    chain()                                                                                     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    totals = []
    for s in (seed + 60, seed + 61):
        fresh = consistency_oracle.build((case[0], s) + case[2:])
        logits.copy_(torch.from_numpy(fresh["logits"]).to(dev))
        mv_q.copy_(torch.from_numpy(fresh["mv"]).to(dev))
        for t in (linked.n_pairs, linked.links, linked.back, found.n_regions, found.run_region, found.records):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        pred = ops.argmax_confusion(logits, None, H, W, align_corners=align)[0].cpu().numpy()
        want = _check_frames(linked, pred, ref, fresh["mv"])
        totals.append([w[0] for w in want])
    assert totals[0] != totals[1]


def test_alter_res_batch_links(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_links' links are the oracle's on alter_res_batch_render's planes
    and the keyframe's mask."""
    import test_gpu_ingest_formats as tf
    from arseg_amd import egress, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop = 64, 96, 4
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"][1:gop]).to(dev)
    with torch.no_grad():
        logits_k, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * (gop - 1)
        key = egress.regions(egress.rle(logits_k, H, W, H * W), H * W // 4)
        labels_r, _ = ev.alter_res_batch_render(lr, refs, frames[1:gop], mvs, 0.5)
        linked, found, labels = ev.alter_res_batch_links(lr, refs, frames[1:gop], mvs, key, H * W, H * W // 4, 0.5)
    assert isinstance(linked, egress.LinkFrames) and isinstance(found, egress.RegionFrames) and torch.equal(labels, labels_r)
    want = _check_frames(linked, labels_r.cpu().numpy(), key.frames.labels.cpu().numpy(), clip["mv"][1:gop])
    print(f"\npairs per frame {[w[0] for w in want]}, regions per frame {found.needed().cpu().tolist()}")


def test_full_size_frame_pair(dev):
    """One 1024x2048 frame against another with block motion: more than 256 workgroups of rows, thousands of pairs."""
    planes = rle_oracle.blob_planes(77, 2, 1024, 2048)
    mv_q = oracle.block_motion(78, 1, 1024, 2048, block=16, amp=6)
    cur = planes[:1].copy()
    cur[0, :, 1024:] = planes[1, :, 1024:]                                                      # half the frame agrees with the reference
    n_got, _, _ = _run(dev, cur, planes[1:], mv_q)
    assert n_got[0] > 256
