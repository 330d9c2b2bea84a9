"""CPU-side checks of the link bytes along the motion chain: the oracle (tests/mv_link_oracle.py) against its hand-written literals,
ingest.chain_records_numpy(return_link=True) against the oracle, the bi / P equivalence, the statistics invariants, the spread of the generated
inputs, ingest.LinkMonitor, and the argument validation of the four new entry points, which happens before any launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import mv_link_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = oracle.hand_cases()
ORDER_IDS = ["".join(map(str, o)) for o in oracle.ORDERS]


@pytest.mark.parametrize("case", HAND, ids=lambda c: c[0])
def test_oracle_equals_its_literals(case):
    _, max_ref, gop, pushes, expected = case
    for policy in oracle.POLICIES:
        want = oracle.hand_expected(expected[policy], gop)
        assert np.array_equal(oracle.chain(pushes, 8, 8, gop, max_ref, policy), want), policy
        if oracle.is_p_case(pushes):
            assert np.array_equal(oracle.chain_p([r for _, r in pushes], 8, 8, gop, max_ref), want)


def test_hand_cases_exercise_what_their_names_say():
    cases = {name: (gop, pushes, exp) for name, _, gop, pushes, exp in HAND}
    assert len(cases) == 10 and sum(oracle.is_p_case(p) for _, p, _ in cases.values()) == 7
    gop, _, exp = cases["an intra block whose flag survives three further hops"]
    assert all(exp["list0"][f][3][3] == (f << 4 | oracle.INTRA) and exp["list0"][f][0][0] == f << 4 for f in (1, 2, 3, 4))
    _, _, exp = cases["a 17-frame chain of ref 0 links saturating at 15"]
    assert exp["mean"][14][0][0] == 0xe0 and exp["mean"][15][0][0] == exp["mean"][16][0][0] == exp["mean"][17][0][0] == 0xf0
    _, _, exp = cases["a bi block with one clamped and one clean list"]
    assert exp["list0"][2] == exp["near"][2] != exp["mean"][2]
    _, _, exp = cases["a bi block, NEAR takes the clamped list 1"]
    assert exp["list0"][2] != exp["near"][2] == exp["mean"][2]
    _, _, exp = cases["an unusable winner over a usable lower index"]
    assert exp["list0"][2][3][2] == 0x21 and exp["list0"][2][0][0] == 0x22 and exp["list0"][2][3][4] == 0x20
    _, _, exp = cases["intra with a gap in D"]
    assert exp["near"][3] == exp["near"][2] and exp["near"][3][0][0] == 0x23
    _, _, exp = cases["ref 2 from frame 2"]
    assert exp["list0"][2][0][0] == 0x10


@pytest.mark.parametrize("case", HAND, ids=lambda c: c[0])
def test_chain_records_numpy_on_the_hand_cases(case):
    from arseg_amd import ingest

    _, max_ref, gop, pushes, expected = case
    for policy in oracle.POLICIES:
        merged, link = ingest.chain_records_numpy(pushes, 8, 8, gop, max_ref, policy, return_link=True)
        assert link.dtype == np.uint8 and link.shape == (gop, 8, 8) and merged.dtype == np.int16
        assert np.array_equal(link, oracle.hand_expected(expected[policy], gop)), policy
        assert np.array_equal(merged, ingest.chain_records_numpy(pushes, 8, 8, gop, max_ref, policy))


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("order", oracle.ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("H,W", oracle.SHAPES)
def test_chain_records_numpy_on_generated_gops(H, W, order, max_ref):
    from arseg_amd import ingest

    for policy in oracle.POLICIES:
        pushes, want = oracle.generated(H, W, order, max_ref, policy)
        merged, link = ingest.chain_records_numpy(pushes, H, W, oracle.GOP, max_ref, policy, return_link=True)
        assert np.array_equal(link, want), policy
        plain = ingest.chain_records_numpy(pushes, H, W, oracle.GOP, max_ref, policy)
        assert isinstance(plain, np.ndarray) and np.array_equal(merged, plain)          # merged identical with and without return_link
        st = oracle.stats(want)
        assert (st[:, 4:].sum(axis=1) == H * W).all()                                     # the hop bins partition the frame
        assert (st[:, 3] <= st[:, 0] + st[:, 1] + st[:, 2]).all() and (st[:, 3] >= st[:, :3].max(axis=1)).all()
        assert not st[0, :4].any() and st[0, 4] == H * W and not st[1:, 4].any()          # frame 0: no flag, no hop; no other frame has 0 hops
    assert inspect.signature(ingest.chain_records_numpy).parameters["return_link"].default is False


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("H,W", oracle.SHAPES)
def test_bi_in_order_equals_p(H, W, max_ref):
    """Every record in list 0, frames in order: the bi entry's bytes are the P entry's, under every policy -- for the oracle's two walks and
    for chain_records_numpy."""
    from arseg_amd import ingest

    pushes, _ = oracle.generated(H, W, oracle.ORDERS[0], max_ref, "list0", False)
    assert oracle.is_p_case(pushes)
    want = oracle.chain_p([r for _, r in pushes], H, W, oracle.GOP, max_ref)
    assert (want[-1] & 7).any() and (want[-1] >> 4).max() >= 3
    for policy in oracle.POLICIES:
        assert np.array_equal(oracle.generated(H, W, oracle.ORDERS[0], max_ref, policy, False)[1], want), policy
        assert np.array_equal(ingest.chain_records_numpy(pushes, H, W, oracle.GOP, max_ref, policy, return_link=True)[1], want), policy


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("order", oracle.ORDERS, ids=ORDER_IDS)
def test_generated_gops_have_the_spread(order, max_ref):
    """So that a passing comparison cannot hide an empty case: per decode order (and max_ref, at both multi-block shapes) the oracle alone
    finds each flag on 1 % .. 60 % of the last frame's pixels, hop counts 1 to 4 all present, and pixels whose flag is inherited."""
    for H, W in ((24, 40), (37, 53)):
        own = {}
        pushes = oracle.generated(H, W, order, max_ref, "mean")[0]
        link = oracle.chain(pushes, H, W, oracle.GOP, max_ref, "mean", own)
        last = link[oracle.GOP - 1]
        for bit in range(3):
            share = float(((last >> bit) & 1).sum()) / (H * W)
            assert 0.01 <= share <= 0.60, (H, W, bit, share)
        assert {1, 2, 3, 4} <= set(np.unique(link[1:] >> 4).tolist())
        inherited = sum(int((((link[f] & 7) & ~own[f]) != 0).sum()) for f in own)
        assert inherited > 0
        list0, near = (oracle.generated(H, W, order, max_ref, pol)[1] for pol in ("list0", "near"))
        assert not np.array_equal(list0, link) and (order == oracle.ORDERS[0] or not np.array_equal(list0, near))
        rec = np.concatenate([r for _, r in pushes])
        assert (rec[:, 7] & 1).any() and ((rec[:, 2] <= 0) & (rec[:, 3] <= 0)).any()


def test_banded_gop_is_what_it_says():
    pushes, link = oracle.generated_banded(3)
    H, W = oracle.BANDED
    assert H > 256 and len(pushes) == 3 and all(r[0, 2] > W and r[0, 3] > H for _, r in pushes)
    assert not (link[1:] & oracle.UNCOVERED).any() and (link[3] & oracle.INTRA).any() and (link[3] & oracle.CLAMPED).any()
    assert set(np.unique(link[3] >> 4).tolist()) >= {1, 2, 3}


def test_link_constants_and_hops():
    import torch

    from arseg_amd import _lib, ingest

    assert (ingest.LINK_INTRA, ingest.LINK_UNCOVERED, ingest.LINK_CLAMPED) == (1, 2, 4) == (oracle.INTRA, oracle.UNCOVERED, oracle.CLAMPED)
    assert _lib.LINK_NSTATS == 20 == oracle.NSTATS
    plane = np.array([[0x00, 0x17, 0xf2, 0x30]], dtype=np.uint8)
    assert ingest.link_hops(plane).tolist() == [[0, 1, 15, 3]]
    assert ingest.link_hops(torch.from_numpy(plane)).tolist() == [[0, 1, 15, 3]]


def test_link_monitor_decisions():
    from arseg_amd import ingest

    def row(intra, uncovered, clamped, any_):
        return [intra, uncovered, clamped, any_] + [0] * 16

    n = 1000
    mon = ingest.LinkMonitor(0.25)
    assert mon.mask == ingest.LINK_INTRA | ingest.LINK_UNCOVERED
    assert mon.update(row(250, 100, 900, 950), n) is False              # the larger of the two counted flags: exactly 25 %, not above; clamped is not counted
    assert mon.update(row(251, 0, 0, 251), n) is True
    assert mon.update(row(0, 251, 0, 251), n) is True
    assert mon.update(row(200, 200, 0, 400), n) is False                # the row vouches for 200 only (the union is 200 .. 400)
    assert mon.update(row(200, 200, 0, 400), n, flagged=400) is True    # ... the caller counted the union on the plane
    assert mon.update(np.array(row(300, 0, 0, 300), dtype=np.int64), n) is True
    every = ingest.LinkMonitor(0.5, mask=7)
    assert every.update(row(10, 10, 10, 501), n) is True and every.update(row(400, 400, 400, 500), n) is False          # column 3
    only = ingest.LinkMonitor(0.0, mask=ingest.LINK_CLAMPED)
    assert only.update(row(900, 900, 0, 950), n) is False and only.update(row(0, 0, 1, 1), n) is True
    assert ingest.LinkMonitor(1.0).update(row(n, n, n, n), n) is False  # all intra (a scene cut) with the threshold at 1: never above
    assert ingest.LinkMonitor(0.99).update(row(n, 0, 0, n), n) is True
    with pytest.raises(TypeError):
        ingest.LinkMonitor()                                             # no default that pretends to be tuned
    for bad in ((-0.1,), (1.5,), (0.5, 0), (0.5, 8), (0.5, 16)):
        with pytest.raises(ValueError):
            ingest.LinkMonitor(*bad)
    with pytest.raises(ValueError):
        mon.update(row(1, 1, 1, 1), 0)
    assert "calibrate" in ingest.LinkMonitor.__doc__


def test_synth_link_chain_holds_what_make_record_chain_cannot():
    from arseg_amd import ingest, synth

    H, W = 48, 64
    frames = synth.make_link_chain(3, H, W, 5)
    assert len(frames) == 5 and all(r.dtype == np.int16 and r.shape[1] == 8 for r in frames)
    link = oracle.chain_p(frames, H, W, 6, 3)
    for bit in range(3):
        assert 0 < ((link[5] >> bit) & 1).sum() < H * W
    merged, got = ingest.chain_records_numpy(list(enumerate(frames, start=1)), H, W, 6, 3, return_link=True)
    assert np.array_equal(got, link)
    again = synth.make_link_chain(3, H, W, 5)
    assert all(np.array_equal(a, b) for a, b in zip(frames, again))
    base = synth.make_record_chain(3, H, W, 5)                          # the existing generator: every pixel covered
    assert not (oracle.chain_p(base, H, W, 6, 3) & oracle.UNCOVERED).any()


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """ARSEG_EINVAL / ARSEG_EWORKSPACE come back before any launch: everything the plain steps refuse, a null link, a misaligned
    link_stats; the reset's own; the linked consistency form's (device pointers are dummies and never dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72)          # odd: 8- but not 16-byte aligned
    EINVAL, EWS = _lib.ARSEG_EINVAL, _lib.ARSEG_EWORKSPACE
    H, W = 10, 12
    need = H * W * 4

    def step(records=one, n=4, merged=one, f=1, gop=12, ws=one, ws_bytes=need, H=H, W=W, max_ref=3, link=one, stats=one):
        return lib.arseg_mv_records_step_link_fwd(records, n, merged, f, gop, ws, ws_bytes, H, W, max_ref, link, stats, null)

    def bi(records=one, n=4, merged=one, f=1, gop=12, done=1, policy=0, ws=one, ws_bytes=2 * need, H=H, W=W, max_ref=3, link=one, stats=one):
        return lib.arseg_mv_records_bi_step_link_fwd(records, n, merged, f, gop, done, policy, ws, ws_bytes, H, W, max_ref, link, stats, null)

    for fn in (step, bi):
        for bad in (dict(link=null), dict(records=null), dict(merged=null), dict(ws=null), dict(n=-1), dict(H=8193, ws_bytes=1 << 40),
                    dict(W=8193, ws_bytes=1 << 40), dict(H=0), dict(W=0), dict(max_ref=0), dict(max_ref=17), dict(f=0), dict(f=12), dict(f=-1),
                    dict(f=1, gop=1), dict(ws=odd), dict(records=odd), dict(merged=ctypes.c_void_p(18)), dict(stats=ctypes.c_void_p(68))):
            assert fn(**bad) == EINVAL, (fn.__name__, bad)
        assert fn(ws_bytes=0) == EWS and fn(ws_bytes=need - 1) == EWS
    assert bi(ws_bytes=need) == EWS                                                        # one map is not enough
    for bad in (dict(gop=65), dict(f=64, gop=65), dict(done=0), dict(done=0b10), dict(f=1, done=0b11), dict(done=1 | 1 << 12), dict(done=1 | 1 << 63),
                dict(policy=-1), dict(policy=3)):
        assert bi(**bad) == EINVAL, bad

    reset = lib.arseg_mv_link_reset                                                        # (link, link_stats, gop, H, W, stream)
    for args in ((null, one, 12, H, W), (one, one, 0, H, W), (one, one, -1, H, W), (one, one, 12, 0, W), (one, one, 12, H, 8193),
                 (one, one, 12, 8193, W), (one, ctypes.c_void_p(68), 12, H, W)):
        assert reset(*args, null) == EINVAL, args

    def linked(labels=one, in_pitch=W, in_ns=H * W, N=2, n_cls=19, H=H, W=W, ref=one, ref_pitch=W, ref_ns=0, mv=one, chg=one, chg_pitch=W,
               chg_ns=H * W, stats=one, link=one, link_pitch=W, link_ns=H * W, mask=3, unlinked=one):
        return lib.arseg_labels_consistency_linked_fwd(labels, in_pitch, in_ns, N, n_cls, H, W, ref, ref_pitch, ref_ns, mv, chg, chg_pitch, chg_ns,
                                                       stats, link, link_pitch, link_ns, mask, unlinked, null)

    for bad in (dict(link=null), dict(link_pitch=W - 1), dict(link_ns=-1), dict(unlinked=ctypes.c_void_p(68)),
                dict(labels=null), dict(ref=null), dict(mv=null), dict(mv=ctypes.c_void_p(66)), dict(chg=null, stats=null), dict(n_cls=0), dict(n_cls=33),
                dict(N=0), dict(H=0), dict(W=0), dict(in_pitch=W - 1), dict(in_ns=-1), dict(ref_pitch=W - 1), dict(ref_ns=-1), dict(chg_pitch=W - 1),
                dict(chg_ns=-1)):
        assert linked(**bad) == EINVAL, bad


def test_host_layer_refusals_without_a_gpu():
    import torch

    from arseg_amd import _lib, egress, evaluation, ingest, ops

    rec = torch.zeros((4, 8), dtype=torch.int16)
    merged, idx = torch.zeros((3, 8, 8, 2), dtype=torch.int16), torch.zeros(128, dtype=torch.int32)
    link, st = torch.zeros((3, 8, 8), dtype=torch.uint8), torch.zeros((3, 20), dtype=torch.int64)
    with pytest.raises(_lib.ArsegError):                                   # no CPU fallback
        ops.mv_link_reset(link, st)
    with pytest.raises(_lib.ArsegError):
        ops.mv_records_step_link(rec, merged, 1, idx, link, st)
    with pytest.raises(_lib.ArsegError):
        ops.mv_records_bi_step_link(rec, merged, 1, 1, idx, link, st)
    planes, mv = torch.zeros((1, 4, 6), dtype=torch.uint8), torch.zeros((1, 4, 6, 2), dtype=torch.int16)
    with pytest.raises(_lib.ArsegError):
        ops.labels_consistency_linked(planes, planes, mv, 12, planes, 3, change_out=planes.clone())
    with pytest.raises(_lib.ArsegError):
        egress.consistency_of_planes(planes, planes, mv, 12, link=planes)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8, 8, device="cpu", track_links=True)
    sig = inspect.signature(ingest.MotionChain.__init__)
    assert list(sig.parameters)[-1] == "track_links" and sig.parameters["track_links"].default is False
    sig = inspect.signature(egress.consistency_of_planes)
    assert list(sig.parameters)[-3:] == ["link", "link_mask", "unlinked"] and sig.parameters["link"].default is None
    assert sig.parameters["link_mask"].default == 3 and sig.parameters["unlinked"].default is None
    base, mine = inspect.signature(evaluation.alter_res_batch_consistency), inspect.signature(evaluation.alter_res_batch_consistency_linked)
    assert list(mine.parameters) == list(base.parameters) + ["link", "link_mask"]
    assert list(base.parameters) == ["lr_net", "ref_ps", "imgs", "mv_qs", "key_labels", "scale", "lut", "change_out", "labels_out", "stats"]


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, ops

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("arseg_mv_link_reset", 6), ("arseg_mv_records_step_link_fwd", 13), ("arseg_mv_records_bi_step_link_fwd", 15),
                         ("arseg_labels_consistency_linked_fwd", 21)):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        declared = re.search(r"\b%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1]) == n_args, name
    for name, plain in (("arseg_mv_records_step_link_fwd", "arseg_mv_records_step_fwd"), ("arseg_mv_records_bi_step_link_fwd", "arseg_mv_records_bi_step_fwd")):
        assert _lib.PROTOTYPES[name][1][:-3] == _lib.PROTOTYPES[plain][1][:-1]            # the plain step's arguments, then link, link_stats, stream
    assert _lib.PROTOTYPES["arseg_labels_consistency_linked_fwd"][1][:15] == _lib.PROTOTYPES["arseg_labels_consistency_fwd"][1][:15]
    for define, value in (("ARSEG_LINK_INTRA", "1"), ("ARSEG_LINK_UNCOVERED", "2"), ("ARSEG_LINK_CLAMPED", "4"), ("ARSEG_LINK_NSTATS", r"\(4 \+ 16\)")):
        assert re.search(r"#define %s %s\b" % (define, value), header) or re.search(r"#define %s %s" % (define, value), header)
    assert re.search(r"#define ARSEG_ABI_VERSION 5\b", header) and lib.arseg_version() == _lib.ABI_VERSION == 5
    for name in ("mv_link_reset", "mv_records_step_link", "mv_records_bi_step_link", "labels_consistency_linked"):
        assert callable(getattr(ops, name))
