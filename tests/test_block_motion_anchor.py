"""Host checks of the keyframe anchoring (include/arseg_hip.h, arseg_block_motion_anchor_fwd): ingest.block_motion_anchor_numpy against the
loop oracle of tests/block_motion_anchor_oracle.py, the hand-built cases with what they must give, the capability on the panned GOP with an
occluder, and the C entry point's refusals (validation comes before any launch, so they need no GPU).  Integers: every comparison is exact."""
import ctypes

import numpy as np
import pytest

import block_motion_anchor_oracle as oracle


def _numpy(c, **kw):
    from arseg_amd import ingest

    c = dict(c, **kw)
    return ingest.block_motion_anchor_numpy(c["cur"], c["key"], c["records"], c["mp"], c["f"], B=c["B"], r=c["r"], lam=c["lam"], intra=c["intra"])


def _loops(c, **kw):
    c = dict(c, **kw)
    return oracle.anchor(c["cur"], c["key"], c["records"], c["mp"], c["f"], c["B"], c["r"], c["lam"], c["intra"])


@pytest.mark.parametrize("case", oracle.grid_cases(), ids=oracle.case_id)
def test_numpy_form_equals_the_loops(case):
    """5 x 7 is one clipped block, 16 x 16 one block without neighbours, 37 x 53 has clipped blocks on both edges; r, lam, intra and f inside."""
    from arseg_amd import ingest

    kind, H, W, B = case
    cur, key, rec, mp = oracle.case(*case)
    anchored = 0
    for r in oracle.REFINES:
        for lam in oracle.LAMS:
            win = oracle.winners_of(kind, H, W, B, r, lam)
            for intra in oracle.INTRAS:
                for f in oracle.FRAMES:
                    want = oracle.outputs(win, rec, f, intra, H, W, B)
                    got = ingest.block_motion_anchor_numpy(cur, key, rec, mp, f, B=B, r=r, lam=lam, intra=intra)
                    assert oracle.same(got, want), (r, lam, intra, f)
                    anchored += int(want[2][0]) if intra == 20 else 0
    if (H, W) == (37, 53):                                             # (a block that fills its frame has (0, 0) alone, which matches no noise)
        n = 18 * len(rec)
        assert 0 < anchored and (anchored < n or kind != "noise")      # the bound in the middle separates on noise: some anchor, some do not


def test_constant_image_cost_alone_decides():
    """Every SAD is 0: with lam > 0 the candidate nearest C1 wins; with lam = 0 the smallest dy, then the smallest dx, of the whole union."""
    H, W, B = 37, 53, 16
    cur, key, rec, mp = oracle.case("constant", H, W, B)
    for r in (1, 3):
        win = oracle.winners_of("constant", H, W, B, r, 0)
        for b, (dx, dy, sad, _, _) in enumerate(win):
            _, _, x0, y0, w, h = oracle.geometry(b, H, W, B)
            cands = oracle.candidates(oracle.centres(b, rec, mp, H, W, B), r, x0, y0, w, h, H, W)
            assert sad == 0 and (dy, dx) == min((c[1], c[0]) for c in cands)
        for dx, dy, sad, drift, _ in oracle.winners_of("constant", H, W, B, r, 3)[5:6]:      # block 5 is interior: its own prediction is a candidate
            assert (sad, drift) == (0, 0)


def test_stripes_tie_to_the_smallest_dx():
    """Period 4: dx and dx + 4 tie at SAD 0 for every dy; at lam = 0 the winner has the smallest dy of the union, then the smallest such dx."""
    H, W, B = 37, 53, 8
    cur, key, rec, mp = oracle.case("stripes", H, W, B)
    for b, (dx, dy, sad, _, _) in enumerate(oracle.winners_of("stripes", H, W, B, 3, 0)):
        _, _, x0, y0, w, h = oracle.geometry(b, H, W, B)
        cands = oracle.candidates(oracle.centres(b, rec, mp, H, W, B), 3, x0, y0, w, h, H, W)
        zero = [(c[1], c[0]) for c in cands if (c[0] - oracle.TOTAL[0]) % 4 == 0 or w < 4]
        if zero and w >= 4:
            assert sad == 0 and (dy, dx) == min(zero)


@pytest.mark.parametrize("name", sorted(oracle.hand_cases()))
def test_hand_built_cases_numpy_equals_loops(name):
    c = oracle.hand_cases()[name]
    assert oracle.same(_numpy(c), _loops(c))


def test_hand_built_cases_give_what_they_were_built_for():
    cases = oracle.hand_cases()
    T = oracle.TOTAL
    # one block that fills the frame: (0, 0) whatever the centres say
    rec, sad, st = _loops(cases["only (0, 0) remains"])
    assert tuple(rec[0]) == (0, 0, 16, 16, 0, 0, 2, 0) and st[0] == 1 and st[3] == abs(0 - (10 + 100)) + abs(0 - (-9 + 100))
    # predictions at +-8191 + the hop: every candidate around them is off the frame; (0, 0) and its neighbours remain
    for name in ("predictions far outside", "predictions far outside, B = 8"):
        c = cases[name]
        counts = []
        win = oracle.winners(c["cur"], c["key"], c["records"], c["mp"], c["B"], c["r"], c["lam"], counts)
        assert max(counts) <= (2 * c["r"] + 1) ** 2 and all(abs(dx) <= c["r"] and abs(dy) <= c["r"] for dx, dy, *_ in win)
        assert max(w[3] for w in win) > 2 * 8191 and oracle.same(_numpy(c), _loops(c))
    # coinciding centres: the union is one window
    for name, v in (("coinciding centres", (0, 0)), ("coinciding centres, moving", T)):
        c = cases[name]
        counts = []
        win = oracle.winners(c["cur"], c["key"], c["records"], c["mp"], c["B"], c["r"], c["lam"], counts)
        H, W = c["cur"].shape
        cs = oracle.centres(5, c["records"], c["mp"], H, W, 16)        # block 5 is interior: seven centres, of which the co-located one is T - HOP
        distinct = {(0, 0), v, (v[0] - oracle.HOP[0], v[1] - oracle.HOP[1])} if v != (0, 0) else {(0, 0)}
        assert len(cs) == 7 and set(cs) == distinct
        assert max(counts) <= len(distinct) * (2 * c["r"] + 1) ** 2 and win[5][:4] == (v[0], v[1], 0, 0)
    # an unusable hop: (hx, hy) = (0, 0), so C1 = C2 = the co-located vector; healed blocks are counted; a neighbour's unusable hop proposes nothing
    c = cases["unusable hops"]
    H, W = c["cur"].shape
    cs5 = oracle.centres(5, c["records"], c["mp"], H, W, 16)
    assert cs5[1] == cs5[2] and len(cs5) == 3 + 2                      # left (4) and lower (9) are usable; right (6, ref 3) and upper (1, ref -1) are not
    assert len(oracle.centres(2, c["records"], c["mp"], H, W, 16)) == 3 + 1      # upper row: left (1) and right... 1 is unusable, 3 usable, lower 6 unusable
    rec, sad, st = _loops(c)
    assert st[1] >= 1 and rec[5, 6] == 3 and tuple(rec[5, 4:6]) == (4 * T[0], 4 * T[1])
    # the rounding and the shift land on the truth at drift 0
    for name in ("hop fields 6 and 10", "merged_prev -3 and 5"):
        c = cases[name]
        H, W = c["cur"].shape
        assert oracle.pred(5, c["records"], c["mp"], H, W, 16) == T
        rec, sad, st = _loops(c)
        assert tuple(rec[5, 4:7]) == (4 * T[0], 4 * T[1], c["f"] - 1) and sad[5] == 0
    for name in ("one row of blocks", "one column of blocks"):
        c = cases[name]
        H, W = c["cur"].shape
        assert max(len(oracle.centres(b, c["records"], c["mp"], H, W, 8)) for b in range(len(c["records"]))) == 5


def test_f_1_copies_through():
    from arseg_amd import ingest

    cur, key, rec, mp = oracle.case("noise", 37, 53, 16)
    for fn in (lambda: ingest.block_motion_anchor_numpy(cur, key, rec, None, 1, B=16, r=2, lam=2, intra=255), lambda: oracle.anchor(cur, key, rec, None, 1, 16, 2, 2, 255)):
        out, sad, st = fn()
        assert np.array_equal(out, rec) and out is not rec and (sad == -1).all() and not st.any()


def test_acceptance_bound_at_and_one_above():
    at, above = oracle.bound_case(0), oracle.bound_case(1)
    for fn in (_numpy, _loops):
        rec, sad, st = fn(at)
        assert tuple(rec[0]) == (0, 0, 16, 16, 0, 0, 1, 0) and sad[0] == 3 * 256 and tuple(st) == (1, 0, 0, 4)       # the hop said (2, 2)
        rec, sad, st = fn(above)
        assert np.array_equal(rec, above["records"]) and sad[0] == -1 and tuple(st) == (0, 0, 1, 0)
        rec, sad, st = fn(above, intra=4)
        assert rec[0, 6] == 1 and sad[0] == 3 * 256 + 1


def test_stats_count_what_they_name():
    c = oracle.hand_cases()["unusable hops"]
    H, W = c["cur"].shape
    win = oracle.winners(c["cur"], c["key"], c["records"], c["mp"], 16, c["r"], c["lam"])
    rec, sad, st = _numpy(c)
    anchored = sad >= 0
    assert st[0] == anchored.sum() and st[2] == (~anchored).sum() and st[0] + st[2] == len(win)
    assert st[1] == sum(1 for b, w in enumerate(win) if anchored[b] and not w[4]) and st[3] == sum(w[3] for b, w in enumerate(win) if anchored[b])
    assert np.array_equal(rec[~anchored], c["records"][~anchored]) and (rec[anchored, 6] == c["f"] - 1).all()


def test_numpy_form_refuses():
    from arseg_amd import ingest

    cur, key, rec, mp = oracle.case("noise", 37, 53, 16)
    for kw in (dict(B=12), dict(r=0), dict(r=4), dict(lam=256), dict(intra=-1), dict(f=0), dict(f=17)):
        args = dict(dict(f=2, B=16, r=2, lam=2, intra=20), **kw)
        with pytest.raises(ValueError):
            ingest.block_motion_anchor_numpy(cur, key, rec, mp, **args)
    with pytest.raises(ValueError):
        ingest.block_motion_anchor_numpy(cur, key[:, :-1], rec, mp, 2)
    with pytest.raises(ValueError):
        ingest.block_motion_anchor_numpy(cur, key, rec[:-1], mp, 2)
    with pytest.raises(ValueError):
        ingest.block_motion_anchor_numpy(cur, key, rec, mp[:-1], 2)


def test_c_abi_refuses_bad_arguments():
    from arseg_amd import _lib

    lib = _lib.load()
    assert _lib.BMA_NSTATS == oracle.NSTATS
    cases = oracle.abi_cases()
    assert len(cases) >= 35
    for name, args, want in cases:
        assert lib.arseg_block_motion_anchor_fwd(*args) == want == _lib.ARSEG_EINVAL, name


# ---- the capability ----
def _hop(cur, prev):
    from arseg_amd import ingest

    return ingest.block_motion_numpy(cur, prev, B=oracle.CAP["B"], R=oracle.CAP["R"], lam=oracle.CAP["lam"], intra=oracle.CAP["intra"])[0]


def _anchor_loops(cur, key, rec, mp, f):
    return oracle.anchor(cur, key, rec, mp, f, oracle.CAP["B"], oracle.CAP["r"], oracle.CAP["lam"], oracle.CAP["intra"])


def _anchor_numpy(cur, key, rec, mp, f):
    from arseg_amd import ingest

    return ingest.block_motion_anchor_numpy(cur, key, rec, mp, f, B=oracle.CAP["B"], r=oracle.CAP["r"], lam=oracle.CAP["lam"], intra=oracle.CAP["intra"])


@pytest.fixture(scope="module")
def plain():
    return oracle.run_gop(_hop)


@pytest.fixture(scope="module")
def anchored():
    return oracle.run_gop(_hop, _anchor_loops)


def test_plain_chain_drifts_and_never_heals(plain):
    """What anchoring is for, first without it: the occluder of frame 2 is gone in frame 3, but every pixel whose chain passes through it keeps
    its flag to the end of the GOP, and the interior error grows."""
    from arseg_amd import ingest

    merged, link, _, _ = plain
    y0, y1, x0, x1 = oracle.OCC
    assert (link[2][y0:y1, x0:x1] & ingest.LINK_INTRA).all()
    for f in (3, 4, 5):                                                # frame f's pixel (x, y) was at (x + 3 (f - 2), y - 2 (f - 2)) in frame 2
        sx, sy = oracle.PAN[0] * (f - 2), oracle.PAN[1] * (f - 2)
        through = link[f][y0 - sy:y1 - sy, x0 - sx:x1 - sx]
        assert (through & ingest.LINK_INTRA).all(), f
    errors = [oracle.off_truth(merged[f], f) for f in range(1, oracle.GOP)]
    assert errors[0] == 0 and 0 < errors[1] < errors[2] < errors[3] < errors[4]
    flagged = [int((link[f] & 7 != 0).sum()) for f in range(1, oracle.GOP)]
    assert flagged[0] == int(oracle.leaves_frame(1).sum()) == 13 * 256 and flagged[4] > flagged[1] > flagged[0]


def test_anchored_chain_is_exact_and_heals(anchored, plain):
    merged, link, pushes, stats = anchored
    assert np.array_equal(merged[1], plain[0][1]) and stats[1] is not None and not stats[1].any()      # f = 1: the hop is the anchor
    assert oracle.off_truth(merged[2], 2) == 32 * 32                   # the occluder itself, and nothing else
    for f in (3, 4, 5):
        assert oracle.off_truth(merged[f], f) == 0, f
        assert np.array_equal(link[f] & 7 != 0, oracle.leaves_frame(f)), f
        assert (link[f][~oracle.leaves_frame(f)] >> 4 == 1).all()       # one hop to the keyframe
    assert stats[3][1] > 0                                             # blocks that were intra at frame 3's hop (the occluder leaving) are healed
    assert all(int(s[0]) >= 31 for s in stats[2:])


def test_anchoring_removes_a_corrupted_hop(anchored):
    def corrupt(f, rec):
        rec = rec.copy()
        if f == 2:
            rec[9, 4] += 8
        return rec

    merged, link, _, stats = oracle.run_gop(_hop, _anchor_loops, corrupt)
    assert np.array_equal(merged[2:], anchored[0][2:]) and np.array_equal(link[2:], anchored[1][2:])
    assert stats[2][3] > 0 and stats[2][3] == anchored[3][2][3] + 2
    plain_bad = oracle.run_gop(_hop, None, corrupt)[0]
    assert all(oracle.off_truth(plain_bad[f], f) > 0 for f in (2, 3, 4, 5))


def test_numpy_form_runs_the_capability_like_the_loops(anchored):
    merged, link, pushes, stats = oracle.run_gop(_hop, _anchor_numpy)
    assert np.array_equal(merged, anchored[0]) and np.array_equal(link, anchored[1])
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(pushes, anchored[2])) and all(np.array_equal(a, b) for a, b in zip(stats[1:], anchored[3][1:]))
