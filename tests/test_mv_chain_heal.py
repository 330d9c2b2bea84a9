"""Host checks of the chain healing (include/arseg_hip.h, arseg_mv_chain_heal_fwd): ingest.mv_chain_heal_numpy against the loop oracle of
tests/mv_chain_heal_oracle.py, the hand-built cases with what each must give, the invariants of every case, the capability on two scenes
(the panned GOP with an occluder as plain hop records; the same pan as off-grid decoder records with intra units through a bidirectional chain
of 20 frames) and the C entry point's refusals (validation comes before any launch, so they need no GPU).  Integers: every comparison is exact."""
import numpy as np
import pytest

import block_motion_anchor_oracle as bma
import mv_chain_heal_oracle as oracle


def _numpy(c, row=None, **kw):
    from arseg_amd import ingest

    return oracle.run_case(ingest.mv_chain_heal_numpy, c, row, **kw)


def _loops(c, row=None, **kw):
    return oracle.run_case(oracle.heal, c, row, **kw)


def _invariants(before_m, before_l, out, mask, row_before):
    """Unflagged pixels and the pixels of blocks that are not healed keep every bit; healed blocks have no flagged pixel left and carry their
    decision; the corrected row is a recount of the new plane where the old row was a recount of the old one."""
    m, l, dec, sad, st, row = out
    H, W = before_l.shape
    touched = np.zeros((H, W), dtype=bool)
    for x0, y0, w, h, vx, vy, state, n in dec.astype(np.int64):
        fl = (before_l[y0:y0 + h, x0:x0 + w] & mask) != 0
        assert n == fl.sum() and state in (0, 1, 2)
        if state == 0:
            touched[y0:y0 + h, x0:x0 + w] = fl
            assert (m[y0:y0 + h, x0:x0 + w][fl] == (vx, vy)).all() and (l[y0:y0 + h, x0:x0 + w][fl] == 0x10).all()
        if state == 2:
            assert (vx, vy) == (0, 0)
    assert np.array_equal(m[~touched], before_m[~touched]) and np.array_equal(l[~touched], before_l[~touched])
    assert st[3] == touched.sum() and st[2] + st[4] == ((before_l & mask) != 0).sum()
    assert np.array_equal((sad >= 0), dec[:, 6] != 2)
    if row is not None:
        assert np.array_equal(row - row_before, oracle.recount(l) - oracle.recount(before_l))


@pytest.mark.parametrize("case", oracle.grid_cases(), ids=oracle.case_id)
def test_numpy_form_equals_the_loops(case):
    """5 x 7 is one clipped block, 16 x 16 one block without neighbours, 37 x 53 has clipped blocks on both edges and neighbours; every r, lam,
    intra, flag_mask and min_flagged inside, on every content and every kind of flagged set."""
    from arseg_amd import ingest

    cur, key, m, l, row = oracle.case(*case)
    B = case[3]
    seen = set()
    for r, lam, intra, mask, mf in oracle.grid_params():
        want = oracle.outputs(oracle.winners_of(*case, r, lam, mask), m, l, B, intra, mask, mf, row)
        got = ingest.mv_chain_heal_numpy(cur, key, m, l, B, r, lam, intra, mask, mf, row)
        assert oracle.same(got, want), (r, lam, intra, mask, mf)
        seen.update(want[2][:, 6].tolist())
        if (r, lam) == (2, 3):
            _invariants(m, l, got, mask, row)
    if case[1:3] == (37, 53) and case[4] != "centres":
        assert seen == {0, 1, 2} or case[0] != "noise"                 # on noise the grid meets healed, kept and skipped blocks


def test_constant_image_cost_alone_decides():
    """Every SAD is 0: with lam = 0 the smallest dy, then the smallest dx, of the whole union wins; everything examined is healed, at intra = 0 too."""
    case = ("constant", 37, 53, 16, "rects")
    cur, key, m, l, row = oracle.case(*case)
    a, k = cur.astype(np.int64), key.astype(np.int64)
    for r in (1, 3):
        win = oracle.winners_of(*case, r, 0, 3)
        assert win
        for b, (dx, dy, sad_fl, _, sad_all) in win.items():
            _, _, x0, y0, w, h = oracle.geometry(b, 37, 53, 16)
            cands = bma.candidates(oracle.centres(b, m, l, 37, 53, 16, 3), r, x0, y0, w, h, 37, 53)
            assert (sad_fl, sad_all) == (0, 0) and (dy, dx) == min((c[1], c[0]) for c in cands)
            assert oracle.winner(b, a, k, m, l, 16, r, 0, 3)[:2] == (dx, dy)
        out = oracle.outputs(win, m, l, 16, 0, 3, 1, row)
        assert out[4][0] == out[4][1] == len(win) and not ((out[1] & 3) != 0).any()


@pytest.mark.parametrize("name", sorted(oracle.hand_cases()) + ["bound", "bound + 1"])
def test_hand_built_cases_numpy_equals_loops(name):
    c = oracle.bound_case(name == "bound + 1") if name.startswith("bound") else oracle.hand_cases()[name]
    row = oracle.recount(c["link"]) + 7
    got, want = _numpy(c, row), _loops(c, row)
    assert oracle.same(got, want)
    _invariants(c["merged"], c["link"], got, c["mask"], row)
    assert oracle.same(_numpy(c)[:5], want[:5]) and _numpy(c)[5] is None


def test_hand_built_cases_give_what_they_were_built_for():
    cases = oracle.hand_cases()
    T = oracle.TOTAL
    v = (4 * T[0], 4 * T[1])
    healed5 = lambda out: out[2][5, 6] == 0 and tuple(out[2][5, 4:6]) == v and out[3][5] == 0
    # one block that fills the frame: (0, 0) whatever the centres say (C1 = (100, 100): the drift counts)
    m, l, dec, sad, st, _ = _loops(cases["only (0, 0) remains"])
    assert tuple(dec[0]) == (0, 0, 16, 16, 0, 0, 0, 256) and tuple(st) == (1, 1, 256, 256, 0, 200) and not m.any() and (l == 0x10).all()
    # coinciding centres: seven centres, two distinct, one window each
    c = cases["coinciding centres"]
    cs = oracle.centres(5, c["merged"], c["link"], 48, 56, 16, 3)
    count = []
    oracle.winner(5, c["cur"].astype(np.int64), c["key"].astype(np.int64), c["merged"], c["link"], 16, 2, 2, 3, count)
    assert len(cs) == 7 and set(cs) == {(0, 0), T} and count[0] <= 2 * 25
    out = _loops(c)
    assert healed5(out) and tuple(out[4]) == (1, 1, 99, 99, 0, 0) and (out[1][18:27, 19:30] == 0x10).all()
    # seven different centres: all are searched; the truth is within 1 of C1 only
    c = cases["seven different centres"]
    cs = oracle.centres(5, c["merged"], c["link"], 48, 56, 16, 3)
    assert len(cs) == 7 and len(set(cs)) == 7 and cs[1] == (T[0] + 1, T[1]) and cs[6] == (T[0] + 2, T[1] - 5)
    out = _loops(c)
    assert healed5(out) and out[4][5] == 1 and (out[1][16:24, 16:32] == 0x20).all()
    # a flagged neighbour centre proposes nothing: block 5 stays; block 4, whose own centre pixel that is, heals on its C1
    kept, used = _loops(cases["a flagged neighbour centre"]), _loops(cases["the same neighbour centre, unflagged"])
    assert kept[2][5, 6] == 1 and kept[2][4, 6] == 0 and (kept[1][16:32, 16:32] == 0x21).all() and kept[1][24, 8] == 0x10
    assert healed5(used) and used[2][4, 6] == 2 and used[4][5] == 20
    c = cases["a flagged neighbour centre"]
    assert T not in oracle.centres(5, c["merged"], c["link"], 48, 56, 16, 3)
    assert T in oracle.centres(5, c["merged"], c["link"], 48, 56, 16, 4)        # under a mask the byte 0x21 does not meet, it is no flag
    # no unflagged pixel: six centres, none near the truth; one spared pixel is C6 and knows it
    none, one = cases["no unflagged pixel in the block"], cases["one unflagged pixel in the block"]
    assert len(oracle.centres(5, none["merged"], none["link"], 48, 56, 16, 3)) == 6
    cs = oracle.centres(5, one["merged"], one["link"], 48, 56, 16, 3)
    assert len(cs) == 7 and cs[6] == T and T not in cs[:6]
    assert _loops(none)[2][5, 6] == 1 and healed5(_loops(one)) and _loops(one)[1][29, 23] == 0x10 and _loops(one)[4][3] == 255
    # the arithmetic shift: (23, -11) >> 2 = (5, -3)
    c = cases["low bits, negative values and +-4 * 8191"]
    cs = oracle.centres(5, c["merged"], c["link"], 48, 56, 16, 3)
    assert cs[1] == T and (8191, -8191) in cs and (-8191, 8191) in cs
    out = _loops(c)
    assert healed5(out) and out[4][5] == 0
    # acceptance is about the flagged pixels alone
    for name, state in (("passes on the block, fails on the flagged pixels", 1), ("fails on the block, passes on the flagged pixels", 0)):
        c = cases[name]
        dx, dy, sad_fl, _, sad_all = oracle.winner(5, c["cur"].astype(np.int64), c["key"].astype(np.int64), c["merged"], c["link"], 16, 2, 2, 3)
        assert (dx, dy) == T and (sad_all <= 20 * 256) == (state == 1) and (sad_fl <= 20 * 16) == (state == 0)
        out = _loops(c)
        assert out[2][5, 6] == state and out[3][5] == sad_fl and ((out[1][20:24, 20:24] == 0x10).all() if state == 0 else (out[1] == c["link"]).all())
    # hop nibbles 1, 7 and 15 leave their bins, 12 pixels enter bin 1; a flag outside the mask does not make a pixel flagged
    c = cases["hop nibbles 1, 7 and 15"]
    row = oracle.recount(c["link"])
    out = _loops(c, row)
    assert healed5(out) and out[2][10, 6] == 2 and out[2][10, 7] == 0 and out[1][40, 40] == 0x24
    assert tuple((out[5] - row)[[0, 1, 2, 3, 4 + 1, 4 + 7, 4 + 15]]) == (-8, -9, -5, -12, 12 - 3, -4, -5) and np.array_equal(out[5], oracle.recount(out[1]))
    assert _loops(c, row, mask=7)[2][10, 6] == 0                        # with CLAMPED in the mask block 10 is examined and heals
    # n(b) = min_flagged and one below
    at, below = _loops(cases["five flagged pixels"]), _loops(cases["five flagged pixels, min_flagged 6"])
    assert healed5(at) and tuple(at[4]) == (1, 1, 5, 5, 0, 0)
    assert tuple(below[2][5]) == (16, 16, 16, 16, 0, 0, 2, 5) and tuple(below[4]) == (0, 0, 0, 0, 5, 0) and below[3][5] == -1
    assert np.array_equal(below[0], cases["five flagged pixels"]["merged"]) and np.array_equal(below[1], cases["five flagged pixels"]["link"])


def test_acceptance_bound_at_and_one_above():
    at, above = oracle.bound_case(0), oracle.bound_case(1)
    for fn in (_numpy, _loops):
        m, l, dec, sad, st, _ = fn(at)
        assert tuple(dec[0]) == (0, 0, 16, 16, 0, 0, 0, 10) and sad[0] == 30 and tuple(st) == (1, 1, 10, 10, 0, 4) and (l[7, 3:13] == 0x10).all()
        m, l, dec, sad, st, _ = fn(above)
        assert tuple(dec[0]) == (0, 0, 16, 16, 0, 0, 1, 10) and sad[0] == 31 and tuple(st) == (1, 0, 10, 0, 0, 0) and np.array_equal(l, above["link"])
        assert fn(above, intra=4)[2][0, 6] == 0


def test_stats_accumulate_over_two_calls():
    """The second call sees the first one's planes: what was healed is skipped, what was kept is examined again; the sums are the oracle's."""
    cur, key, m, l, row = oracle.tiles_case()
    first = oracle.heal(cur, key, m, l, 16, 2, 2, 20, 3, 1, row)
    second = oracle.heal(cur, key, first[0], first[1], 16, 2, 2, 20, 3, 1, first[5])
    assert 0 < first[4][1] < first[4][0] and second[4][0] >= first[4][0] - first[4][1] and second[4][4] == 0
    from arseg_amd import ingest

    a = ingest.mv_chain_heal_numpy(cur, key, m, l, 16, 2, 2, 20, 3, 1, row)
    b = ingest.mv_chain_heal_numpy(cur, key, a[0], a[1], 16, 2, 2, 20, 3, 1, a[5])
    assert oracle.same(a, first) and oracle.same(b, second) and np.array_equal(a[4] + b[4], first[4] + second[4])
    assert np.array_equal(b[5], oracle.recount(b[1]))


def test_numpy_form_refuses():
    from arseg_amd import ingest

    cur, key, m, l, row = oracle.case("noise", 37, 53, 16, "rects")
    ok = dict(B=16, r=2, lam=2, intra=20, flag_mask=3, min_flagged=1)
    for kw in (dict(B=12), dict(r=0), dict(r=4), dict(lam=256), dict(intra=-1), dict(flag_mask=0), dict(flag_mask=8), dict(min_flagged=0), dict(min_flagged=65)):
        with pytest.raises(ValueError):
            ingest.mv_chain_heal_numpy(cur, key, m, l, **dict(ok, **kw))
    for args in ((cur, key[:, :-1], m, l), (cur, key, m[:-1], l), (cur, key, m, l[:, :-1]), (cur, key, m.astype(np.int32), l)):
        with pytest.raises(ValueError):
            ingest.mv_chain_heal_numpy(*args, **ok)
    with pytest.raises(ValueError):
        ingest.mv_chain_heal_numpy(cur, key, m, l, link_stats_row=row[:-1], **ok)


def test_c_abi_refuses_bad_arguments():
    from arseg_amd import _lib

    lib = _lib.load()
    assert _lib.HEAL_NSTATS == oracle.NSTATS and _lib.LINK_NSTATS == oracle.LINK_NSTATS
    cases = oracle.abi_cases()
    assert len(cases) >= 35
    for name, args, want in cases:
        assert lib.arseg_mv_chain_heal_fwd(*args) == want == _lib.ARSEG_EINVAL, name


# ---- the capability ----
@pytest.fixture(scope="module")
def scene1():
    frames = bma.gop_frames()
    pushes = list(oracle.scene1_pushes())
    return frames, oracle.run_chain(pushes, frames, bma.GOP, oracle.CAP["max_ref"]), oracle.run_chain(pushes, frames, bma.GOP, oracle.CAP["max_ref"], oracle.cap_heal(oracle.heal))


def test_scene_1_plain_records_heal_after_every_push(scene1):
    """The panned GOP of the anchor's tests, driven by PLAIN hop records.  Without healing every pixel whose chain passes through the occluder of
    frame 2 keeps its flag to frame 5; with a heal after every push the flags are, from frame 3 on, exactly the pixels of the blocks that leave
    the frame, and no interior pixel is off 4 f (3, -2)."""
    frames, plain, healed = scene1
    H, W = frames[0].shape
    interior = np.zeros((H, W), dtype=bool)
    interior[bma.INTERIOR] = True
    y0, y1, x0, x1 = bma.OCC
    for f in (3, 4, 5):                                                # the plain chain: frame f's pixel (x, y) was at (x + 3 (f - 2), y - 2 (f - 2)) in frame 2
        sx, sy = bma.PAN[0] * (f - 2), bma.PAN[1] * (f - 2)
        assert (plain[1][f][y0 - sy:y1 - sy, x0 - sx:x1 - sx] & 1).all(), f
        assert oracle.off_truth(plain[0][f], f, interior) > 0
    merged, link, stats, rows = healed
    assert np.array_equal(merged[1], plain[0][1]) and np.array_equal(link[1], plain[1][1]) and stats[1][1] == 0        # nothing of frame 1's border is in the keyframe
    assert (link[2][y0:y1, x0:x1] & 1).all() and oracle.off_truth(merged[2], 2, interior) == 32 * 32                    # nothing of the occluder is in the keyframe
    for f in (3, 4, 5):
        leaves = oracle.leaves_frame(f, H, W)
        assert np.array_equal(link[f] & 7 != 0, leaves), f
        assert oracle.off_truth(merged[f], f, interior) == 0 and oracle.off_truth(merged[f], f, ~leaves) == 0, f
        assert (link[f][~leaves] >> 4 <= f).all()
    assert stats[3][1] > 0 and stats[3][3] > 32 * 32
    for f in range(1, bma.GOP):
        assert np.array_equal(rows[f], oracle.recount(link[f])), f


def test_scene_1_numpy_form_runs_like_the_loops(scene1):
    from arseg_amd import ingest

    frames, _, healed = scene1
    got = oracle.run_chain(list(oracle.scene1_pushes()), frames, bma.GOP, oracle.CAP["max_ref"], oracle.cap_heal(ingest.mv_chain_heal_numpy))
    assert np.array_equal(got[0], healed[0]) and np.array_equal(got[1], healed[1])
    assert all(np.array_equal(got[2][f], healed[2][f]) and np.array_equal(got[3][f], healed[3][f]) for f in range(1, bma.GOP))


def test_scene_2_decoder_records_bidirectional_gop_of_20():
    """What anchoring could not take: prediction units off the grid, of mixed sizes, some intra; a B-frame pushed after the frame it looks ahead
    to; 19 frames after the keyframe.  From the frame after the last intra unit whose content is in view, every flagged pixel of the healed
    chain lies in a block that leaves the frame and every pixel outside those blocks is exactly 4 f (3, -2); the plain chain still carries
    thousands of flagged pixels there.  Loops and numpy form agree on the whole GOP."""
    from arseg_amd import ingest

    frames, pushes = oracle.scene2_frames(), list(oracle.scene2_pushes())
    H, W = frames[0].shape
    assert [f for f, _ in pushes].index(5) < [f for f, _ in pushes].index(4) and oracle.GOP2 - 1 > 16
    sizes = {(int(w), int(h)) for _, r in pushes for w, h in r[:, 2:4]}
    assert sizes == {(32, 32), (16, 8), (8, 8)} and any((r[:, 0] % 16 != 0).any() and (r[:, 6] == -1).any() for _, r in pushes)
    plain = oracle.run_chain(pushes, frames, oracle.GOP2, oracle.MAX_REF2, None, True)
    healed = oracle.run_chain(pushes, frames, oracle.GOP2, oracle.MAX_REF2, oracle.cap_heal(oracle.heal), True)
    fast = oracle.run_chain(pushes, frames, oracle.GOP2, oracle.MAX_REF2, oracle.cap_heal(ingest.mv_chain_heal_numpy), True)
    assert np.array_equal(fast[0], healed[0]) and np.array_equal(fast[1], healed[1])
    assert all(np.array_equal(fast[2][f], healed[2][f]) and np.array_equal(fast[3][f], healed[3][f]) for f in range(1, oracle.GOP2))
    merged, link, stats, rows = healed
    for f in range(1, oracle.GOP2):                                    # frames 18 and 19 come after the last such unit; it holds for every frame
        stays = ~oracle.leaves_frame(f, H, W)
        assert stays.any() and not ((link[f] & 7 != 0) & stays).any(), f
        assert oracle.off_truth(merged[f], f, stays) == 0, f
        assert ((plain[1][f] & 3 != 0) & stays).sum() > 1000 and oracle.off_truth(plain[0][f], f, stays) > 1000, f
        assert np.array_equal(rows[f], oracle.recount(link[f])), f
    assert oracle.LAST_INTRA2 == 17 and all(int(stats[f][1]) > 0 for f in (17, 18, 19))                 # frames past 16 are healed, not only inherited
