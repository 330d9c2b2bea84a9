"""The quad-tree split of estimated block motion without a GPU: ingest.block_motion_split_numpy (the host form of
arseg_block_motion_split_fwd) against the loop oracle of tests/block_motion_split_oracle.py, the contract's invariants, what the split buys on
a scene whose dense field is known exactly, the spread of the seeded cases the GPU file compares the kernel on, and the refusals that need no
device.  Integers in, integers out: every comparison is exact."""
import numpy as np
import pytest

import block_motion_split_oracle as oracle


@pytest.mark.parametrize("case", oracle.grid_cases(), ids=oracle.case_id)
def test_numpy_form_equals_the_loop_oracle(case):
    """5 x 7 (only child 0 exists), 16 x 16 (one parent, no neighbours), 37 x 53 (clipped children at both edges) and 48 x 64, with records from
    block_motion_numpy, from block_motion_pyr_numpy(levels=2) and hand-planted, at every r, lam, intra and split_gain."""
    from arseg_amd import ingest

    cur, ref, rec = oracle.grid_case(*case)
    for r in oracle.REFINES:
        for lam in oracle.LAMS:
            found = oracle.grid_found(*case, r, lam)
            for intra in oracle.INTRAS:
                for gain in oracle.GAINS:
                    got = ingest.block_motion_split_numpy(cur, ref, rec, r, lam, intra, gain)
                    assert oracle.same(got, oracle.outputs(found, lam, intra, gain)), (r, lam, intra, gain)


def test_5x7_has_only_child_0():
    cur, ref, rec = oracle.grid_case("full", 5, 7)
    (usable, _, kids), = oracle.grid_found("full", 5, 7, 2, 3)
    assert kids[0][:4] == (0, 0, 7, 5) and kids[1:] == [None, None, None]


@pytest.mark.parametrize("name", sorted(oracle.rank_cases()))
def test_rank_rule_on_constant_and_striped_images(name):
    from arseg_amd import ingest

    cur, ref, rec, r, lam = oracle.rank_cases()[name]
    found = oracle.search(cur, ref, rec, r, lam)
    want = oracle.outputs(found, lam, 255, 0)
    assert oracle.same(ingest.block_motion_split_numpy(cur, ref, rec, r, lam, 255, 0), want)
    winners = {(k[4], k[5]) for _, _, kids in found for k in kids}
    if name.startswith("constant"):
        assert winners == {(0, 0)}                                     # every candidate ties on SAD: rank 0 first
    elif name == "stripes":
        # SAD 0 at dx = 1 mod 4 only; centres (0, 0) and (-3, 0) at r = 3 reach dx in -6 .. 3 and dy in -3 .. 3: the smallest dy, then the smallest dx
        # (column 0 cannot move left: its parents are unusable and its children find dx = 1)
        assert {(k[4], k[5]) for _, _, kids in found[5:7] for k in kids} == {(-3, -3)}        # row 1, columns 1 and 2 of 3 x 4
        assert all(k[6] == 0 for _, _, kids in found for k in kids)
    else:
        inner = [kids for b, (_, _, kids) in enumerate(found) if b % 4 < 3]            # the last column's right children cannot move right
        assert all(k[6] == 0 and k[4] == 1 for kids in inner for k in kids)            # (0, 0) and (1, 1) at r = 1: dx = 1 is the only column at SAD 0


@pytest.mark.parametrize("case", oracle.noise_cases(), ids=oracle.case_id)
def test_seeded_noise_cases_are_spread(case):
    """So that the GPU comparison cannot be vacuous: at the nominal parameters between 10 % and 90 % of a case's parents are split, at least
    one child row is written intra and at least one unusable parent is healed.  The cases with one parent (5 x 7, 16 x 16) cannot meet a share
    and are in the grid above instead."""
    from arseg_amd import ingest

    H, W = case
    cur, ref, rec = oracle.noise_case(H, W)
    n = oracle.NOMINAL
    children, sad, st = oracle.outputs(oracle.noise_found(H, W, n["r"], n["lam"]), n["lam"], n["intra"], n["split_gain"])
    assert 0.1 * len(rec) <= st[0] <= 0.9 * len(rec) and st[3] >= 1 and st[1] >= 1, st
    assert st[0] > st[1] and st[4] > 0                                 # usable parents are split as well
    kinds = rec[:, 6].astype(int), np.abs(rec[:, 4:6].astype(int)).max(axis=1)
    assert (kinds[0] == oracle.INTRA_REF).any() and (kinds[0] == 1).any() and (kinds[1] == 2000).any() and (kinds[1] == 2004).any()
    assert oracle.same(ingest.block_motion_split_numpy(cur, ref, rec, **n), (children, sad, st))


def test_vectors_of_500_are_usable_and_501_are_not():
    H, W = 48, 1200
    rec = oracle.grid_records(H, W, 4 * 500, 0)
    rec[1, 4] = 4 * 501
    rec[2, 4] = 4 * 500 + 2                                            # 500.5 rounds to the even 500
    rec[3, 4] = 4 * 501 - 2                                            # 500.5 again
    rec[4, 4] = 4 * 501 - 1
    use = [oracle.parent_vector(rec, 0, bj, H, W, 0) for bj in range(5)]
    assert [u for _, u in use] == [True, False, True, True, False] and [p[0] for p, _ in use] == [500, 501, 500, 500, 501]


def test_every_row_is_written_and_stats_equal_a_recount():
    from arseg_amd import ingest

    for H, W in oracle.noise_cases():
        cur, ref, rec = oracle.noise_case(H, W)
        for intra, gain in ((20, 32), (0, 0), (255, 65535)):
            children, sad, st = ingest.block_motion_split_numpy(cur, ref, rec, 2, 3, intra, gain)
            assert children.shape == (4 * len(rec), 8) and children.dtype == np.int16 and sad.shape == (4 * len(rec),) and sad.dtype == np.uint32
            assert oracle.recount(children) == (st[0], st[2], st[3], st[5])
            c = children.astype(np.int64)
            zero = ~c.any(axis=1)
            assert (zero | ((c[:, 2] > 0) & (c[:, 3] > 0) & (c[:, 7] == 0) & np.isin(c[:, 6], (0, oracle.INTRA_REF)))).all()
            assert not c[c[:, 6] == oracle.INTRA_REF][:, 4:6].any()


def test_split_gain_65535_with_all_parents_usable_leaves_the_chain_as_it_was():
    from arseg_amd import ingest

    s = oracle.SCENE
    ref, cur = oracle.two_layer_frames(s["H"], s["W"], s["border"])
    rec = ingest.block_motion_numpy(cur, ref, B=16, R=s["R"], lam=s["lam"], intra=255)[0]
    assert (rec[:, 6] == 0).all()
    children, _, st = ingest.block_motion_split_numpy(cur, ref, rec, s["r"], s["lam"], 255, 65535)
    assert not children.any() and not st.any()
    both = np.concatenate([rec, children])
    one = ingest.chain_records_numpy([(1, rec)], s["H"], s["W"], 2, 1, return_link=True)
    two = ingest.chain_records_numpy([(1, both)], s["H"], s["W"], 2, 1, return_link=True)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])


def test_an_intra_parent_with_one_matched_child_is_split_and_the_others_are_written_intra():
    """16 x 16 in a 48 x 48 frame: the parent in the middle is intra; its upper left child is the reference moved by (2, 1), which the left
    neighbour's vector proposes; the other three children are fresh noise."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(oracle.SEED + 50))
    ref = g.integers(0, 256, (48, 48), dtype=np.uint8)
    cur = g.integers(0, 256, (48, 48), dtype=np.uint8)
    cur[16:24, 16:24] = ref[17:25, 18:26]
    rec = oracle.grid_records(48, 48, 8, 4)
    rec[4, 4:7] = (0, 0, oracle.INTRA_REF)
    want = oracle.outputs(oracle.search(cur, ref, rec, 1, 2), 2, 20, 32)
    got = ingest.block_motion_split_numpy(cur, ref, rec, 1, 2, 20, 32)
    assert oracle.same(got, want)
    assert [tuple(row) for row in got[0][16:20]] == [(16, 16, 8, 8, 8, 4, 0, 0), (24, 16, 8, 8, 0, 0, 16, 0), (16, 24, 8, 8, 0, 0, 16, 0), (24, 24, 8, 8, 0, 0, 16, 0)]
    assert got[1][16] == 0 and (got[1][17:20] > 20 * 64).all() and got[2][1] == 1 and got[2][3] >= 3      # the one unusable parent is the one healed
    got0 = ingest.block_motion_split_numpy(cur, ref, rec, 1, 2, 0, 32)           # intra 0: SAD 0 still matches
    assert np.array_equal(got0[0][16:20], got[0][16:20])


def _exact(dense, truth):
    return (dense[..., :2] == truth).all(axis=-1) & (dense[..., 2] == 0)


@pytest.mark.parametrize("axis", ["x", "y"])
def test_two_layer_scene_straddling_parents_are_split_and_carry_the_true_vectors(axis):
    """Two noise canvases that meet mid-block, each sliding along the border: nothing is occluded, so the dense field is known exactly.
    Away from the frame border (there the true vector takes a 16 x 16 parent out of the frame but not all of its children, so the contract
    itself splits parents that lie in one layer) every straddling parent is split, every pixel of its children carries its layer's vector at
    SAD 0, and no parent wholly inside one layer is split.  The last assertion cannot pass without the feature: more pixels carry the true
    vector than with the unsplit B = 16 records."""
    from arseg_amd import ingest

    s = oracle.SCENE
    H, W = (s["H"], s["W"]) if axis == "x" else (s["W"], s["H"])
    ref, cur = oracle.two_layer_frames(H, W, s["border"], axis=axis)
    truth = oracle.true_field(H, W, s["border"], axis=axis)
    by, bx = oracle.grid(H, W)
    for intra in (255, 20):                                            # the straddling parents arrive matched (usable) or intra (healed)
        rec = ingest.block_motion_numpy(cur, ref, B=16, R=s["R"], lam=s["lam"], intra=intra)[0]
        children, sad, st = ingest.block_motion_split_numpy(cur, ref, rec, s["r"], s["lam"], intra, s["split_gain"])
        split = (children.reshape(-1, 4, 8)[..., 2] > 0).any(axis=1).reshape(by, bx)
        dense = ingest.records_to_dense(np.concatenate([rec, children]), H, W)
        exact = _exact(dense, truth)
        straddling = 0
        for bi, bj in oracle.interior_parents(H, W):
            lo = 16 * bj if axis == "x" else 16 * bi
            if lo < s["border"] < lo + 16:
                straddling += 1
                assert split[bi, bj] and exact[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16].all(), (intra, bi, bj)
                assert not sad[4 * (bi * bx + bj):4 * (bi * bx + bj) + 4].any()
            else:
                assert not split[bi, bj], (intra, bi, bj)
        assert straddling == 3
        assert (st[1] > 0) == (intra == 20)
        before = _exact(ingest.records_to_dense(rec, H, W), truth)
        assert exact.sum() > before.sum() and not (before & ~exact).any(), (intra, int(before.sum()), int(exact.sum()))


def test_estimator_refuses_without_a_device():
    from arseg_amd import _lib, ingest

    for kw, word in ((dict(block=8, split_refine=2), "block=16"), (dict(split_refine=2, anchor_refine=1), "anchor_refine"), (dict(split_refine=4), "split_refine"),
                     (dict(split_refine=-1), "split_refine"), (dict(split_refine=1, split_gain=65536), "split_gain"), (dict(split_refine=1, split_gain=-1), "split_gain")):
        with pytest.raises(_lib.ArsegError, match=word):
            ingest.MotionEstimator(64, 96, **kw)
    with pytest.raises(_lib.ArsegError, match="GPU only"):            # the arguments are fine: what is missing is the device
        ingest.MotionEstimator(64, 96, split_refine=2, device="cpu")


def test_numpy_form_refuses():
    from arseg_amd import ingest

    cur, ref, rec = oracle.noise_case(37, 53)
    for kw in (dict(r=0), dict(r=4), dict(lam=256), dict(intra=-1), dict(split_gain=65536), dict(split_gain=-1), dict(ref_index=16)):
        with pytest.raises(ValueError):
            ingest.block_motion_split_numpy(cur, ref, rec, **kw)
    for bad in (lambda: ingest.block_motion_split_numpy(cur, ref[:-1], rec), lambda: ingest.block_motion_split_numpy(cur, ref, rec[:-1]),
                lambda: ingest.block_motion_split_numpy(cur, ref, rec.astype(np.int32))):
        with pytest.raises(ValueError):
            bad()


def test_ref_index_other_than_0():
    """Parents that carry ref_index 3 are the usable ones, those with 0 are not; matched children carry 3."""
    from arseg_amd import ingest

    cur, ref, rec = oracle.noise_case(48, 64)
    rec = rec.copy()
    rec[rec[:, 6] == 0, 6] = 3
    rec[5, 6] = 0
    want = oracle.outputs(oracle.search(cur, ref, rec, 2, 3, 3), 3, 20, 32, 3)
    assert oracle.same(ingest.block_motion_split_numpy(cur, ref, rec, 2, 3, 20, 32, 3), want)
    assert set(np.unique(want[0][:, 6])) == {0, 3, 16} and not oracle.search(cur, ref, rec, 2, 3, 3)[5][0]


def test_c_abi_refuses_bad_arguments():
    """Every ARSEG_EINVAL case of the header through ctypes: validation comes before any launch, so no device is needed."""
    from arseg_amd import _lib

    lib = _lib.load()
    assert _lib.BMS_NSTATS == oracle.NSTATS == 6
    cases = oracle.abi_cases()
    assert len(cases) >= 30
    for name, args, want in cases:
        assert lib.arseg_block_motion_split_fwd(*args) == want == _lib.ARSEG_EINVAL, name
