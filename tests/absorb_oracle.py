"""Oracle of arseg_rle_absorb_fwd (include/arseg_hip.h), written from the contract and independent of run walking: the per-pixel region
ids of links_oracle.region_planes, the borders counted by comparing the id plane with itself shifted by one column and by one row, the
target rule and the value replacement on the pixel plane, and the expected code as rle_oracle.encode of the result.  Independent of
arseg_amd.egress.absorb_numpy (which is tested against it).  Everything is an integer: the tests compare with np.array_equal.  Also the
-1 / -2 / capacity rules (``expected``), the hand-made cases with their answers written out literally, and the inputs both test files use."""
import numpy as np

import links_oracle
import regions_oracle
import rle_oracle

GUARD_I32 = regions_oracle.GUARD_I32
GUARD_I64 = regions_oracle.GUARD_I64
GUARD_WORD = rle_oracle.GUARD_WORD


def borders(reg, R):
    """The region-id plane int64 [H,W] -> int64 [R,R]: border[r, s] = the 4-neighbour pixel pairs (p, q) with p in r and q in s."""
    out = np.zeros((R, R), dtype=np.int64)
    for a, b in ((reg[:, :-1], reg[:, 1:]), (reg[:-1, :], reg[1:, :])):
        differ = a != b
        np.add.at(out, (a[differ], b[differ]), 1)
        np.add.at(out, (b[differ], a[differ]), 1)
    return out


def absorb_plane(plane, min_area, protect=None, connectivity=8):
    """One plane uint8 [H,W] -> a dict: plane (the result, uint8 [H,W]), target int32 [R], n_absorbed, pairs (the distinct (small, stable)
    neighbour pairs), side (links_oracle.region_planes' dict of the input) and row_start / runs (the code of the result)."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    side = links_oracle.region_planes(plane[None], connectivity)[0]
    reg, R = side["reg"], side["R"]
    area = np.bincount(reg.reshape(-1), minlength=R)
    value = np.zeros(R, dtype=np.int64)
    value[reg.reshape(-1)] = plane.reshape(-1)
    stable = area >= min_area
    if protect is not None:
        stable |= np.isin(value, list(protect))
    border = borders(reg, R)
    target = np.where(stable, -1, -2).astype(np.int32)
    pairs = 0
    for r in np.flatnonzero(~stable):
        votes = np.where(stable, border[r], 0)
        pairs += int(np.count_nonzero(votes))
        if votes.max() > 0:
            target[r] = int(np.argmax(votes))                     # the first of equal maxima: the smaller s
    new_value = np.where(target >= 0, value[np.maximum(target, 0)], value)
    result = new_value[reg].astype(np.uint8)
    row_start, runs = rle_oracle.encode(result[None])
    return {"plane": result, "target": target, "n_absorbed": int((target >= 0).sum()), "pairs": pairs, "side": side,
            "row_start": row_start[0], "runs": runs[0]}


def expected(answer, processable, pcap, out_cap, tcap, out_row_start_before, out_runs_before, target_before):
    """What the buffers of one frame hold after the call.  answer: absorb_plane's; processable: the run code did not overflow and
    0 <= n_regions <= rcap; the three buffers as they were -> (n_absorbed, out_row_start, out_runs, target).  Not processable: -1 and
    nothing is touched; more than pcap distinct pairs: -2 and nothing is touched; otherwise out_row_start exact, the words below out_cap
    exact and the rest untouched, target exact below min(R, tcap) and untouched from there on."""
    rs = np.array(out_row_start_before, dtype=np.int32, copy=True)
    words = np.array(out_runs_before, dtype=np.uint32, copy=True)
    target = np.array(target_before, dtype=np.int32, copy=True)
    if not processable:
        return -1, rs, words, target
    if answer["pairs"] > pcap:
        return -2, rs, words, target
    rs[:] = answer["row_start"]
    k = min(len(answer["runs"]), out_cap)
    words[:k] = answer["runs"][:k]
    t = min(len(answer["target"]), tcap)
    target[:t] = answer["target"][:t]
    return answer["n_absorbed"], rs, words, target


def device_inputs(planes, cap=None, rcap=None, connectivity=8, extra=3):
    """The five arrays as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them, made on the host by the oracles: links_oracle's four
    and regions int64 [N,rcap,8] (rcap: default room for every region and ``extra`` more; the rows from min(R, rcap) on hold guards, as do
    all rows of a frame whose run code overflowed)."""
    row_start, runs, n_regions, run_region = links_oracle.device_inputs(planes, cap, connectivity, extra)
    N, H, W = planes.shape
    labelled = regions_oracle.label_planes(planes, connectivity)
    rcap = max(l[0] for l in labelled) + extra if rcap is None else rcap
    regions = np.full((N, rcap, 8), GUARD_I64, dtype=np.int64)
    for n, (R, _, rec) in enumerate(labelled):
        if n_regions[n] >= 0:
            regions[n, :min(R, rcap)] = rec[:rcap]
    return row_start, runs, n_regions, run_region, regions


def median_area(plane, connectivity=8):
    """A min_area that makes about half the regions of the plane small."""
    return max(2, int(np.median(regions_oracle.label_planes(np.ascontiguousarray(plane)[None], connectivity)[0][2][:, 1])) + 1)


def _p(rows):
    return np.array(rows, dtype=np.uint8)


def _w(x, v):
    return (x << 8) | v


_CUT = [[0] * 8, [0, 9, 9, 4, 4, 9, 9, 0], [0] * 8]
_CHECKER = [[1, 2], [3, 4]]
_TALL = [[3, 3, 3, 3, 5, 5, 5], [7] * 7]

# Hand-made cases with the answers written out (not computed by this file): name -> (plane rows, options of absorb_plane, expected rows,
# expected row_start, expected words, target, n_absorbed).  The regions are numbered in the raster order of their first pixel; the answers
# hold for both connectivities of the input labelling (no two regions of one value touch at a corner only).
HAND = {
    # the 0s: region 0 (20 pixels); 9 9: region 1; 4 4: region 2; 9 9: region 3.  min_area 3: the three are small, each borders the 0s
    # along 5 pixel pairs (2 above, 2 below, 1 at the side) and a small neighbour, which does not count
    "specks-into-background": (_CUT, {"min_area": 3}, [[0] * 8] * 3, [0, 1, 2, 3], [_w(0, 0)] * 3, [-1, 0, 0, 0], 3),
    # 4 is protected, hence stable: each 9 9 borders the 0s along 5 pairs and the 4s along 1
    "protected-value-stays": (_CUT, {"min_area": 3, "protect": {4}}, [[0] * 8, [0, 0, 0, 4, 4, 0, 0, 0], [0] * 8], [0, 1, 4, 5],
                              [_w(0, 0), _w(0, 0), _w(3, 4), _w(5, 0), _w(0, 0)], [-1, 0, -1, 0], 2),
    # one pixel pair to either side: the tie goes to the smaller index.  H = 1
    "tie-to-the-smaller-index": ([[1, 1, 1, 5, 2, 2, 2]], {"min_area": 2}, [[1, 1, 1, 1, 2, 2, 2]], [0, 2], [_w(0, 1), _w(4, 2)], [-1, 0, -1], 1),
    # the 1s were two regions (neither is small); the row becomes one run
    "row-merging": ([[1, 1, 5, 1, 1]], {"min_area": 2}, [[1, 1, 1, 1, 1]], [0, 1], [_w(0, 1)], [-1, 0, -1], 1),
    # four single pixels of four values: every neighbour is small, nobody has a target
    "only-small-neighbours": (_CHECKER, {"min_area": 2}, _CHECKER, [0, 2, 4], [_w(0, 1), _w(1, 2), _w(0, 3), _w(1, 4)], [-2, -2, -2, -2], 0),
    "min-area-1-is-the-identity": (_CUT, {"min_area": 1}, _CUT, [0, 1, 6, 7],
                                   [_w(0, 0), _w(0, 0), _w(1, 9), _w(3, 4), _w(5, 9), _w(7, 0), _w(0, 0)], [-1, -1, -1, -1], 0),
    # the 5 5 5 (region 1) touches the 3s (region 0) along 1 pixel pair at its side and the 7s below (region 2) along 3: with the vertical
    # contact counted once per pair of runs the two would tie and the 3s win as the smaller index
    "overlap-length-decides": (_TALL, {"min_area": 4}, [[3, 3, 3, 3, 7, 7, 7], [7] * 7], [0, 2, 3], [_w(0, 3), _w(4, 7), _w(0, 7)],
                               [-1, 2, -1], 1),
    # a speck (region 1: one 8) touching the 6s above along 1 pixel pair, the 2 to its right along 1 and the 2 below along 1: the 2s
    # (region 2, first pixel (1, 1)) have 2 pairs, the 6s 1
    "vertical-and-horizontal-add-up": ([[6, 6, 6], [8, 2, 2], [2, 2, 2]], {"min_area": 2}, [[6, 6, 6], [2, 2, 2], [2, 2, 2]], [0, 1, 2, 3],
                                       [_w(0, 6), _w(0, 2), _w(0, 2)], [-1, 2, -1], 1),
}
HAND_IDS = list(HAND)


def hand_plane(name):
    return _p(HAND[name][0])


# the seeded planes of both test files with the min_area that goes with them: (name, planes uint8 [N,H,W], min_area, protect)
def seeded_cases():
    out = []
    for case in rle_oracle.CASES:
        planes = rle_oracle.build(case)
        out.append((case[0], planes, median_area(planes[0]), None))
    noise = regions_oracle.noise_planes(*regions_oracle.NOISE)
    out.append(("noise", noise, 4, None))
    out.append(("noise-protected", noise, 6, {0, 127}))
    return out
