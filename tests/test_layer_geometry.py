"""The edge-geometry table of tests/layer_geometry.py, on the CPU: its float64 reference is right (independent plain loops, one case per op at
least), the table has teeth (each of seven emulated indexing defects moves some case of its class by more than ten times the bound the GPU
test applies, in every storage), and the GPU sweep cannot pass vacuously (every route label has two cases at least, every class holds
every op it applies to, every threshold has a case on each side, the counts are pinned).  Nothing here launches;
tests/test_gpu_layer_geometry.py does."""
import math

import numpy as np
import pytest
import torch

import layer_geometry as lg

DT = [None, torch.float16, torch.bfloat16]
NAME = {None: "f32", torch.float16: "fp16", torch.bfloat16: "bf16"}
# the ops whose reference a defect changes at all
DEFECT_OPS = {"seg_offset": ("frame_ingest",), "image_straddle": ("head",), "ld_as_c": lg.APPLIES["views"], "floor_bin": ("adaptive_avgpool", "psp_pool_matrix"),
              "no_clamp": ("resize_nhwc", "resize_nchw", "psp_prior_sum"), "band_tail": ("global_reduce",), "sibling_unwritten": ("psp_pool_matrix",)}
# the capped grids that have a case past their cap: (op, route).  Not among them: the run form of the NCHW resize, whose 65536 x 256 runs of
# 8 or 16 outputs are a tensor of 512 MB at the least.
WRAPPED = {("maxpool3x3s2", "maxpool"), ("psp_prior_sum", "prior:px"), ("resize_nhwc", "resize:generic"), ("resize_nchw", "nchw:scalar"), ("resize_nchw", "nchw:x4"),
           ("scale_add", "scale_add"), ("head", "head:g12"), ("head", "head:mfma8"), ("head", "head16:g12"), ("head", "head16:mfma"), ("frame_ingest", "ingest:px"),
           ("frame_u8_to_nhwc4", "u8:px"), ("cast", "cast:to16"), ("cast", "cast:to32")}


# ---------------------------------------------------------------------------------------------------------------- plain loops
def loop_bilinear(x, Hout, Wout, align):
    """x [H, W] -> [Hout, Wout] from the definition (include/arseg_hip.h): the half-pixel source index, its clamp, the four taps"""
    H, W = x.shape
    out = np.zeros((Hout, Wout))

    def src(dst, n_in, n_out):
        s = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) if align else max((dst + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(math.floor(s)), n_in - 1)
        return i0, min(i0 + 1, n_in - 1), s - i0
    for oy in range(Hout):
        y0, y1, ly = src(oy, H, Hout)
        for ox in range(Wout):
            x0, x1, lx = src(ox, W, Wout)
            out[oy, ox] = (1 - ly) * ((1 - lx) * x[y0, x0] + lx * x[y0, x1]) + ly * ((1 - lx) * x[y1, x0] + lx * x[y1, x1])
    return out


def loop_pool(x, oh, ow):
    """x [H, W, C] -> [oh, ow, C]: bin b of an axis covers floor(b H / s) .. ceil((b + 1) H / s)"""
    H, W, C = x.shape
    out = np.zeros((oh, ow, C))
    for by in range(oh):
        for bx in range(ow):
            y0, y1 = by * H // oh, math.ceil((by + 1) * H / oh)
            x0, x1 = bx * W // ow, math.ceil((bx + 1) * W / ow)
            acc = np.zeros(C)
            for y in range(y0, y1):
                for xx in range(x0, x1):
                    acc += x[y, xx]
            out[by, bx] = acc / ((y1 - y0) * (x1 - x0))
    return out


def loop_reference(c, dtype=None):
    o = {k: None if v is None else v.numpy() for k, v in lg.operands(c.id, dtype).items()}
    p, x = c.p, o.get("x")
    if c.op == "maxpool3x3s2":
        N, H, W, C = x.shape
        out = np.full((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), -np.inf)
        for oy in range(out.shape[1]):
            for ox in range(out.shape[2]):
                for dy in range(3):
                    for dx in range(3):
                        iy, ix = 2 * oy - 1 + dy, 2 * ox - 1 + dx
                        if 0 <= iy < H and 0 <= ix < W:
                            out[:, oy, ox] = np.maximum(out[:, oy, ox], x[:, iy, ix])
        return out
    if c.op == "adaptive_avgpool":
        return np.stack([loop_pool(x[n], p["oh"], p["ow"]) for n in range(p["N"])])
    if c.op == "psp_pool_matrix":
        C, n = p["C"], len(p["sizes"])
        out, off = np.zeros((p["N"], sum(s * s for s in p["sizes"]), n * C)), 0
        for i, s in enumerate(p["sizes"]):
            for b in range(p["N"]):
                out[b, off:off + s * s, i * C:(i + 1) * C] = loop_pool(x[b], s, s).reshape(s * s, C)
            off += s * s
        return out
    if c.op == "psp_prior_sum":
        t = o["t"]
        out, off = np.zeros((p["N"], p["H"], p["W"], p["C"])), 0
        for s in p["sizes"]:
            for n in range(p["N"]):
                for ch in range(p["C"]):
                    out[n, :, :, ch] += loop_bilinear(t[n, off:off + s * s, ch].reshape(s, s), p["H"], p["W"], False)
            off += s * s
        return out
    if c.op == "global_reduce":
        out = np.zeros((p["N"], p["C"]))
        for n in range(p["N"]):
            for ch in range(p["C"]):
                px = [x[n, y, xx, ch] for y in range(p["H"]) for xx in range(p["W"])]
                out[n, ch] = sum(px) / len(px) if p["rop"] == "mean" else max(px)
        return out
    if c.op in ("resize_nhwc", "resize_nchw"):
        xc = x.transpose(0, 3, 1, 2) if c.op == "resize_nhwc" else x
        out = np.zeros(xc.shape[:2] + (p["Hout"], p["Wout"]))
        for n in range(xc.shape[0]):
            for ch in range(xc.shape[1]):
                if p["mode"] == "nearest":
                    for oy in range(p["Hout"]):
                        for ox in range(p["Wout"]):
                            out[n, ch, oy, ox] = xc[n, ch, min(oy * p["Hin"] // p["Hout"], p["Hin"] - 1), min(ox * p["Win"] // p["Wout"], p["Win"] - 1)]
                else:
                    out[n, ch] = loop_bilinear(xc[n, ch], p["Hout"], p["Wout"], p["align"])
        return out.transpose(0, 2, 3, 1) if c.op == "resize_nhwc" else out
    if c.op == "scale_add":
        out = np.zeros(x.shape)
        for n in range(p["N"]):
            for ch in range(p["C"]):
                out[n, :, :, ch] = x[n, :, :, ch] * o["scale"][n, 0, 0, ch] + (0.0 if o["full"] is None else o["full"][n, :, :, ch]) \
                    + (0.0 if o["vec"] is None else o["vec"][n, 0, 0, ch])
        return out
    if c.op == "head":
        out = np.zeros((p["N"], p["n_cls"], p["H"], p["W"]))
        for n in range(p["N"]):
            for y in range(p["H"]):
                for xx in range(p["W"]):
                    z = np.array([sum(o["wf"][k, ch] * x[n, y, xx, ch] for ch in range(p["C"])) + o["bf"][k] for k in range(p["n_cls"])])
                    out[n, :, y, xx] = z - (z.max() + math.log(sum(math.exp(v - z.max()) for v in z))) if p["lsm"] else z
        return out
    if c.op in ("frame_ingest", "frame_u8_to_nhwc4"):
        img = o["img"] if c.op == "frame_ingest" else ((o["img"] / 255.0 - np.array(lg.U8_MEAN)) / np.array(lg.U8_STD)).transpose(0, 3, 1, 2)
        out = np.zeros((p["N"], p["h"], p["w"], 3))
        for n in range(p["N"]):
            for ch in range(3):
                out[n, :, :, ch] = loop_bilinear(img[n, ch], p["h"], p["w"], True)
        return out
    if c.op == "to_nhwc":
        out = np.zeros((p["N"], p["H"], p["W"], p["C"]))
        for ch in range(p["C"]):
            out[:, :, :, ch] = x[:, ch]
        return out
    if c.op == "to_nchw_contiguous":
        out = np.zeros((p["N"], p["C"], p["H"], p["W"]))
        for ch in range(p["C"]):
            out[:, ch] = x[:, :, :, ch]
        return out
    assert c.op == "cast"
    return lg.inputs(c.id)["x"].to(dtype).double().numpy()


LOOP_CASES = ["mp_n1", "ap_n1", "ap_n2", "pm_n1", "pr_n1", "gr_s33_mean", "gr_s143_max", "rs_n1", "rs_n2", "rs_n3", "rs_t1a", "rn_n1", "rn_n2", "sa_s33", "hd_s33c12",
              "hd_s143c20", "fi_n1", "fi_same", "fu_n1", "tn_t", "tc_t", "ct_t16", "ct_t32"]


def test_the_plain_loops_cover_every_op():
    assert {lg.BY_ID[i].op for i in LOOP_CASES} == set(lg.OPS)


@pytest.mark.parametrize("case_id", LOOP_CASES)
def test_reference_is_the_plain_loop(case_id):
    c = lg.BY_ID[case_id]
    for dname in c.dtypes:
        dtype = lg.DTYPES[dname]
        want, got = loop_reference(c, dtype), lg.want(case_id, dtype).numpy()
        assert got.shape == want.shape
        assert float(np.abs(got - want).max()) <= 1e-12, dname


def small_cases():
    return [c for c in lg.CASES if c.cls != "grid_wrap"]


def test_explicit_taps_and_bins_without_a_defect_are_the_reference():
    """The forms the defect models are built on are the operation itself when no defect is set: on every case but the grid_wrap ones."""
    for c in small_cases():
        for dname in c.dtypes:
            w = lg.want(c.id, lg.DTYPES[dname])
            e = float((lg.reference(c.id, lg.DTYPES[dname], defect="none") - w).abs().max())
            assert e <= 1e-12 * max(1.0, float(w.abs().max())), (c.id, dname, e)


def detected(defect, dtype, cases):
    """the cases the defect moves by more than 10 x the bound the GPU test applies (an exact op: at all); a NaN is a miss of any bound"""
    hit = []
    for c in cases:
        if NAME[dtype] not in c.dtypes or c.op not in DEFECT_OPS[defect]:
            continue
        w, bad = lg.want(c.id, dtype), lg.reference(c.id, dtype, defect=defect)
        if not bool(lg.within(bad, w, lg.bound(c, dtype, w), factor=10.0).all()):
            hit.append(c.id)
    return hit


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("defect", lg.DEFECTS)
def test_every_emulated_defect_is_detected(defect, dtype):
    hit = detected(defect, dtype, small_cases())
    print(f"{defect} {NAME[dtype]}: {len(hit)} cases move by more than 10 x the bound: {' '.join(hit)}")
    assert hit, defect
    assert any(lg.BY_ID[i].cls == lg.DEFECT_CLASS[defect] for i in hit), (defect, lg.DEFECT_CLASS[defect])


def test_seg_offset_needs_a_second_segment_and_ld_as_c_needs_the_guards():
    """Why the table holds staged rows of two and three segments, and why the GPU test puts NaN around a view: the first segment of a staged
    row is right under seg_offset, so no single-segment case moves; and a view whose neighbours hold the operand's own kind of numbers
    gives plausible values under ld_as_c, which only the value check can then catch."""
    for dtype in DT:
        hit = detected("seg_offset", dtype, small_cases())
        assert hit and all(lg.BY_ID[i].p["w"] > 256 for i in hit), hit
        multi = [c.id for c in small_cases() if c.op == "frame_ingest" and lg.route(c, NAME[dtype])[0] in ("ingest:rows2", "ingest:rows3")]
        assert sorted(hit) == sorted(multi) and len(multi) >= 5
    x = lg.operands("rs_v")["x"]
    assert bool(torch.isnan(lg.misread_as_dense(x)).any()) and torch.equal(lg.misread_as_dense(x, 0, 0), x)


# ---------------------------------------------------------------------------------------------------------------- the sweep cannot pass vacuously
def tally():
    """route label -> (case, storage) pairs that reach it; route label -> cases"""
    pairs, cases = {}, {}
    for c in lg.CASES:
        for dname in c.dtypes:
            for label in lg.route(c, dname):
                pairs[label] = pairs.get(label, 0) + 1
                cases.setdefault(label, set()).add(c.id)
    return pairs, cases


def test_every_route_has_two_cases_and_the_counts_are_pinned():
    pairs, cases = tally()
    for label in sorted(pairs):
        print(f"{label:20s} {pairs[label]:3d} launches on {len(cases[label]):3d} cases")
    assert set(pairs) == set(lg.ALL_ROUTES), set(pairs) ^ set(lg.ALL_ROUTES)
    assert all(len(v) >= 2 for v in cases.values()), {k: sorted(v) for k, v in cases.items() if len(v) < 2}
    assert pairs == lg.ROUTE_COUNTS, {k: (pairs.get(k), lg.ROUTE_COUNTS.get(k)) for k in set(pairs) | set(lg.ROUTE_COUNTS) if pairs.get(k) != lg.ROUTE_COUNTS.get(k)}


def test_every_class_holds_every_op_it_applies_to():
    assert {c.cls for c in lg.CASES} == set(lg.CLASSES) and {c.op for c in lg.CASES} == set(lg.OPS)
    for cls in lg.CLASSES:
        assert {c.op for c in lg.of_class(cls)} == set(lg.APPLIES[cls]), cls
        for op in lg.APPLIES[cls]:
            # ... in every storage the op has
            have = {d for c in lg.of_class(cls, op) for d in c.dtypes}
            full = {d for c in lg.CASES if c.op == op for d in c.dtypes}
            assert have == full, (cls, op, have)
    for c in lg.CASES:
        assert c.dtypes in (lg.ALL, lg.F32, lg.D16), c.id


def test_every_threshold_has_a_case_on_each_side():
    for dname, a, ra, b, rb in lg.THRESHOLDS:
        assert ra != rb
        assert ra in lg.route(lg.BY_ID[a], dname) and rb not in lg.route(lg.BY_ID[a], dname), (dname, a, lg.route(lg.BY_ID[a], dname))
        assert rb in lg.route(lg.BY_ID[b], dname) and (ra not in lg.route(lg.BY_ID[b], dname) or lg.BY_ID[b].op == "psp_pool_matrix"), (dname, b, lg.route(lg.BY_ID[b], dname))
    # the predicates at their very edges, as csrc/layers.hip states them
    p = lambda i: lg.BY_ID[i].p      # noqa: E731
    assert [p(i)["N"] * -(-p(i)["C"] // 16) for i in ("gr_w255_max", "gr_w256_max", "gr_b63_mean", "gr_b64_mean")] == [255, 256, 63, 64]
    assert [p(i)["H"] * p(i)["W"] for i in ("gr_hw2047_mean", "gr_hw2048_mean", "gr_b63_mean")] == [2047, 2048, 45 * 47]
    assert lg.reduce_parts(lg.BY_ID["gr_b63_mean"], "f32") == 8 and (45 * 47) % 8          # uneven bands
    assert lg.reduce_parts(lg.BY_ID["gr_c512_mean"], "fp16") == 1 and lg.reduce_parts(lg.BY_ID["gr_c264_mean"], "bf16") > 1
    assert [p(i)["oh"] * p(i)["ow"] * -(-p(i)["C"] // 16) * p(i)["N"] for i in ("ap_g255", "ap_g256")] == [255, 256]
    assert [p(i)["N"] * p(i)["H"] * (p(i)["C"] // 4) for i in ("pr_px", "pr_rw", "pr_w1", "pr_small")] == [48640, 49152, 49152, 49152]
    assert p("pr_small")["H"] < max(p("pr_small")["sizes"]) and p("pr_w1")["W"] == 1
    assert {p(c.id)["C"] for c in lg.of_class("thresholds", "head") if c.dtypes == lg.F32} == {8, 64, 72, 128, 136, 12, 512, 20}
    assert {p(c.id)["n_cls"] for c in lg.of_class("thresholds", "head") if c.dtypes == lg.F32} >= {1, 12, 13, 19, 20, 32}
    assert {p(c.id)["C"] for c in lg.of_class("thresholds", "head") if c.dtypes == lg.D16} == {64, 128, 512, 576, 24}
    span = lambda i: 255.0 * (p(i)["W"] - 1) / (p(i)["w"] - 1) + 8.0      # noqa: E731
    assert 1050.0 < span("fi_span_u") <= 1056.0 < span("fi_span_o") < 1062.0
    assert {p(c.id)["w"] for c in lg.of_class("thresholds", "frame_ingest")} >= {255, 256, 257, 513}
    # the four block-row forms, the straddling tiles of the wide heads
    forms = {label for c in lg.of_class("thresholds", "psp_pool_matrix") for label in lg.route(c, "f32")}
    assert forms == {"psp:onepass", "blockrow:c64t1024", "blockrow:c64t256", "blockrow:c16t1024", "blockrow:c16t256"}
    for c in lg.of_class("image_straddle"):
        hw = p(c.id).get("Hout", p(c.id).get("H", 0)) * p(c.id).get("Wout", p(c.id).get("W", 0))
        assert p(c.id)["N"] * (p(c.id)["C"] if c.op == "resize_nchw" else 1) >= 3, c.id
        if c.op == "head":
            assert hw in (33, 143, 257) and math.gcd(hw, 256) == 1, c.id
    heads = {(d, label) for c in lg.of_class("image_straddle", "head") for d in c.dtypes for label in lg.route(c, d)}
    assert heads >= {("f32", f"head:{k}") for k in ("mfma8", "mfma16", "g12", "g19", "g32")} | {(d, f"head16:{k}") for d in lg.D16 for k in ("mfma", "g12", "g19", "g32")}
    assert {p(c.id)["C"] for c in lg.of_class("image_straddle", "head") if "head16:mfma" in lg.route(c, "fp16" if "fp16" in c.dtypes else "f32")} >= {128, 192, 512}


def test_sizes_and_grid_caps():
    """No tensor above 64 MiB (but the two grids whose second trip starts exactly there: lg.OVERSIZE); a grid_wrap case is past its cap by 1 % at
    the most, no other case is past one; every capped grid but the NCHW run form has a case past its cap."""
    wrapped = set()
    for c in lg.CASES:
        for dname in c.dtypes:
            assert lg.tensor_bytes(c, dname) <= lg.MAX_TENSOR_BYTES + lg.OVERSIZE.get(c.id, 0), (c.id, dname, lg.tensor_bytes(c, dname))
            gi = lg.grid_items(c, dname)
            if c.cls == "grid_wrap":
                assert gi is not None and gi[1] < gi[0] <= 1.01 * gi[1], (c.id, dname, gi)
                wrapped.add((c.op, lg.route(c, dname)[0]))
            else:
                assert gi is None or gi[0] <= gi[1], (c.id, dname, gi)
                assert lg.tensor_bytes(c, dname) <= 16 * lg.MIB, c.id
    assert wrapped == WRAPPED, wrapped ^ WRAPPED
    assert all(lg.BY_ID[i].cls == "grid_wrap" for i in lg.OVERSIZE)
