"""The edge-geometry table of tests/conv_geometry.py, on the CPU: its float64 reference is right (an independent plain loop), the table has
teeth (each of five emulated indexing defects moves some case by more than ten times the bound the GPU test applies), and the GPU sweep
cannot pass vacuously (from the library's device-free plan query alone: every plan id is accepted in every class it can apply in, every
class sees refusals, no case is refused by everything).  Nothing here launches; tests/test_gpu_conv_geometry.py does."""
import numpy as np
import pytest
import torch

import conv_geometry as cg

# (accepted, refused) pinned (case, plan) pairs per class and engine, from the query: a change of the plan table or of the case table shows up here
COUNTS = {
    "tiny": {"f32": (228, 144), "f16x3": (314, 58), "fp16": (131, 73), "bf16": (131, 73)},
    "dil_gt_map": {"f32": (95, 60), "f16x3": (123, 32), "fp16": (48, 37), "bf16": (48, 37)},
    "thresholds": {"f32": (285, 180), "f16x3": (418, 47), "fp16": (201, 54), "bf16": (201, 54)},
    "m_edges": {"f32": (342, 216), "f16x3": (458, 100), "fp16": (190, 116), "bf16": (190, 116)},
    "many_images": {"f32": (95, 60), "f16x3": (128, 27), "fp16": (52, 33), "bf16": (52, 33)},
    "parity": {"f32": (190, 120), "f16x3": (230, 80), "fp16": (82, 88), "bf16": (82, 88)},
    "padding": {"f32": (76, 48), "f16x3": (92, 32), "fp16": (32, 36), "bf16": (32, 36)},
    "nonsquare": {"f32": (76, 48), "f16x3": (92, 32), "fp16": (32, 36), "bf16": (32, 36)},
    "narrow_k": {"f32": (133, 84), "f16x3": (161, 56), "fp16": (56, 63), "bf16": (56, 63)},
}


def loop_reference(c, dtype=None):
    """The operation as plain numpy loops in float64, written from the definition (include/arseg_hip.h): out[n, oy, ox, co] = act(scale[co] *
    sum_{r, s, ci} in[n, oy * stride - pad + r * dil, ox * stride - pad + s * dil, ci] * w[co, ci, r, s] + bias[co] + residual)."""
    assert not c.up2
    ins = cg.inputs(c.id)
    x, w, res = (None if v is None else v.numpy() for v in cg.operands(c.id, dtype))
    Ho = (c.H + 2 * c.pad - c.dil * (c.R - 1) - 1) // c.stride + 1
    Wo = (c.W + 2 * c.pad - c.dil * (c.S - 1) - 1) // c.stride + 1
    out = np.zeros((c.N, Ho, Wo, c.Cout))
    for n in range(c.N):
        for oy in range(Ho):
            for ox in range(Wo):
                acc = np.zeros(c.Cout)
                for r in range(c.R):
                    for s in range(c.S):
                        iy, ix = oy * c.stride - c.pad + r * c.dil, ox * c.stride - c.pad + s * c.dil
                        if 0 <= iy < c.H and 0 <= ix < c.W:
                            acc += w[:, :, r, s] @ x[n, iy, ix]
                out[n, oy, ox] = acc
    if ins["bn"] is not None:
        gamma, beta, mean, var = (v.double().numpy() for v in ins["bn"])
        b = ins["b"].double().numpy() if ins["b"] is not None else 0.0
        out = (out + b - mean) / np.sqrt(var + cg.BN_EPS) * gamma + beta
    elif ins["b"] is not None:
        out = out + ins["b"].double().numpy()
    if res is not None:
        out = out + res
    if c.act == "relu":
        out = np.maximum(out, 0.0)
    elif c.act == "prelu":
        out = np.where(out >= 0, out, cg.SLOPE * out)
    return out


@pytest.mark.parametrize("case_id", ["z5x9", "z2big", "d35", "q1x3s2"])          # pad 0, pad > same, dilation > map, a 1x3 kernel with stride 2
def test_reference_is_the_plain_loop(case_id):
    c = cg.BY_ID[case_id]
    want = loop_reference(c)
    got = cg.want(case_id).numpy()
    assert got.shape == want.shape == (c.N,) + cg.out_hw(c) + (c.Cout,)
    assert float(np.abs(got - want).max()) <= 1e-12
    got16 = cg.want(case_id, torch.bfloat16).numpy()
    assert float(np.abs(got16 - loop_reference(c, torch.bfloat16)).max()) <= 1e-12


def test_tap_loop_without_a_defect_is_the_reference():
    """The loop the defect models are built on is the conv itself when no defect is set: on every case."""
    for c in cg.CASES:
        e = float((cg.reference(c.id, defect="none") - cg.want(c.id)).abs().max())
        assert e <= 1e-12, (c.id, e)


def test_every_class_has_a_full_epilogue_case():
    for cls in cg.CLASSES:
        assert any(c.res and c.bn and c.bias and c.act == "prelu" for c in cg.of_class(cls)), cls
    assert {c.cls for c in cg.CASES} == set(cg.CLASSES)
    for c in cg.CASES:
        assert c.N * cg.out_hw(c)[0] * cg.out_hw(c)[1] <= 4096, c.id
        # the two kernels that take no residual (the stem kernel, up_3's persistent kernel: include/arseg_hip.h) meet none here, so that the
        # query, which is not told about a residual, is the whole verdict of every launch
        assert not (c.res and (cg.is_stem(c) or (c.up2 and c.Cin == 64 and c.Cout == 64))), c.id


def detected(defect, dtype, cases, guard=float("nan")):
    """the cases the defect moves by more than 10 x the bound the GPU test applies (fp32: TOL absolute; 16-bit: tol16 elementwise)"""
    hit = []
    for c in cases:
        w, bad = cg.want(c.id, dtype), cg.reference(c.id, dtype, defect=defect, guard=guard)
        bound = 10 * (cg.TOL if dtype is None else cg.tol16(w, dtype))
        if not bool(((bad - w).abs() <= bound).all()):          # (a NaN from a guard image is a miss of any bound)
            hit.append(c.id)
    return hit


@pytest.mark.parametrize("dtype", [None, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("defect", cg.DEFECTS)
def test_every_emulated_defect_is_detected(defect, dtype):
    hit = detected(defect, dtype, cg.CASES)
    print(f"{defect}: {len(hit)} of {len(cg.CASES)} cases move by more than 10 x the bound: {' '.join(hit)}")
    assert hit, defect
    expected_class = {"clamp_pad": "tiny", "batch_wrap": "many_images", "floor_out": "parity", "rs_swap": "narrow_k", "phase_drop": "dil_gt_map"}[defect]
    assert any(cg.BY_ID[i].cls == expected_class for i in hit), (defect, expected_class)


def test_batch_wrap_needs_the_guard_images():
    """Why the GPU test puts a NaN image before and after the batch: on a single image a read of "row -1" leaves the tensor, and where the
    allocator left zeros there the result is the right one.  With zeros outside, no N = 1 case moves at all; with NaN guards every N = 1
    case whose kernel reaches above or below the map does."""
    single = [c for c in cg.CASES if c.N == 1]
    reaches = [c.id for c in single if any(oy * c.stride - c.pad + r * c.dil in (-1, cg.conv_hw(c)[0]) for oy in range(cg.out_hw(c)[0]) for r in range(c.R))]
    assert len(reaches) >= 20
    assert detected("batch_wrap", None, single, guard=0.0) == []
    for c in single:
        assert torch.equal(cg.reference(c.id, defect="batch_wrap", guard=0.0), cg.reference(c.id, defect="none")), c.id
    assert detected("batch_wrap", None, single) == reaches


def tally(name, cls):
    acc = ref = 0
    for c in cg.of_class(cls):
        for cfg, sk in cg.plans(name):
            if cg.verdict(c, name, cfg, sk)[0]:
                acc += 1
            else:
                ref += 1
    return acc, ref


def test_coverage_floor():
    """From the query alone.  Every id of both engines (and every split-K pair) is accepted on at least one case of every class in which its
    kind can apply (cg.applies); every class has refused (case, plan) pairs on every engine -- at the least the stem kernel and up_3's kernel
    off their shapes; no case is refused by every plan; and no plan is accepted in a class it is said not to apply in."""
    for name in cg.ENGINES:
        for cls in cg.CLASSES:
            cases = cg.of_class(cls)
            for cfg, sk in cg.plans(name):
                n_ok = sum(cg.verdict(c, name, cfg, sk)[0] for c in cases)
                assert (n_ok > 0) == cg.applies(name, cfg, sk, cls), (name, cls, cfg, sk, n_ok)
            acc, ref = tally(name, cls)
            print(f"{cls:12s} {name:6s} accepted {acc:4d} refused {ref:4d}")
            assert ref > 0, (name, cls)
            assert (acc, ref) == COUNTS[cls][name], (name, cls, (acc, ref))
        for c in cg.CASES:
            assert any(cg.verdict(c, name, cfg, sk)[0] for cfg, sk in cg.plans(name)), (name, c.id)


def test_plan_tables_are_walked_not_assumed():
    from arseg_amd import _lib

    assert len(cg.table_ids(_lib.CONV_ENGINE_F32)) >= 24 and len(cg.table_ids(_lib.CONV_ENGINE_16)) >= 14
    kinds32 = {_lib.conv_plan_row(_lib.CONV_ENGINE_F32, i).kind for i in cg.table_ids(_lib.CONV_ENGINE_F32)}
    kinds16 = {_lib.conv_plan_row(_lib.CONV_ENGINE_16, i).kind for i in cg.table_ids(_lib.CONV_ENGINE_16)}
    assert kinds32 == {_lib.PLAN_AUTO, _lib.PLAN_TILE, _lib.PLAN_TILE_WIDE, _lib.PLAN_PATCH, _lib.PLAN_UP2_C64}
    assert kinds16 == {_lib.PLAN_AUTO, _lib.PLAN_TILE, _lib.PLAN_PATCH, _lib.PLAN_STEM}


def test_every_route_is_eligible_somewhere():
    """... and the routes above the engines, whose eligibility is a host condition: each is eligible in the classes its shape occurs in."""
    where = {}
    for name in cg.ENGINES:
        for c in cg.CASES:
            for label in cg.routes(c, name):
                where.setdefault((name, label.split(":")[0]), set()).add(c.cls)
    assert where[("f32", "wino")] == where[("f16x3", "wino")] == set(cg.PATCH_CLASSES)
    assert where[("f16x3", "x3")] == {"m_edges", "many_images"}          # (Cin % 32 == 0: narrow_k's 1x1 convs have 4, 36 and 100 channels)
    assert where[("f32", "taps")] == where[("f16x3", "taps")] == {"tiny", "many_images"}
    assert where[("f16x3", "up2_c64")] == set(cg.UP2_C64_CLASSES)
    assert where[("fp16", "rows16")] == where[("bf16", "rows16")] == {"m_edges", "many_images"}


def test_query_output_size_is_the_reference_size():
    for name in cg.ENGINES:
        for c in cg.CASES:
            for cfg, sk in cg.plans(name):
                ok, info = cg.verdict(c, name, cfg, sk)
                if ok:
                    assert (info.Ho, info.Wo) == cg.out_hw(c) == tuple(cg.want(c.id).shape[1:3]), (name, c.id, cfg, sk)
