"""Every plan and route that computes in split fp16 (ARSEG_MATH_F16X3), held to fp32-grade error against fp64: e = max|got - want| / max|want|
<= margin x e32, e32 the error of the plain float32 loop on the same inputs (tests/split_accuracy.py; tests/test_split_accuracy.py proves on the CPU
that this bound passes the correct arithmetic and fails a low half lost in one K step).  The table: every tile_cfg 1..23 and the split-K
pairs of arseg_conv2d_fwd, the Winograd route on both of its GEMMs, the LDS-DMA GEMM with fp32 and split-row output, the tap decomposition,
up_3's persistent kernel, the folded PSP bottleneck -- and ids 0..12 of the f32 back end, which is the fp32 arithmetic itself.  Each case is
drawn under both distributions; a launch is accepted exactly when the device-free plan query accepts it; outputs start as NaN.

Every test prints the figures it asserts (route, e, e / e32, margin); ``pytest -s`` shows them."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

import split_accuracy as sa

pytestmark = pytest.mark.gpu

CONV = [(c.id, d) for c in sa.conv_cases() for d in sa.DISTS]
WINO = [(c.id, d) for c in sa.CASES if sa.has_wino(c) for d in sa.DISTS]
ONE_BY_ONE = [(c.id, d) for c in sa.conv_cases() if c.k == 1 and c.Cin % 32 == 0 for d in sa.DISTS]
UP2 = [(c.id, d) for c in sa.CASES if c.up2 for d in sa.DISTS]
PSP = [(c.id, d) for c in sa.CASES if c.psp for d in sa.DISTS]
WINO_PLANS = (7, 100, 101, 102, 103, 104, 105, 106)
REQUIRED = ([f"tile:{cfg}" for cfg in range(1, 24)] + [f"splitk:{cfg},{sk}" for cfg, sk in sa.SPLIT_K_PAIRS] + [f"f32:{cfg}" for cfg in range(13)]
            + [f"wino:{p}" for p in WINO_PLANS] + [f"wino_up2:{p}" for p in WINO_PLANS] + ["x3", "x3split", "taps", "tapssplit", "taps_f32in", "up2_c64:0", "up2_c64:3",
                                                                                             "psp", "pspsplit"])

Row = collections.namedtuple("Row", "route e e32 margin problem")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib, ops

    _lib.load()
    prev = ops.set_conv_math("f16x3")
    assert ops.gemm_x3_enabled()
    yield torch.device("cuda:0")
    ops.set_conv_math(prev)


@functools.lru_cache(maxsize=None)
def on_device(case_id, dist):
    """(PackedConv, x NHWC with the channels padded to 4, residual NHWC or None) of a case on the device"""
    from arseg_amd import _lib
    from arseg_amd.packing import PackedConv

    c, ins, dev = sa.BY_ID[case_id], sa.inputs(case_id, dist), torch.device("cuda:0")
    act = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU, "sigmoid": _lib.ACT_SIGMOID}[c.act]
    pc = PackedConv(ins["w"], ins["b"], ins["bn"], c.stride, c.pad, c.dil, act, sa.SLOPE if c.act == "prelu" else 0.0, dev)
    x = F.pad(ins["x"].permute(0, 2, 3, 1), (0, -c.Cin % 4)).contiguous().to(dev)
    res = None if ins["res"] is None else ins["res"].permute(0, 2, 3, 1).contiguous().to(dev)
    return pc, x, res


class Table:
    """The rows of one (group, case, distribution): what ran, its error and bound, and what went wrong."""

    def __init__(self, case_id, dist, e32=None):
        self.case_id, self.dist, self.rows = case_id, dist, []
        self.want, self.e32 = sa.yardstick(case_id, dist)
        if e32 is not None:
            self.e32 = e32

    def nan_out(self):
        c = sa.BY_ID[self.case_id]
        return torch.full((c.N,) + sa.out_hw(c) + (c.Cout,), float("nan"), device="cuda:0")

    def add(self, route, kind, got):
        if isinstance(got, str):
            self.rows.append(Row(route, float("nan"), self.e32, 0.0, got))
            return
        m, e = sa.margin(self.case_id, kind), sa.stat(got, self.want)
        self.rows.append(Row(route, e, self.e32, m, "" if e <= m * self.e32 else f"e = {e:.3g} > {m:g} x e32 = {m * self.e32:.3g}"))

    def launch(self, route, kind, expected, fn):
        """fn() -> the result; it must be accepted exactly when ``expected`` says so."""
        from arseg_amd import _lib

        try:
            got = fn()
        except _lib.ArsegError as err:
            if expected:
                self.add(route, kind, f"refused although the plan query accepts it: {err}")
            return
        if not expected:
            self.add(route, kind, "accepted although the plan query refuses it")
        self.add(route, kind, got)


def settle(tab):
    """Print the rows, return them; the caller asserts."""
    for r in tab.rows:
        print(f"{tab.case_id:4s} {tab.dist:6s} {r.route:14s} e = {r.e:.3g} = {r.e / r.e32:5.2f} x e32 ({r.e32:.3g}), margin {r.margin:g} {r.problem}")
    return tab.rows


def failures(rows):
    return [f"{r.route}: {r.problem}" for r in rows if r.problem]


# ---------------------------------------------------------------------------------------------- the groups, each computed once
@functools.lru_cache(maxsize=None)
def tiles(case_id, dist):
    """every tile_cfg 1..23 with split_k 1 and the split-K pairs of arseg_conv2d_fwd under f16x3"""
    from arseg_amd import _lib, ops

    c, tab = sa.BY_ID[case_id], Table(case_id, dist)
    pc, x, res = on_device(case_id, dist)
    for cfg, sk in [(cfg, 1) for cfg in range(1, 24)] + list(sa.SPLIT_K_PAIRS):
        out = tab.nan_out()
        tab.launch(f"tile:{cfg}" if sk == 1 else f"splitk:{cfg},{sk}", "tile" if sk == 1 else "splitk", sa.accepted(case_id, cfg, sk, _lib.MATH_F16X3),
                   lambda: ops.conv2d(x, pc, residual=res, out=out, tile_cfg=cfg, split_k=sk, up2=c.up2))
    return settle(tab)


@functools.lru_cache(maxsize=None)
def f32_plans(case_id, dist):
    """ids 0..12 under the f32 back end (0: the library's heuristic, the tuner off)"""
    from arseg_amd import _lib, ops

    c, tab = sa.BY_ID[case_id], Table(case_id, dist)
    pc, x, res = on_device(case_id, dist)
    prev, prev_cfg = ops.set_conv_math("f32"), ops.configure(conv_autotune=False)
    try:
        for cfg in range(13):
            out = tab.nan_out()
            tab.launch(f"f32:{cfg}", "f32", sa.accepted(case_id, cfg, 0 if cfg == 0 else 1, _lib.MATH_F32),
                       lambda: ops.conv2d(x, pc, residual=res, out=out, tile_cfg=cfg, split_k=0 if cfg == 0 else 1, up2=c.up2))
    finally:
        ops.configure(**prev_cfg)
        ops.set_conv_math(prev)
    return settle(tab)


@functools.lru_cache(maxsize=None)
def winograd(case_id, dist):
    """ops._conv_wino with its batched GEMM pinned to the implicit-GEMM plan 7 and to the LDS-DMA tiles 100..106, against the float32 Winograd's e32"""
    from arseg_amd import _lib, ops

    c, tab = sa.BY_ID[case_id], Table(case_id, dist, sa.wino_yardstick(case_id, dist))
    pc, x, res = on_device(case_id, dist)
    assert pc.wino_u is not None
    H, W = (2 * c.H, 2 * c.W) if c.up2 else (c.H, c.W)
    key = ("wino_gemm", 0, _lib.load().arseg_wino43_tiles(c.N, H, W, c.dil), pc.cin_pad, c.Cout, _lib.MATH_F16X3)
    saved = ops._conv_plans.get(key)
    try:
        for plan in WINO_PLANS:
            ops._conv_plans[key] = plan
            out = tab.nan_out()
            ops._conv_wino(x, pc, res, out, c.N, H, W, up2=c.up2)
            tab.add(("wino_up2:" if c.up2 else "wino:") + str(plan), "wino", out)
    finally:
        if saved is None:
            ops._conv_plans.pop(key, None)
        else:
            ops._conv_plans[key] = saved
    return settle(tab)


@functools.lru_cache(maxsize=None)
def gemm_x3(case_id, dist):
    """ops._conv1x1_x3, every tile shape: fp32 output, and split-row output read back through SplitRows.float()"""
    from arseg_amd import ops

    c, tab = sa.BY_ID[case_id], Table(case_id, dist)
    pc, x, res = on_device(case_id, dist)
    for cfg in range(7):
        out = tab.nan_out()
        ops._conv1x1_x3(x, pc, res, out, cfg=cfg)
        tab.add(f"x3/{cfg}", "x3", out)
        if c.Cout % 32 == 0:
            rows = ops._conv1x1_x3(x, pc, res, None, out_split=True, cfg=cfg)
            tab.add(f"x3split/{cfg}", "x3split", rows.float() if isinstance(rows, ops.SplitRows) else "out_split returned no SplitRows")
    return settle(tab)


@functools.lru_cache(maxsize=None)
def taps(case_id, dist):
    """the tap decomposition of the conv after a x2 upsample: from split rows (with and without split-row output) and from fp32 input"""
    from arseg_amd import ops

    tab = Table(case_id, dist)
    pc, x, _ = on_device(case_id, dist)
    xs = ops.split_rows(x)
    got = ops.conv2d(xs, pc, up2=True)
    tab.add("taps", "taps", got if isinstance(got, torch.Tensor) else "no fp32 tensor")
    got = ops.conv2d(xs, pc, up2=True, out_split=True)
    tab.add("tapssplit", "tapssplit", got.float() if isinstance(got, ops.SplitRows) else "out_split returned no SplitRows")
    out = tab.nan_out()
    ops._conv_up2_taps(x, pc, out)
    tab.add("taps_f32in", "taps", out)
    return settle(tab)


@functools.lru_cache(maxsize=None)
def up2_c64(case_id, dist):
    from arseg_amd import ops

    tab = Table(case_id, dist)
    pc, x, _ = on_device(case_id, dist)
    for max_wgs in (0, 3):
        out = tab.nan_out()
        ops.conv_up2_c64(x, pc, out=out, max_wgs=max_wgs)
        tab.add(f"up2_c64:{max_wgs}", "up2_c64", out)
    return settle(tab)


@functools.lru_cache(maxsize=None)
def psp(case_id, dist):
    """ops.psp_bottleneck_x3 against the fp64 prior sum + 1x1 conv + ReLU"""
    from arseg_amd import ops

    tab = Table(case_id, dist)
    pc, x, _ = on_device(case_id, dist)
    t = sa.inputs(case_id, dist)["t"].to(x.device)
    assert ops.psp_x3_foldable(pc)
    got = ops.psp_bottleneck_x3(x, t, pc, sa.PSP_SIZES, out_split=False)
    tab.add("psp", "psp", got)
    got = ops.psp_bottleneck_x3(x, t, pc, sa.PSP_SIZES)
    tab.add("pspsplit", "psp", got.float() if isinstance(got, ops.SplitRows) else "no SplitRows")
    return settle(tab)


GROUPS = [(tiles, CONV), (f32_plans, CONV), (winograd, WINO), (gemm_x3, ONE_BY_ONE), (taps, UP2), (up2_c64, [("i64", d) for d in sa.DISTS]), (psp, PSP)]


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("case_id,dist", CONV)
def test_every_tile_plan_and_split_k_pair(dev, case_id, dist):
    assert not failures(tiles(case_id, dist))


@pytest.mark.parametrize("case_id,dist", CONV)
def test_f32_back_end_is_the_fp32_arithmetic(dev, case_id, dist):
    assert not failures(f32_plans(case_id, dist))


@pytest.mark.parametrize("case_id,dist", WINO)
def test_winograd_route_on_both_gemms(dev, case_id, dist):
    assert not failures(winograd(case_id, dist))


@pytest.mark.parametrize("case_id,dist", ONE_BY_ONE)
def test_lds_dma_gemm_fp32_and_split_row_output(dev, case_id, dist):
    assert not failures(gemm_x3(case_id, dist))


@pytest.mark.parametrize("case_id,dist", UP2)
def test_tap_decomposition(dev, case_id, dist):
    assert not failures(taps(case_id, dist))


@pytest.mark.parametrize("dist", sa.DISTS)
def test_up2_c64_persistent_kernel(dev, dist):
    assert not failures(up2_c64("i64", dist))


@pytest.mark.parametrize("case_id,dist", PSP)
def test_folded_psp_bottleneck(dev, case_id, dist):
    assert not failures(psp(case_id, dist))


def test_every_plan_and_route_ran_under_each_distribution(dev):
    """Coverage does not erode: every id 1..23, every split-K pair, ids 0..12 of the f32 back end and every route above produced a checked
    result on at least one case under each distribution (the groups are computed once; run alone, this test computes them)."""
    ran = {d: set() for d in sa.DISTS}
    for group, params in GROUPS:
        for case_id, dist in params:
            ran[dist] |= {r.route.split("/")[0] for r in group(case_id, dist) if r.margin > 0}
    for d in sa.DISTS:
        missing = [r for r in REQUIRED if r not in ran[d]]
        assert not missing, (d, missing)
