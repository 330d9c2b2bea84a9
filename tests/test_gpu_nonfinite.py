"""NaN / Inf propagation of every kernel ("Non-finite values"): one table of ops, each held by the dependency probe of
tests/nonfinite.py to

  (a) a non-finite result wherever the output depends on the planted element,
  (b) a finite result within the op's own tolerance everywhere outside the allowed set A (= T, the outputs torch's fp64 reference makes
      non-finite; larger only where the entry says why),
  (c) a NaN stays a NaN (never an infinity);  exact: the non-finite set equals T for a NaN;  select: NaN / +Inf / -Inf as the reference has them.

Each entry plants NaN, +Inf and -Inf in turn at three sites of every float input: an interior element, a corner element, and an element of the
last channel vector.  The shapes are the smallest that reach each kernel; one entry runs all the plans of its shape (a failure lists them).
The tolerances are those of the ops' own tests, named where they are used; the references are torch on the CPU in fp64 and oracle/cpu_ref.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nonfinite as nf
import test_gpu_conv_views as cv

pytestmark = pytest.mark.gpu
ULP = cv.ULP
SLOPE = cv.SLOPE
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTN = {F32: "f32", F16: "f16", BF16: "bf16"}
WINO = "Winograd F(4,3): the 6x6 input transform mixes the tile, so T grows to whole 4x4 output tiles on the dilation lattice"
PATCH = ("matrix-core CReFF: P.V runs over the 8 x 14 keys under an 8 x 2 query patch, with probability 0 on the keys outside a query's own window "
         "(0 x NaN), so T grows to whole 2-row x 8-column query patches")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


rnd = cv.rnd
ACTS = {"none": lambda v: v, "relu": torch.relu, "prelu": lambda v: torch.where(v >= 0, v, SLOPE * v), "sigmoid": torch.sigmoid}


def act_code(act):
    from arseg_amd import _lib

    return {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU, "sigmoid": _lib.ACT_SIGMOID}[act]


def tol16(dtype, rel_extra=0.0, extra=0.0):
    """close16 of tests/test_gpu_16bit.py as a mask: |got - want| <= 0.51 ulp |want| + extra + rel_extra * max|want| + 1e-6."""
    def close(got, want):
        e = extra + (rel_extra * float(want.abs().max()) if want.numel() else 0.0)
        return (got - want).abs() <= ULP[dtype] * 0.51 * want.abs() + e + 1e-6
    return close


def tol_rel(rel):
    return lambda got, want: (got - want).abs() <= rel * (float(want.abs().max()) if want.numel() else 0.0)


ANY = lambda got, want: torch.ones_like(got, dtype=torch.bool)      # noqa: E731  (the chain entries: values are held by the single-conv entries)


class Spec:
    """One table entry: ``inputs`` (CPU tensors, finite), ``ref(inputs) -> fp64``, ``calls`` [(label, fn(inputs on the device) -> tensor, opts)],
    ``plant`` {input name: {site name: index}}, and the defaults of the per-call opts close / exact / select.  A call's opts may also hold
    ``grow`` (its allowed set, larger than T) together with ``reason``, one line that says why."""

    def __init__(self, inputs, ref, calls, plant, close, exact=False, select=False, math=None):
        self.inputs, self.ref, self.calls, self.plant, self.close, self.exact, self.select, self.math = inputs, ref, calls, plant, close, exact, select, math


TABLE = {}


def entry(name):
    def reg(fn):
        assert name not in TABLE, name
        TABLE[name] = fn
        return fn
    return reg


def nhwc_sites(inputs, keys, vec):
    return {k: nf.sites_nhwc(tuple(inputs[k].shape), vec) for k in keys if k in inputs}


# ================================================================================================ conv, fp32 engine
def ref32(name, act=None):
    """The fp64 reference of case ``name`` of tests/test_gpu_conv_views.py as a function of its inputs {"x", "res"} (NHWC), with another activation."""
    N, H, W, Cin, Cout, k, pad, dil, act0, use_bn, use_bias, use_res, up2 = cv.CASES32[name]
    c, fn = cv.case32(name), ACTS[act or act0]

    def f(i):
        xin = i["x"].double().permute(0, 3, 1, 2)
        if up2:
            xin = F.interpolate(xin, scale_factor=2.0, mode="bilinear", align_corners=False)
        y = F.conv2d(xin, c["w"].double(), None if c["b"] is None else c["b"].double(), padding=pad, dilation=dil)
        if c["bn"] is not None:
            bn = c["bn"]
            y = F.batch_norm(y, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
        if "res" in i:
            y = y + i["res"].double().permute(0, 3, 1, 2)
        return fn(y).permute(0, 2, 3, 1).contiguous()
    return f


@functools.lru_cache(maxsize=None)
def packed32(name, act, dev):
    from arseg_amd.packing import PackedConv

    N, H, W, Cin, Cout, k, pad, dil, act0, use_bn, use_bias, use_res, up2 = cv.CASES32[name]
    if act is None:
        return cv.packed32(name, dev)
    c = cv.case32(name)
    return PackedConv(c["w"], c["b"], c["bn"], 1, pad, dil, act_code(act), SLOPE, dev)


def inputs32(name):
    c = cv.case32(name)
    return {k: v for k, v in (("x", c["x"]), ("res", c["res"])) if v is not None}


def conv_calls(plans, oshape, dtype=F32, opts=None):
    """(label, fn(x, res, out)) of tests/test_gpu_conv_views.py -> calls of this table; ``out`` starts as a finite sentinel, so an element a plan
    does not write misses (b) or (a).  ``opts``: {label prefix: per-call opts}."""
    def wrap(fn):
        def call(i):
            ld = oshape[3] if dtype == F32 else (oshape[3] + 7) // 8 * 8          # (16-bit rows are padded to 8 channels, as ops.conv2d allocates them)
            o = torch.full(tuple(oshape[:3]) + (ld,), cv.SENTINEL, dtype=dtype, device=i["x"].device)[..., :oshape[3]]
            fn(i["x"], i.get("res"), o)
            return o
        return call
    return [(label, wrap(fn), next((v for k, v in (opts or {}).items() if label.startswith(k)), {})) for label, fn in plans]


def wino_plans(dev, pc, N, H, W, math, up2=False):
    return [(f"wino{g}", cv.wino(dev, pc, N, H, W, g, up2=up2)) for g in ((7, 100) if math == "f16x3" else (7,))]


def spec32(name, math, plans, grow=None, act=None, close=None):
    c = cv.case32(name)
    inputs = inputs32(name)
    opts = {"wino": {"grow": grow, "reason": WINO, "exact": False}} if grow is not None else None
    # tolerance: TOL of tests/test_gpu_conv_views.py (= test_conv2d / test_conv2d_winograd of tests/test_gpu_ops.py); the tap route its 5e-5
    calls = conv_calls(plans, c["oshape"], opts=dict(opts or {}, taps={"close": nf.within(cv.TOL_TAPS)}))
    return Spec(inputs, ref32(name, act), calls, nhwc_sites(inputs, ("x", "res"), 4), close or nf.within(cv.TOL), exact=True, math=math)


for _math in ("f32", "f16x3"):
    def _conv32_entries(math=_math):
        @entry(f"conv32/c1-3x3/{math}")
        def _(dev):
            """every implicit-GEMM tile, the split-K pairs (epilogue in the reduce kernel), the patch-resident plans, Winograd on both GEMMs"""
            N, H, W = cv.CASES32["c1"][:3]
            pc = packed32("c1", None, dev)
            plans = cv.direct_plans(pc, math)
            if math == "f16x3":
                plans += [(f"p{cfg}", cv.direct(pc, cfg, 1)) for cfg in (13, 14, 15, 16, 20, 21, 22)]
            return spec32("c1", math, plans + wino_plans(dev, pc, N, H, W, math), grow=nf.grow_tiles(4, 4))

        @entry(f"conv32/c2-3x3-dil4/{math}")
        def _(dev):
            N, H, W = cv.CASES32["c2"][:3]
            pc = packed32("c2", None, dev)
            return spec32("c2", math, cv.direct_plans(pc, math) + wino_plans(dev, pc, N, H, W, math), grow=nf.grow_tiles(4, 4, d=4))

        @entry(f"conv32/c3-1x1/{math}")
        def _(dev):
            """tiles, and under f16x3 the LDS-DMA GEMM (gemm_x3: ReLU + residual in its epilogue), every tile shape"""
            from arseg_amd import ops

            pc = packed32("c3", None, dev)
            plans = cv.direct_plans(pc, math, split_k=False)
            if math == "f16x3":
                plans += [(f"x3/{c}", (lambda c: lambda x_, r, o: ops._conv1x1_x3(x_, pc, r, o, False, c))(c)) for c in range(7)]
            return spec32("c3", math, plans)

        @entry(f"conv32/c4-1x1-ragged/{math}")
        def _(dev):
            """Cin = 36: the planted channel 35 sits next to the K padding"""
            pc = packed32("c4", None, dev)
            return spec32("c4", math, cv.direct_plans(pc, math, split_k=False))

        @entry(f"conv32/c5-up2/{math}")
        def _(dev):
            """the fused-upsample conv: tile 7 on the materialised upsample, the tap decomposition (upconv.hip), the patch plans that
            interpolate while they stage, up_3's persistent kernel (23, conv_up2_c64.hip), Winograd with the upsample in its input transform"""
            from arseg_amd import ops

            N, h, w = cv.CASES32["c5"][:3]
            pc = packed32("c5", None, dev)
            plans = [("t7", cv.direct(pc, 7, 1, up2=True)), ("taps", lambda x_, r, o: ops._conv_up2_taps(x_, pc, o))]
            if math == "f16x3":
                plans += [(f"p{cfg}", cv.direct(pc, cfg, 1, up2=True)) for cfg in (13, 15, 20, 21, 22, 23)]
            return spec32("c5", math, plans + wino_plans(dev, pc, N, 2 * h, 2 * w, math, up2=True), grow=nf.grow_tiles(4, 4))

        for act in ("none", "relu", "prelu", "sigmoid"):
            def _act_entries(act=act):
                @entry(f"conv32/c1-{act}/{math}")
                def _(dev):
                    """the activation on the branch-free epilogue (tile 7, patch plan 13), the generic one of the split-K reduce kernel, Winograd's"""
                    N, H, W = cv.CASES32["c1"][:3]
                    pc = packed32("c1", act, dev)
                    plans = [("t7", cv.direct(pc, 7, 1)), ("t3/3", cv.direct(pc, 3, 3)), ("t1/2", cv.direct(pc, 1, 2))]
                    if math == "f16x3":
                        plans += [("p13", cv.direct(pc, 13, 1))]
                    return spec32("c1", math, plans + wino_plans(dev, pc, N, H, W, math), grow=nf.grow_tiles(4, 4), act=act)

                @entry(f"conv32/c5-up2-{act}/{math}")
                def _(dev):
                    """the activation in the tap gather (upconv.hip) and in up_3's persistent kernel (conv_up2_c64.hip)"""
                    from arseg_amd import ops

                    pc = packed32("c5", act, dev)
                    plans = [("taps", lambda x_, r, o: ops._conv_up2_taps(x_, pc, o))]
                    if math == "f16x3":
                        plans += [("p23", cv.direct(pc, 23, 1, up2=True)), ("p13", cv.direct(pc, 13, 1, up2=True))]
                    return spec32("c5", math, plans, act=act)
            _act_entries()
    _conv32_entries()


for _act in ("none", "relu", "prelu"):
    @entry(f"conv32/identity-1x1-{_act}/f32")
    def _(dev, act=_act):
        """select: a 1x1 conv with identity weights in f32 math hands every element to the epilogue as it is -- NaN / +Inf / -Inf must come out as
        torch's ReLU / PReLU / identity leave them (the other channels of the pixel see 0 x Inf = NaN in both)"""
        from arseg_amd.packing import PackedConv

        C = 36
        x = rnd(3100, 1, 5, 7, C)
        w = torch.eye(C).reshape(C, C, 1, 1).contiguous()
        pc = PackedConv(w, None, None, 1, 0, 1, act_code(act), SLOPE, dev)
        ref = lambda i: ACTS[act]((i["x"].double().unsqueeze(-2) * w.double().reshape(C, C)).sum(-1))      # noqa: E731  elementwise: no BLAS between the NaN and the sum
        plans = [(f"t{cfg}", cv.direct(pc, cfg, 1)) for cfg in (1, 7, 12)]
        inputs = {"x": x}
        return Spec(inputs, ref, conv_calls(plans, (1, 5, 7, C)), nhwc_sites(inputs, ("x",), 4), nf.within(cv.TOL), exact=True, select=True, math="f32")


@entry("conv32/gemm_x3_cat-relu")
def _(dev):
    """arseg_gemm_x3_cat_fwd (the folded PSP bottleneck) with ReLU, every tile shape; tolerance of test_gemm_x3_cat (3e-6 of max|want|)"""
    from arseg_amd import _lib

    lib = _lib.load()
    B, M, K, K2, N = 2, 77, 32, 64, 36
    P = lambda a: ctypes.c_void_p(a.data_ptr() if a is not None else None)      # noqa: E731
    w, x2, w2 = rnd(3201, N, K, scale=0.1), rnd(3202, M, K2).abs(), rnd(3203, B, N, K2, scale=0.3)
    scale, bias = rnd(3204, N).abs().add(0.5), rnd(3205, N)
    inputs = {"x": rnd(3200, B, M, K)}

    def ref(i):
        return torch.relu((torch.einsum("bmk,nk->bmn", i["x"].double(), w.double()) + torch.einsum("mk,bnk->bmn", x2.double(), w2.double())) * scale.double() + bias.double())

    def call(cfg):
        def run(i):
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            sp = {}
            for name, a in (("x", i["x"]), ("w", w.to(dev)), ("x2", x2.to(dev)), ("w2", w2.to(dev))):
                sp[name] = torch.empty_like(a)
                _lib.check(lib.arseg_split_rows_fwd(P(a), a.shape[-1], P(sp[name]), a.numel() // a.shape[-1], a.shape[-1], 1.0, None, 0.0, st), "split")
            out = torch.full((B, M, N), cv.SENTINEL, device=dev)
            sc, bi = scale.to(dev), bias.to(dev)
            _lib.check(lib.arseg_gemm_x3_cat_fwd(P(sp["x"]), P(sp["w"]), P(sp["x2"]), P(sp["w2"]), P(out), M, N, K, K2, N, B, M * K * 4, 0, 0, N * K2 * 4, M * N,
                                                 P(sc), P(bi), _lib.ACT_RELU, 0.0, 0, cfg, None, 0.0, st), "gemm_x3_cat")
            torch.cuda.synchronize()
            return out
        return run
    sites = {"x": {"interior": (0, 40, 17), "corner": (1, 76, 0), "lastvec": (1, 33, 31)}}
    return Spec(inputs, ref, [(f"cfg{c}", call(c), {}) for c in range(7)], sites, tol_rel(3e-6), exact=True)


# ================================================================================================ conv, 16-bit engine
#        N, H,  W,  Cin, Cout, k, stride, pad, dil, act,    bn,   bias,  res,   up2
CASES16 = {
    "c6": (2, 9, 50, 64, 72, 3, 1, 2, 2, "prelu", True, True, True, False),          # cases c6 / c6n / c8 of tests/test_gpu_conv_views.py
    "c6n": (2, 9, 40, 64, 72, 3, 1, 2, 2, "prelu", True, True, True, False),
    "c8": (2, 7, 9, 128, 128, 1, 1, 0, 1, "relu", True, False, True, False),
    "up2": (2, 7, 25, 64, 64, 3, 1, 1, 1, "prelu", True, True, False, True),         # c7's layer on inputs the x2 upsample represents exactly (below)
    "stem": (1, 18, 22, 8, 64, 7, 2, 3, 1, "relu", True, False, False, False),       # the stem kernel (plan 9): RGB padded to 8 channels
    "tail": (1, 9, 40, 64, 36, 3, 1, 1, 1, "prelu", True, True, False, False),       # Cout % 8 != 0: the scalar tail of the patch kernel's epilogue
}


@functools.lru_cache(maxsize=None)
def case16(name, dtype, act=None):
    N, H, W, Cin, Cout, k, stride, pad, dil, act0, use_bn, use_bias, use_res, up2 = CASES16[name]
    act = act or act0
    seed = 4000 + 10 * sorted(CASES16).index(name)
    g = np.random.Generator(np.random.PCG64(seed))
    x = rnd(seed + 1, N, H, W, Cin)
    if up2:          # multiples of 1/2 in [-3.5, 3.5]: the x2 bilinear blend (weights 9, 3, 3, 1 / 16) of such values is exact in fp32, fp16 and bf16, so
        x = (2 * x).round().clamp(-7, 7) / 2          # the reference of the fused plans needs no rounded intermediate
    if name == "stem":
        x[..., 3:] = 0
    x = x.to(dtype)
    creal = 3 if name == "stem" else Cin
    w = rnd(seed + 2, Cout, creal, k, k, scale=(2.0 / (creal * k * k)) ** 0.5)
    b = rnd(seed + 3, Cout, scale=0.1) if use_bias else None
    bn = (cv.t(g.uniform(0.75, 1.25, Cout).astype(np.float32)), rnd(seed + 4, Cout, scale=0.1), rnd(seed + 5, Cout, scale=0.1),
          cv.t(g.uniform(0.5, 1.5, Cout).astype(np.float32)))
    Ho, Wo = ((H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1)
    if up2:
        Ho, Wo = 2 * H, 2 * W
    res = rnd(seed + 6, N, Ho, Wo, Cout).to(dtype) if use_res else None

    def ref(i):          # fp64 on the rounded operands (the fp64 block of test_conv2d16)
        xin = i["x"][..., :creal].double().permute(0, 3, 1, 2)
        if up2:
            xin = F.interpolate(xin, scale_factor=2.0, mode="bilinear", align_corners=False)
        y = F.conv2d(xin, w.to(dtype).double(), None, stride=stride, padding=pad, dilation=dil)
        gam, bet, mu, var = (v.double() for v in bn)
        sc = gam / torch.sqrt(var + 1e-5)
        sh = bet - mu * sc + (b.double() * sc if use_bias else 0)
        y = y * sc[None, :, None, None] + sh[None, :, None, None]
        if "res" in i:
            y = y + i["res"].double().permute(0, 3, 1, 2)
        return ACTS[act](y).permute(0, 2, 3, 1).contiguous()

    inputs = {k_: v for k_, v in (("x", x), ("res", res)) if v is not None}
    return {"inputs": inputs, "w": w, "b": b, "bn": bn, "ref": ref, "oshape": (N, Ho, Wo, Cout), "creal": creal}


@functools.lru_cache(maxsize=None)
def packed16(name, act, dev):
    from arseg_amd.packing import PackedConv

    N, H, W, Cin, Cout, k, stride, pad, dil, act0, use_bn, use_bias, use_res, up2 = CASES16[name]
    c = case16(name, F16)
    return PackedConv(c["w"], c["b"], c["bn"], stride, pad, dil, act_code(act or act0), SLOPE, dev)


def spec16(name, dtype, plans, act=None, sites=None):
    c = case16(name, dtype, act)
    # tolerance: near16 of tests/test_gpu_conv_views.py = close16 with extra = 2e-5 max|want| (test_conv2d16)
    return Spec(c["inputs"], c["ref"], conv_calls(plans, c["oshape"], dtype), sites or nhwc_sites(c["inputs"], ("x", "res"), 8), tol16(dtype, rel_extra=2e-5), exact=True)


for _dt in (F16, BF16):
    def _conv16_entries(dt=_dt):
        n = DTN[dt]

        @entry(f"conv16/c6-3x3-dil2/{n}")
        def _(dev):
            """conv16_kernel (tiles 1..4), its split-K reduce kernel, the squarer patch plans (5..8 refuse W = 50: c6n runs them)"""
            pc = packed16("c6", None, dev)
            plans = [(f"cfg{cfg}", cv.conv16(pc, cfg)) for cfg in (1, 2, 3, 4, 10, 11, 12, 13)] + [(f"cfg{cfg}/{sk}", cv.conv16(pc, cfg, sk)) for cfg, sk in cv.SPLIT_K16]
            return spec16("c6", dt, plans)

        @entry(f"conv16/c6n-3x3-dil2/{n}")
        def _(dev):
            pc = packed16("c6n", None, dev)
            return spec16("c6n", dt, [(f"cfg{cfg}", cv.conv16(pc, cfg)) for cfg in (5, 6, 7, 8, 11, 13)])

        @entry(f"conv16/c8-1x1/{n}")
        def _(dev):
            """tiles, and the LDS-DMA GEMM (gemm_rows16: the 16-bit epilogue of gemm_x3.hip)"""
            from arseg_amd import ops

            pc = packed16("c8", None, dev)
            plans = [(f"cfg{cfg}", cv.conv16(pc, cfg)) for cfg in (1, 2, 3, 4)]
            plans += [(f"rows{cfg}", (lambda cfg: lambda x_, r, o: ops.gemm_rows16(x_, pc, residual=r, out=o, cfg=cfg))(cfg)) for cfg in (0, 3, 9, 11)]
            return spec16("c8", dt, plans)

        @entry(f"conv16/up2/{n}")
        def _(dev):
            """the patch plans that interpolate while they stage"""
            pc = packed16("up2", None, dev)
            return spec16("up2", dt, [(f"cfg{cfg}", cv.conv16(pc, cfg, up2=True)) for cfg in (5, 7, 10, 11, 13)])

        @entry(f"conv16/stem/{n}")
        def _(dev):
            """the stem kernel's epilogue (plan 9) next to tile 1; planted in the three real channels (the padding channels have no reference)"""
            pc = packed16("stem", None, dev)
            sites = {"x": {"interior": (0, 9, 11, 1), "corner": (0, 17, 21, 0), "lastvec": (0, 8, 10, 2)}}
            return spec16("stem", dt, [("cfg9", cv.conv16(pc, 9)), ("cfg1", cv.conv16(pc, 1))], sites=sites)

        @entry(f"conv16/tail-cout36/{n}")
        def _(dev):
            """Cout = 36: the scalar tail of the patch kernel's epilogue (plans 5, 7, 11), and tile 1"""
            pc = packed16("tail", None, dev)
            return spec16("tail", dt, [(f"cfg{cfg}", cv.conv16(pc, cfg)) for cfg in (5, 7, 11, 1)])

        for act in ("none", "relu", "sigmoid"):          # (prelu: c6 / c6n above)
            @entry(f"conv16/c6n-{act}/{n}")
            def _(dev, act=act):
                """the activation in conv16_kernel (tile 1), the patch kernel (plan 7) and the split-K reduce kernel"""
                pc = packed16("c6n", act, dev)
                return spec16("c6n", dt, [("cfg1", cv.conv16(pc, 1)), ("cfg7", cv.conv16(pc, 7)), ("cfg1/2", cv.conv16(pc, 1, 2))], act=act)
    _conv16_entries()


# ================================================================================================ the two-conv chain
def _chain(dev, dtype, math):
    """3x3 + ReLU -> 1x1 + ReLU, 64 channels, 9 x 11, on the plans a model run takes: a NaN in the input is NaN in the output on D -- the ReLU of
    the first conv must not turn it into 0 for the second.  Only the sets are held here; the values are the single-conv entries' business."""
    from arseg_amd import _lib, ops
    from arseg_amd.packing import PackedConv

    x = rnd(5000, 1, 9, 11, 64).to(dtype)
    w1, w2 = rnd(5001, 64, 64, 3, 3, scale=(2.0 / 576) ** 0.5), rnd(5002, 64, 64, 1, 1, scale=(2.0 / 64) ** 0.5)
    b1, b2 = rnd(5003, 64, scale=0.1), rnd(5004, 64, scale=0.1)
    pc1 = PackedConv(w1, b1, None, 1, 1, 1, _lib.ACT_RELU, 0.0, dev)
    pc2 = PackedConv(w2, b2, None, 1, 0, 1, _lib.ACT_RELU, 0.0, dev)
    wd = (lambda w: w.to(dtype).double()) if dtype != F32 else (lambda w: w.double())

    def ref(i):
        h = torch.relu(F.conv2d(i["x"].double().permute(0, 3, 1, 2), wd(w1), b1.double(), padding=1))
        return torch.relu(F.conv2d(h, wd(w2), b2.double())).permute(0, 2, 3, 1).contiguous()

    calls = [("auto", lambda i: ops.conv2d(ops.conv2d(i["x"], pc1), pc2), {}),
             ("tile1", lambda i: ops.conv2d(ops.conv2d(i["x"], pc1, tile_cfg=1, split_k=1), pc2, tile_cfg=1, split_k=1), {})]
    inputs = {"x": x}
    return Spec(inputs, ref, calls, nhwc_sites(inputs, ("x",), 8), ANY, exact=True, math=math)


entry("chain/f32-storage/f16x3")(lambda dev: _chain(dev, F32, "f16x3"))
entry("chain/f32-storage/f32")(lambda dev: _chain(dev, F32, "f32"))
entry("chain/f16-storage")(lambda dev: _chain(dev, F16, None))
entry("chain/bf16-storage")(lambda dev: _chain(dev, BF16, None))


# ================================================================================================ small layers
def nchw(t_):
    return t_.double().permute(0, 3, 1, 2)


def nhwc(t_):
    return t_.permute(0, 2, 3, 1).contiguous()


def sliced(call):
    """``call`` on x as the channel slice [..., 8:8+C] of a wider NHWC buffer whose other channels hold finite junk."""
    def run(i):
        x = i["x"]
        wide = torch.full(tuple(x.shape[:3]) + (x.shape[3] + 16,), 0.75, dtype=x.dtype, device=x.device)
        wide[..., 8:8 + x.shape[3]] = x
        return call(dict(i, x=wide[..., 8:8 + x.shape[3]]))
    return run


def layer(name, dtypes, shape, ref, call, close, exact=False, select=False, slices=True, extra=None, plant=None, vec=None, scale=1.0):
    """Entries ``name``/<storage>[/slice] for an op on one NHWC input "x" (+ ``extra(dtype)`` finite inputs): ``ref(i)`` fp64 in NHWC, ``call(i)`` on the
    device, ``close(dtype)`` the tolerance of the op's own test.  ``scale``: the spread of x (a max over many elements wants them below the probe's +3)."""
    for dt in dtypes:
        for sl in ((False, True) if slices else (False,)):
            @entry(f"{name}/{DTN[dt]}" + ("/slice" if sl else ""))
            def _(dev, dt=dt, sl=sl):
                inputs = {"x": rnd(6000 + len(name), *shape, scale=scale).to(dt)}
                if extra:
                    inputs.update({k: v.to(dt) for k, v in extra().items()})
                sites = {k: nf.sites_nhwc(tuple(inputs[k].shape), vec or (4 if dt == F32 else 8)) for k in (plant or ("x",))}
                return Spec(inputs, ref, [("call", sliced(call) if sl else call, {})], sites, close(dt), exact=exact, select=select)


ALL = (F32, F16, BF16)
exact0 = lambda dt: nf.within(0.0)      # noqa: E731


def _ops():
    from arseg_amd import ops

    return ops


def _lib():
    from arseg_amd import _lib as lib

    return lib


# maxpool: a selection, exact (test_maxpool, test_small_layers16); maxpool3x3s2 copies a slice to dense rows first: no slice entry
layer("maxpool3x3s2", ALL, (2, 9, 13, 24), lambda i: nhwc(F.max_pool2d(nchw(i["x"]), 3, 2, 1)), lambda i: _ops().maxpool3x3s2(i["x"]), exact0,
      exact=True, select=True, slices=False)
# global max: exact (test_adaptive_avgpool_and_global_reduce, test_psp_pyramid16_and_global_max); mean: 1e-5 fp32 (the same test), close16 + 1e-6
# (test_small_layers16).  9 x 13: one stage; 40 x 52 x 36 channels of 2 images: the fp32 workspace form (test_global_reduce_two_stage's second shape, halved)
mean_tol = lambda dt: nf.within(1e-5) if dt == F32 else tol16(dt, extra=1e-6)      # noqa: E731
for _shape, _tag in (((2, 9, 13, 24), "one-stage"), ((2, 40, 52, 40), "workspace")):
    layer(f"global_max/{_tag}", ALL, _shape, lambda i: i["x"].double().amax(dim=(1, 2), keepdim=True), lambda i: _ops().global_reduce(i["x"], _lib().REDUCE_MAX),
          exact0, exact=True, select=True, scale=0.5)
    layer(f"global_mean/{_tag}", ALL, _shape, lambda i: i["x"].double().mean(dim=(1, 2), keepdim=True), lambda i: _ops().global_reduce(i["x"], _lib().REDUCE_MEAN),
          mean_tol if _tag == "one-stage" else (lambda dt: nf.within(2e-6) if dt == F32 else tol16(dt, extra=1e-6)), exact=True)
# adaptive average pool (fp32 only): 1e-5 (test_adaptive_avgpool_and_global_reduce); 9 x 13 into 2 x 2 and 6 x 6: overlapping bins
for _s in (2, 6):
    layer(f"adaptive_avgpool/{_s}", (F32,), (2, 9, 13, 20), lambda i, s=_s: nhwc(F.adaptive_avg_pool2d(nchw(i["x"]), (s, s))),
          lambda i, s=_s: _ops().adaptive_avgpool(i["x"], s, s), lambda dt: nf.within(1e-5), exact=True)

SIZES = (1, 2, 3, 6)
ROWS = sum(s * s for s in SIZES)


def _pool_matrix_ref(i):
    x = i["x"]
    N, H, W, C = x.shape
    want = torch.zeros(N, ROWS, 1, len(SIZES) * C, dtype=torch.float64)
    off = 0
    for k, s in enumerate(SIZES):
        want[:, off:off + s * s, 0, k * C:(k + 1) * C] = F.adaptive_avg_pool2d(nchw(x), s).permute(0, 2, 3, 1).reshape(N, s * s, C)
        off += s * s
    return want


# 1e-6 fp32 (test_psp_pool_matrix), close16 + 1e-6 (test_psp_pyramid16_and_global_max)
layer("psp_pool_matrix", ALL, (2, 9, 13, 24), _pool_matrix_ref, lambda i: _ops().psp_pool_matrix(i["x"], SIZES),
      lambda dt: nf.within(1e-6) if dt == F32 else tol16(dt, extra=1e-6), exact=True)


def _prior_ref(i, H=9, W=13):
    t_ = i["x"][:, :, 0]
    N, _, C = t_.shape
    want, off = torch.zeros(N, C, H, W, dtype=torch.float64), 0
    for s in SIZES:
        want += F.interpolate(t_[:, off:off + s * s].double().reshape(N, s, s, C).permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=False)
        off += s * s
    return nhwc(want)


# close16 + 1e-5 max|want| (test_psp_pyramid16_and_global_max); fp32: the same fp32-accumulation term alone.  "x" is t as [N, rows, 1, C]
layer("psp_prior_sum", ALL, (2, ROWS, 1, 24), _prior_ref, lambda i: _ops().psp_prior_sum(i["x"][:, :, 0], SIZES, 9, 13),
      lambda dt: tol_rel(1e-5) if dt == F32 else tol16(dt, rel_extra=1e-5), slices=False)

# resizes: 1e-5 fp32 (test_resize), close16 + 1e-5 (test_small_layers16); nearest exact.  Not exact: a kernel may skip a weight-0 tap torch multiplies
res_tol = lambda dt: nf.within(1e-5) if dt == F32 else tol16(dt, extra=1e-5)      # noqa: E731
for _tag, _hw, _out, _mode, _al in (("nearest", (5, 7), (10, 14), "nearest", False), ("nearest-odd", (5, 7), (11, 13), "nearest", False),
                                    ("bilinear-aligned", (5, 6), (13, 17), "bilinear", True), ("bilinear", (3, 5), (9, 12), "bilinear", False),
                                    ("bilinear-x2", (9, 13), (18, 26), "bilinear", False), ("bilinear-down", (10, 18), (9, 17), "bilinear", True)):
    def _resize(tag=_tag, hw=_hw, out=_out, mode=_mode, al=_al):
        kw = dict(mode=mode) if mode == "nearest" else dict(mode=mode, align_corners=al)
        m = lambda: _lib().NEAREST if mode == "nearest" else _lib().BILINEAR      # noqa: E731
        layer(f"resize_nhwc/{tag}", ALL, (2,) + hw + (24,), lambda i: nhwc(F.interpolate(nchw(i["x"]), out, **kw)),
              lambda i: _ops().resize_nhwc(i["x"], out[0], out[1], m(), al), exact0 if mode == "nearest" else res_tol, exact=mode == "nearest", select=mode == "nearest")
    _resize()
# resize_nchw (fp32; "x" is NCHW here, the sites are its own): generic, the x4 kernel (Wout % 4 == 0), the run-based x8 kernel, nearest
for _tag, _hw, _out, _mode, _al in (("nearest", (5, 7), (10, 14), "nearest", False), ("bilinear-aligned", (5, 6), (13, 17), "bilinear", True),
                                    ("bilinear-x4kernel", (3, 5), (9, 12), "bilinear", False), ("bilinear-runs-x8", (5, 3), (40, 24), "bilinear", False)):
    @entry(f"resize_nchw/{_tag}/f32")
    def _(dev, hw=_hw, out=_out, mode=_mode, al=_al):
        from arseg_amd import _lib, ops

        kw = dict(mode=mode) if mode == "nearest" else dict(mode=mode, align_corners=al)
        inputs = {"x": rnd(6100, 2, 6, *hw)}
        sites = {"x": {"interior": (0, 3, hw[0] // 2, hw[1] // 2), "corner": (1, 0, hw[0] - 1, hw[1] - 1), "lastvec": (1, 5, 0, hw[1] // 2)}}
        call = lambda i: ops.resize_nchw(i["x"], out[0], out[1], _lib.NEAREST if mode == "nearest" else _lib.BILINEAR, al)      # noqa: E731
        return Spec(inputs, lambda i: F.interpolate(i["x"].double(), out, **kw), [("call", call, {})], sites, nf.within(0.0 if mode == "nearest" else 1e-5),
                    exact=mode == "nearest", select=mode == "nearest")


def _sa_extra():
    return {"scale": rnd(6201, 2, 1, 1, 24), "add_full": rnd(6202, 2, 5, 7, 24), "add_vec": rnd(6203, 2, 1, 1, 24)}


# scale_add: 1e-6 fp32 (test_scale_add_head_frame_layouts), close16 + 1e-6 (test_small_layers16); planted in x, scale, add_full and add_vec in turn
layer("scale_add", ALL, (2, 5, 7, 24), lambda i: i["x"].double() * i["scale"].double() + i["add_full"].double() + i["add_vec"].double(),
      lambda i: _ops().scale_add(i["x"], i["scale"], add_full=i["add_full"], add_vec=i["add_vec"]), lambda dt: nf.within(1e-6) if dt == F32 else tol16(dt, extra=1e-6),
      exact=True, slices=False, extra=_sa_extra, plant=("x", "scale", "add_full", "add_vec"))

# head: 1e-4 fp32, 2e-4 16-bit (test_vector_width_edges, test_small_layers16).  C = 24 / 64: fp32 matrix-core kernel; C = 20 (fp32) and 24 (16-bit): the
# generic kernel; C = 64 (16-bit): its matrix-core kernel
for _C, _ncls, _lsm, _dts in ((64, 12, True, ALL), (64, 19, False, ALL), (24, 5, True, ALL), (24, 12, False, ALL), (20, 12, True, (F32,)), (20, 19, False, (F32,))):
    def _head(C=_C, ncls=_ncls, lsm=_lsm, dts=_dts):
        wf, bf = rnd(6300 + C, ncls, C, scale=0.2), rnd(6301 + C, ncls, scale=0.1)

        def ref(i):
            y = F.conv2d(nchw(i["x"]), wf.double()[:, :, None, None], bf.double())
            return F.log_softmax(y, dim=1) if lsm else y
        layer(f"head/c{C}-cls{ncls}" + ("-logsoftmax" if lsm else ""), dts, (2, 5, 7, C), ref, lambda i: _ops().head(i["x"], wf.to(i["x"].device), bf.to(i["x"].device), lsm),
              lambda dt: nf.within(1e-4 if dt == F32 else 2e-4), exact=True)
    _head()

# cast: exact in both directions (test_small_layers16)
for _src, _dst in ((F32, F16), (F32, BF16), (F16, F32), (BF16, F32)):
    @entry(f"cast/{DTN[_src]}-to-{DTN[_dst]}")
    def _(dev, src=_src, dst=_dst):
        from arseg_amd import ops

        inputs = {"x": rnd(6400, 2, 5, 7, 24).to(src)}
        return Spec(inputs, lambda i: i["x"].to(dst).double(), [("call", lambda i: ops.cast(i["x"], dst), {})], nhwc_sites(inputs, ("x",), 8), nf.within(0.0),
                    exact=True, select=True)

# frame ingest from a float frame ("x" is NCHW RGB): same size exact, the align_corners=True downscale 1e-5 (test_scale_add_head_frame_layouts) /
# close16 + 1e-6 (test_small_layers16); the result is the three colour channels of NHWC4 / NHWC8
for _dt in ALL:
    for _tag, _hw in (("same", (20, 30)), ("down", (10, 15))):
        @entry(f"frame_ingest/{_tag}/{DTN[_dt]}")
        def _(dev, dt=_dt, hw=_hw, tag=_tag):
            from arseg_amd import ops

            inputs = {"x": rnd(6500, 2, 3, 20, 30)}
            sites = {"x": {"interior": (0, 1, 9, 14), "corner": (1, 0, 19, 29), "lastvec": (1, 2, 4, 7)}}
            ref = lambda i: F.interpolate(i["x"].double(), hw, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)      # noqa: E731

            def call(i):
                out = ops.frame_ingest(i["x"], hw[0], hw[1], dt)
                assert float(out[..., 3:].abs().max()) == 0.0, "frame_ingest: the padding channels are not zero"
                return out[..., :3]
            close = (nf.within(0.0 if tag == "same" else 1e-5)) if dt == F32 else tol16(dt, extra=1e-6)
            return Spec(inputs, ref, [("call", call, {})], sites, close)


# ================================================================================================ warp and CReFF
# References: oracle/cpu_ref.py on the fp32 inputs (grid_sample wants the feature in the grid's fp32).  A result that does not depend on the site
# has the same bits under both probes, so D is as sharp as in fp64.  Motion: whole pixels, a few of them; a block of samples wholly off the image
# (their reference value is 0, whatever the border holds) and, at the border, samples with one or two taps outside.
def motion(seed, B, H, W):
    g = np.random.Generator(np.random.PCG64(seed))
    mv = g.integers(-2, 3, (B, H, W, 2)) * 4
    mv[:, : (H + 1) // 2, : W // 3, 0] = -4 * (W + 5)          # far off the image to the left: both taps of a row clamp onto column 0
    mv[:, H - 2:, W - 3:, 1] = 4 * (H + 3)                     # and off the bottom, next to the last pixel
    # every site of px_sites is sampled by somebody: the interior pixel by itself; the origin, the last pixel and pixel (H/2 - 1, 1) from
    # outside the blocks above (zero motion is not the identity -- ix = x W / (W - 1) - 0.5 -- so the two border samples have taps off the image)
    b = W // 3
    mv[:, H // 2, W // 2] = 0
    mv[:, 0, b] = (-4 * b, 0)
    mv[:, H // 2 - 1, b] = (-4 * (b - 1), 0)
    mv[:, H - 1, W - 4] = (12, 0)
    return torch.from_numpy(mv.astype(np.int16))


def px_sites(H, W, C, lead=()):
    """interior pixel; the image origin and the last pixel (border: clamped taps land on them); the last channel"""
    return {"interior": lead + (H // 2, W // 2, C // 2 + 1), "origin": lead + (0, 0, 1), "corner": lead + (H - 1, W - 1, 0), "lastvec": lead + (H // 2 - 1, 1, C - 1)}


def _warp_ref(i, mv):
    from oracle import cpu_ref

    x = i["x"].float()
    return nhwc(cpu_ref.warp_feature(x.permute(0, 3, 1, 2).contiguous(), cpu_ref.mv_resize(cpu_ref.mv_from_int16(mv), x.shape[1], x.shape[2]))).double()


for _H, _W in ((7, 9), (18, 35)):
    def _warp_entries(H=_H, W=_W):
        C, B = 16, 2
        mv = motion(7000 + H, B, H, W)

        for lay in ("nchw", "nhwc"):
            @entry(f"warp/{lay}/{H}x{W}")
            def _(dev, lay=lay):
                """ops.warp on a float flow field; 2e-5 (test_warp_large_motion)"""
                from arseg_amd import _lib, ops

                inputs = {"x": rnd(7001, B, H, W, C)}
                flow = (mv.double() / 4).to(dev)
                if lay == "nchw":
                    call = lambda i: nhwc(ops.warp(i["x"].permute(0, 3, 1, 2).contiguous(), flow, _lib.NCHW))      # noqa: E731
                else:
                    call = lambda i: ops.warp(i["x"], flow, _lib.NHWC)      # noqa: E731
                return Spec(inputs, lambda i: _warp_ref(i, mv), [("call", call, {})], {"x": px_sites(H, W, C, (0,))}, nf.within(2e-5))

        for out in ("nhwc", "c8"):
            @entry(f"warp_mvq/f32-{out}/{H}x{W}")
            def _(dev, out=out):
                """the MV-guided warp (identity MV resize); 1e-5 (test_warp_mvq_fused)"""
                from arseg_amd import _lib, ops

                inputs = {"x": rnd(7002, B, H, W, C)}
                mvd = mv.to(dev)
                if out == "nhwc":
                    call = lambda i: ops.warp_mvq(i["x"], mvd, _lib.NHWC)      # noqa: E731
                else:
                    call = lambda i: ops.from_c8(ops.warp_mvq(i["x"], mvd, _lib.C8), _lib.NHWC)      # noqa: E731
                return Spec(inputs, lambda i: _warp_ref(i, mv), [("call", call, {})], {"x": px_sites(H, W, C, (0,))}, nf.within(1e-5))

        for dt in (F16, BF16):
            @entry(f"warp_mvq/{DTN[dt]}-c8/{H}x{W}")
            def _(dev, dt=dt):
                """the 16-bit keyframe feature -> fp32 C8; 1e-5 on the rounded feature (test_warp_mvq16)"""
                from arseg_amd import _lib, ops

                inputs = {"x": rnd(7003, B, H, W, C).to(dt)}
                mvd = mv.to(dev)

                def call(i):
                    o = torch.empty((B, C // 8, H, W, 8), dtype=torch.float32, device=dev)
                    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    _lib.check(_lib.load().arseg_warp_mvq16_fwd(ctypes.c_void_p(i["x"].data_ptr()), ops._DT16[dt], ctypes.c_void_p(mvd.data_ptr()),
                                                                ctypes.c_void_p(o.data_ptr()), B, C, H, W, H, W, st), "warp_mvq16")
                    return ops.from_c8(o, _lib.NHWC)
                return Spec(inputs, lambda i: _warp_ref(i, mv), [("call", call, {})], {"x": px_sites(H, W, C, (0,))}, nf.within(1e-5))

        @entry(f"local_attention/{H}x{W}")
        def _(dev):
            """local_similar (planted in q and in k) then local_weighting of k by the softmax of the scores, NCHW and channels_last; 1e-5, the
            tighter bound of test_local_pair (its 1e-4 is for the scores alone)"""
            from arseg_amd import ops
            from oracle import cpu_ref

            inputs = {"q": rnd(7004, B, H, W, 8, scale=0.3), "k": rnd(7005, B, H, W, 8, scale=0.3)}
            f = lambda t_: t_.float().permute(0, 3, 1, 2).contiguous()      # noqa: E731

            def ref(i):
                w = torch.softmax(cpu_ref.local_similar(f(i["q"]), f(i["k"]), 7, 7), dim=3)
                return nhwc(cpu_ref.local_weighting(f(i["k"]), w, 7, 7)).double()

            def call(cl):
                def run(i):
                    q, k = i["q"].permute(0, 3, 1, 2), i["k"].permute(0, 3, 1, 2)          # channels_last views
                    if not cl:
                        q, k = q.contiguous(), k.contiguous()
                    return nhwc(ops.local_weighting(k, torch.softmax(ops.local_similar(q, k, 7, 7), dim=3), 7, 7))
                return run
            sites = {k_: px_sites(H, W, 8, (0,)) for k_ in ("q", "k")}
            return Spec(inputs, ref, [("nchw", call(False), {}), ("channels_last", call(True), {})], sites, nf.within(1e-5))
    _warp_entries()


@functools.lru_cache(maxsize=None)
def attention(C, dev):
    from arseg_amd import synth
    from arseg_amd.model import MyAttention
    from arseg_amd.packing import PackedAttention

    m = synth.load_synth_weights(MyAttention(C, kW=7, kH=7), 7, attn_gain=0.35)
    return {kk: v.clone() for kk, v in m.state_dict().items()}, PackedAttention(m, dev)


def _creff_ref(i, sd, mv=None):
    """warp (if ``mv``) -> MyAttention on the fp32 values of the inputs: "hr" [B,Hp,Wp,C] keyframe features, "lr" [B,hp,wp,C]"""
    from oracle import cpu_ref

    f = lambda t_: t_.float().permute(0, 3, 1, 2).contiguous()      # noqa: E731
    hr = f(i["hr"])
    if mv is not None:
        hr = cpu_ref.warp_feature(hr, cpu_ref.mv_resize(cpu_ref.mv_from_int16(mv), hr.shape[2], hr.shape[3]))
    return nhwc(cpu_ref.my_attention(sd, "", hr, f(i["lr"]), 7, 7)).double()


def _configured(call, **kw):
    def run(i):
        from arseg_amd import ops

        prev = ops.configure(**kw)
        try:
            return call(i)
        finally:
            ops.configure(**prev)
    return run


for _H, _W in ((7, 9), (18, 35)):
    def _creff_entries(H=_H, W=_W):
        h, w, B = (H + 1) // 2, (W + 1) // 2, 2
        mv = motion(7100 + H, B, H, W)
        patch = {"grow": nf.grow_tiles(2, 8), "reason": PATCH}          # tiles and strips start at multiples of 16 columns and of 2 rows

        def sites(C):          # two frames: whatever one plant reaches in its own frame, the other frame stays outside A
            return {"hr": px_sites(H, W, C, (0,)), "lr": px_sites(h, w, C, (1,))}

        @entry(f"creff/{H}x{W}")
        def _(dev):
            """arseg_creff_fwd on its three kernels; 1e-4 (test_creff_vs_oracle at this gain)"""
            from arseg_amd import _lib, ops

            C = 16
            sd, pa = attention(C, dev)
            inputs = {"hr": rnd(7101, B, H, W, C), "lr": rnd(7102, B, h, w, C)}
            call = lambda i: ops.from_c8(ops.creff(ops.to_c8(i["hr"], _lib.NHWC), i["lr"], pa, None, False, 7, 7)[0], _lib.NHWC)      # noqa: E731
            calls = [("valu", _configured(call, creff_impl="valu"), {}), ("mfma16", _configured(call, creff_impl="mfma", creff_tile_rows=16), patch),
                     ("mfma8", _configured(call, creff_impl="mfma", creff_tile_rows=8), patch)]
            return Spec(inputs, lambda i: _creff_ref(i, sd), calls, sites(C), nf.within(1e-4))

        @entry(f"creff_warp/fused-f32/{H}x{W}")
        def _(dev):
            """the fused warp + CReFF kernels: rolling (default schedule, and 6-row segments on 3 workgroups) and tiles; 1e-4 (test_creff_warp_fused)"""
            from arseg_amd import _lib, ops

            C = 64
            sd, pa = attention(C, dev)
            inputs = {"hr": rnd(7103, B, H, W, C), "lr": rnd(7104, B, h, w, C)}
            mvd = mv.to(dev)
            call = lambda i: ops.creff_warp([i["hr"][b] for b in range(B)], mvd, i["lr"], pa, None, False, 7, 7, p_layout=_lib.NHWC)[0]      # noqa: E731
            calls = [("roll", _configured(call, creff_warp_impl="roll", creff_seg_rows=0, creff_max_wgs=0), patch),
                     ("roll/seg6", _configured(call, creff_warp_impl="roll", creff_seg_rows=6, creff_max_wgs=3), patch),
                     ("tiles", _configured(call, creff_warp_impl="tiles", creff_seg_rows=0, creff_max_wgs=0), patch)]
            return Spec(inputs, lambda i: _creff_ref(i, sd, mv), calls, sites(C), nf.within(1e-4))

        for dt in (F16, BF16):
            @entry(f"creff_warp/direct-{DTN[dt]}/{H}x{W}")
            def _(dev, dt=dt):
                """the rolling kernel reading 16-bit features as they are (bit-equal to the fp32 kernel on the widened values:
                tests/test_gpu_creff16.py); 1e-4 on the rounded inputs, as the fp32 kernel"""
                from arseg_amd import _lib, ops

                C = 64
                sd, pa = attention(C, dev)
                inputs = {"hr": rnd(7105, B, H, W, C).to(dt), "lr": rnd(7106, B, h, w, C).to(dt)}
                mvd = mv.to(dev)
                call = lambda i: ops.creff_warp([i["hr"][b] for b in range(B)], mvd, i["lr"], pa, None, False, 7, 7, p_layout=_lib.NHWC)[0]      # noqa: E731
                return Spec(inputs, lambda i: _creff_ref(i, sd, mv), [("direct", _configured(call, creff_warp16="direct", creff_warp_impl=""), patch)], sites(C), nf.within(1e-4))

        for dt in (F32, F16):
            @entry(f"creff_warp/two-kernel-c128-{DTN[dt]}/{H}x{W}")
            def _(dev, dt=dt):
                """C = 128: a warp launch + the matrix-core CReFF kernel; 2e-4 (test_creff_warp_wide_and_16bit)"""
                from arseg_amd import _lib, ops

                C = 128
                sd, pa = attention(C, dev)
                inputs = {"hr": rnd(7107, B, H, W, C).to(dt), "lr": rnd(7108, B, h, w, C).to(dt)}
                mvd = mv.to(dev)
                call = lambda i: ops.creff_warp([i["hr"][b] for b in range(B)], mvd, i["lr"], pa, None, False, 7, 7, p_layout=_lib.NHWC)[0]      # noqa: E731
                return Spec(inputs, lambda i: _creff_ref(i, sd, mv), [("call", call, patch)], sites(C), nf.within(2e-4))
    _creff_entries()


# ================================================================================================ the test
def _to_dev(i, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in i.items()}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_nonfinite(dev, name):
    from arseg_amd import ops

    spec = TABLE[name](dev)
    prev = ops.set_conv_math(spec.math) if spec.math else None
    fails, n = [], 0
    try:
        for key, sites in spec.plant.items():
            for site in sites.values():
                p = nf.Probe(name, spec.ref, spec.inputs, key, site)
                for v in nf.PLANTS:
                    ind = _to_dev(p.inputs[v], dev)
                    for label, call, o in spec.calls:
                        n += 1
                        assert o.get("grow") is None or o.get("reason"), f"{name} [{label}]: an allowed set larger than T needs its reason in the table"
                        try:
                            p.check(v, call(ind), o.get("close", spec.close), exact=o.get("exact", spec.exact), select=o.get("select", spec.select), grow=o.get("grow"))
                        except AssertionError as e:
                            fails.append(f"[{label}] {e}")
    finally:
        if prev is not None:
            ops.set_conv_math(prev)
    assert not fails, f"{len(fails)} of {n} checks failed:\n" + "\n".join(fails[:60])


def test_cast_overflow_gives_inf(dev):
    """fp32 finite values above the fp16 range become +-Inf, as .to(torch.float16) gives; bf16 keeps them finite (same exponent range)."""
    from arseg_amd import ops

    x = rnd(6600, 4, 40)
    x[0, 3], x[1, 7], x[2, 0], x[3, 39] = 65520.0, -1e5, 3e38, 65519.0          # 65520 rounds to Inf (ties to even), 65519 to 65504
    for dst in (F16, BF16):
        got, want = ops.cast(x.to(dev), dst).cpu(), x.to(dst)
        assert torch.equal(nf.klass(got), nf.klass(want)) and torch.equal(got.view(torch.int16), want.view(torch.int16)), dst
    assert int((nf.klass(x.to(F16)) != 0).sum()) == 3 and int((nf.klass(x.to(BF16)) != 0).sum()) == 0
