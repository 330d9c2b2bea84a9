"""Every conv plan on channel-slice views: the input, the output and the residual of a conv are slices of wider NHWC buffers all the time
(zero-copy concat: layer4's last block, BiSeNet's fcat), and which kernel serves such a call is decided by timing -- so each plan is pinned
here in turn and held to the same five properties on each view:

  1. the dense call on the pinned plan is deterministic (two runs, torch.equal);
  2. the view call returns the dense call's bits (a view changes addresses, never arithmetic);
  3. the view call is accepted exactly when the dense call is;
  4. the neighbours of the output slice keep their sentinel (-7.0) bit for bit, and the wide input / residual buffers (NaN outside the slice,
     so that any read outside it poisons the result) are unchanged;
  5. the automatic plan and the pinned reference plans also meet the fp64 reference of the operation within the tolerance of the path's
     dense test (2e-4 fp32 direct / Winograd, 5e-5 tap decomposition, close16 for the 16-bit path).

The output slice itself starts as NaN: an element a plan does not write fails (2).

Views (offsets in channels).  fp32 -- A "aligned": in 32|0, out 16|16, res 8|4;  B "16-byte only": in 4|4, out 4|8, res 12|0;  C "odd":
in as B (the library wants a 16-byte-aligned input with in_ld % 4 == 0), out 5|6, res 3|0: odd pitches, nothing vector aligned.  16-bit -- A:
in 8|8, out 8|16, res 16|0 (multiples of 8 halves, which the library requires).  In B the output and the residual have the same pitch (Cout
+ 12) at different offsets; in A and C all three pitches differ.

The cached-route tests at the end cover the host-side hole: the plan key of ``conv2d`` holds the shape, not the pitch / alignment of ``out``
and ``residual``, so a plan cached from a dense call ("x3", "taps", tile_cfg 23, "gemm16") meets a later view it refuses."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import SENTINEL, bits, boxed, maxdiff, neighbours_intact, pinned, t

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = [torch.float16, torch.bfloat16]
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}          # as tests/test_gpu_16bit.py
TOL, TOL_TAPS = 2e-4, 5e-5                                            # tests/test_gpu_ops.py: test_conv2d / test_conv2d_winograd*, the tap route

V32 = {"A": {"inp": (32, 0), "out": (16, 16), "res": (8, 4)},
       "B": {"inp": (4, 4), "out": (4, 8), "res": (12, 0)},
       "C": {"inp": (4, 4), "out": (5, 6), "res": (3, 0)}}
V16 = {"A": {"inp": (8, 8), "out": (8, 16), "res": (16, 0)}}
SPLIT_K32 = ((3, 3), (7, 3), (1, 2), (5, 2), (11, 2), (9, 3))         # test_conv2d's pairs; (19, 2) joins them under f16x3
SPLIT_K16 = ((1, 2), (3, 3), (4, 8))                                  # test_conv2d16's pairs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(params=["f32", "f16x3"])
def conv_math(request):
    from arseg_amd import ops

    prev = ops.set_conv_math(request.param)
    yield request.param
    ops.set_conv_math(prev)


def rnd(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32))


def close16(got, want, dtype, extra=0.0):
    """|got - want| <= ulp/2 * |want| + (fp32 accumulation slack) elementwise (the bound of tests/test_gpu_16bit.py)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    tol = ULP[dtype] * 0.51 * want.abs() + extra + 1e-6
    bad = (got - want).abs() > tol
    assert not bool(bad.any()), (float((got - want).abs().max()), int(bad.sum()))


def sweep(plans, x, res, oshape, view, refs=(), refuse=(), loose=()):
    """Oracles 1-5 for every (label, fn) of ``plans`` on one view; fn(x, res, out) launches one pinned plan.  ``view``: {"inp" / "out" / "res":
    (lead, trail)}, "inp" None = the dense input.  ``refs``: {label: check(got)} -- the reference check of those plans, made on the view's
    result.  ``refuse``: the labels whose plan refuses this shape (dense and view alike); every other plan must run.  ``loose``: labels that
    may pick another kernel for a view (an automatic plan with a layout fallback): held to everything but the bit equality.  Returns the
    number of plans that ran."""
    from arseg_amd import _lib

    def fresh():
        return torch.full(oshape, NAN, dtype=x.dtype, device=x.device)

    dense = {}
    for label, fn in plans:
        a, b = fresh(), fresh()
        try:
            fn(x, res, a)
        except _lib.ArsegError:
            assert label in refuse, f"{label}: refused the dense call"
            dense[label] = None
            continue
        assert label not in refuse, f"{label}: expected to refuse this shape"
        fn(x, res, b)
        assert torch.equal(a, b), f"{label}: two dense runs differ by {maxdiff(a, b):.3g}"
        dense[label] = a
    wx, vx = (None, x) if view["inp"] is None else boxed(x, *view["inp"], NAN)
    wr, vr = (None, None) if res is None else boxed(res, *view["res"], NAN)
    wx0 = None if wx is None else wx.clone()
    wr0 = None if wr is None else wr.clone()
    lead, cout = view["out"][0], oshape[3]
    n_run = 0
    for label, fn in plans:
        wo, vo = boxed(fresh(), *view["out"], SENTINEL)
        if dense[label] is None:
            with pytest.raises(_lib.ArsegError):
                fn(vx, vr, vo)
        else:
            fn(vx, vr, vo)                                       # (an ArsegError here: the view is refused where dense is accepted)
            if label not in loose:
                assert torch.equal(vo, dense[label]), f"{label}: view differs from dense by {maxdiff(vo, dense[label]):.3g}"
            if label in refs:
                refs[label](vo)
            n_run += 1
        assert neighbours_intact(wo, lead, cout), f"{label}: wrote outside the output slice"
        if dense[label] is None:
            assert bool(torch.isnan(vo).all()), f"{label}: refused the call but wrote the output"
        assert wx is None or torch.equal(bits(wx), bits(wx0)), f"{label}: the input buffer changed"
        assert wr is None or torch.equal(bits(wr), bits(wr0)), f"{label}: the residual buffer changed"
    return n_run


# ------------------------------------------------------------------------------------------------ fp32 cases
#        N, H,  W,  Cin, Cout, k, pad, dil, act,    bn,    bias,  res,   up2      (up2: H x W is the LOW resolution, the conv runs at 2H x 2W)
CASES32 = {
    "c1": (2, 9, 50, 64, 96, 3, 1, 1, "relu", True, False, True, False),        # row / column tails against the 64-wide tiles, Cout tail
    "c2": (1, 10, 13, 128, 128, 3, 4, 4, "relu", True, False, True, False),     # layer4's last block, shrunk
    "c3": (2, 7, 9, 64, 128, 1, 0, 1, "relu", False, True, True, False),
    "c4": (1, 5, 7, 36, 10, 1, 0, 1, "none", False, True, False, False),        # K padding next to NaN neighbours, Cout tail next to sentinels
    "c5": (2, 7, 25, 64, 64, 3, 1, 1, "prelu", True, True, False, True),        # up_3, shrunk
}
SLOPE = 0.2


@functools.lru_cache(maxsize=None)
def case32(name):
    """The layer, its NHWC inputs and its fp64 reference (NHWC): built once, shared by every test of the case, never written."""
    N, H, W, Cin, Cout, k, pad, dil, act, use_bn, use_bias, use_res, up2 = CASES32[name]
    seed = 1000 + 10 * int(name[1:])
    g = np.random.Generator(np.random.PCG64(seed))
    x = rnd(seed + 1, N, H, W, Cin)
    w = rnd(seed + 2, Cout, Cin, k, k, scale=float(np.sqrt(2.0 / (Cin * k * k))))
    b = rnd(seed + 3, Cout, scale=0.1) if use_bias else None
    bn = None
    if use_bn:
        bn = (t(g.uniform(0.5, 1.5, Cout).astype(np.float32)), rnd(seed + 4, Cout, scale=0.1), rnd(seed + 5, Cout, scale=0.1),
              t(g.uniform(0.5, 1.5, Cout).astype(np.float32)))                   # gamma, beta, mean, var
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    res = rnd(seed + 6, N, Ho, Wo, Cout) if use_res else None
    xin = x.double().permute(0, 3, 1, 2)
    if up2:
        xin = F.interpolate(xin, scale_factor=2.0, mode="bilinear", align_corners=False)
    y = F.conv2d(xin, w.double(), None if b is None else b.double(), padding=pad, dilation=dil)
    if bn is not None:
        y = F.batch_norm(y, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
    if res is not None:
        y = y + res.double().permute(0, 3, 1, 2)
    if act == "relu":
        y = F.relu(y)
    elif act == "prelu":
        y = torch.where(y >= 0, y, SLOPE * y)
    return {"x": x, "w": w, "b": b, "bn": bn, "res": res, "want": y.permute(0, 2, 3, 1).contiguous(), "oshape": (N, Ho, Wo, Cout)}


@functools.lru_cache(maxsize=None)
def packed32(name, dev):
    from arseg_amd import _lib
    from arseg_amd.packing import PackedConv

    N, H, W, Cin, Cout, k, pad, dil, act, use_bn, use_bias, use_res, up2 = CASES32[name]
    c = case32(name)
    code = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU}[act]
    return PackedConv(c["w"], c["b"], c["bn"], 1, pad, dil, code, SLOPE, dev)


def on_dev(name, dev):
    c = case32(name)
    return c["x"].to(dev), None if c["res"] is None else c["res"].to(dev)


def near(name, tol):
    want = case32(name)["want"]

    def check(got):
        e = maxdiff(got, want)
        assert e <= tol, f"{e:.3g} from the fp64 reference (bound {tol:g})"
    return check


def tiles32(math):
    return tuple(range(1, 13)) + ((17, 18, 19) if math == "f16x3" else ())


def direct(pc, cfg, sk, up2=False):
    from arseg_amd import ops

    return lambda x, r, o: ops.conv2d(x, pc, residual=r, out=o, tile_cfg=cfg, split_k=sk, up2=up2)


def auto(pc, up2=False):
    from arseg_amd import ops

    return lambda x, r, o: ops.conv2d(x, pc, residual=r, out=o, up2=up2)


def wino(dev, pc, N, H, W, gemm, up2=False):
    """The Winograd route with its batched GEMM pinned to ``gemm`` (implicit-GEMM tile, or 100 + a gemm_x3 tile): nothing is tuned."""
    from arseg_amd import _lib, ops

    def fn(x, r, o):
        T = _lib.load().arseg_wino43_tiles(N, H, W, pc.dil)
        with pinned(("wino_gemm", dev.index, T, pc.cin_pad, pc.cout, ops._config.sw.math), gemm):
            ops._conv_wino(x, pc, r, o, N, H, W, up2=up2)
    return fn


def direct_plans(pc, math, split_k=True):
    plans = [(f"t{cfg}", direct(pc, cfg, 1)) for cfg in tiles32(math)]
    if split_k:
        plans += [(f"t{cfg}/{sk}", direct(pc, cfg, sk)) for cfg, sk in SPLIT_K32 + (((19, 2),) if math == "f16x3" else ())]
    return plans


@pytest.mark.parametrize("view", ["A", "B", "C"])
def test_conv3x3_views(dev, conv_math, view):
    """Case 1: 3x3 s1 p1 d1, 64 -> 96, N=2, 9 x 50, BN + ReLU, residual: every implicit-GEMM tile, the split-K pairs (their reduce kernel
    reads the residual and writes ``out`` itself), the patch-resident plans (none may refuse at W = 50, dil 1) and Winograd on both GEMMs."""
    N, H, W = CASES32["c1"][:3]
    pc = packed32("c1", dev)
    x, res = on_dev("c1", dev)
    plans = [("auto", auto(pc))] + direct_plans(pc, conv_math)
    if conv_math == "f16x3":
        plans += [(f"p{cfg}", direct(pc, cfg, 1)) for cfg in (13, 14, 15, 16, 20, 21, 22)]
    plans += [(f"wino{g}", wino(dev, pc, N, H, W, g)) for g in ((7, 100) if conv_math == "f16x3" else (7,))]
    refs = {k: near("c1", TOL) for k in ("auto", "t7", "wino7", "wino100")}
    n_run = sweep(plans, x, res, case32("c1")["oshape"], V32[view], refs=refs)
    assert n_run == {"f32": 20, "f16x3": 32}[conv_math]


@pytest.mark.parametrize("view", ["A", "C"])
def test_conv3x3_dilated_views(dev, conv_math, view):
    """Case 2: 3x3 dil 4 pad 4, 128 -> 128, N=1, 10 x 13, BN + ReLU, residual (layer4's last block writes cat[..., :C] with a dense
    residual): tiles, split-K and Winograd's polyphase path."""
    N, H, W = CASES32["c2"][:3]
    pc = packed32("c2", dev)
    x, res = on_dev("c2", dev)
    plans = [("auto", auto(pc))] + direct_plans(pc, conv_math)
    plans += [(f"wino{g}", wino(dev, pc, N, H, W, g)) for g in ((7, 100) if conv_math == "f16x3" else (7,))]
    refs = {k: near("c2", TOL) for k in ("auto", "t7", "wino7", "wino100")}
    n_run = sweep(plans, x, res, case32("c2")["oshape"], V32[view], refs=refs)
    assert n_run == {"f32": 20, "f16x3": 25}[conv_math]


@pytest.mark.parametrize("view", ["A", "B"])
def test_conv1x1_views(dev, conv_math, view):
    """Case 3: 1x1, 64 -> 128, N=2, 7 x 9, bias + ReLU, residual: tiles, and the LDS-DMA GEMM (split-row pre-pass of the input view, then
    every tile shape; its epilogue loads the residual and stores the output as 16-byte pieces)."""
    from arseg_amd import ops

    pc = packed32("c3", dev)
    x, res = on_dev("c3", dev)
    plans = [("auto", auto(pc))] + direct_plans(pc, conv_math, split_k=False)
    if conv_math == "f16x3":
        plans += [(f"x3/{c}", (lambda c: lambda x_, r, o: ops._conv1x1_x3(x_, pc, r, o, False, c))(c)) for c in range(7)]
    refs = {k: near("c3", TOL) for k in ("auto", "t7", "x3/3")}
    n_run = sweep(plans, x, res, case32("c3")["oshape"], V32[view], refs=refs)
    assert n_run == {"f32": 13, "f16x3": 23}[conv_math]


@pytest.mark.parametrize("view", ["B", "C"])
def test_conv1x1_ragged_channels_views(dev, conv_math, view):
    """Case 4: 1x1, 36 -> 10 (Cin % 32 != 0, Cout % 4 != 0), N=1, 5 x 7, bias: the K padding of every tile sits next to the NaN neighbours of
    the input slice, the Cout tail next to the sentinels."""
    pc = packed32("c4", dev)
    x, _ = on_dev("c4", dev)
    plans = [("auto", auto(pc))] + direct_plans(pc, conv_math, split_k=False)
    n_run = sweep(plans, x, None, case32("c4")["oshape"], V32[view], refs={k: near("c4", TOL) for k in ("auto", "t7")})
    assert n_run == {"f32": 13, "f16x3": 16}[conv_math]


@pytest.mark.parametrize("view", ["A", "B"])
def test_conv_up2_views(dev, conv_math, view):
    """Case 5: conv3x3 on the x2 upsample of x_low [2,7,25,64] -> 64 channels at 14 x 50, bias + BN + PReLU: the patch plans that interpolate
    while they stage (13, 15, 20..22), up_3's persistent kernel (23), the tap decomposition, Winograd with the upsample in its input
    transform, and tile 7 on the materialised upsample.  Input and output views A and B."""
    from arseg_amd import ops

    N, h, w = CASES32["c5"][:3]
    pc = packed32("c5", dev)
    x, _ = on_dev("c5", dev)
    plans = [("auto", auto(pc, up2=True)), ("t7", direct(pc, 7, 1, up2=True)), ("taps", lambda x_, r, o: ops._conv_up2_taps(x_, pc, o))]
    if conv_math == "f16x3":
        plans += [(f"p{cfg}", direct(pc, cfg, 1, up2=True)) for cfg in (13, 15, 20, 21, 22, 23)]
    plans += [(f"wino{g}", wino(dev, pc, N, 2 * h, 2 * w, g, up2=True)) for g in ((7, 100) if conv_math == "f16x3" else (7,))]
    refs = {k: near("c5", TOL) for k in ("auto", "t7", "p13", "p23", "wino7", "wino100")}
    refs["taps"] = near("c5", TOL_TAPS)
    n_run = sweep(plans, x, None, case32("c5")["oshape"], V32[view], refs=refs)
    assert n_run == {"f32": 4, "f16x3": 11}[conv_math]


def test_conv_up2_split_rows_input_views(dev):
    """Case 5 from a SplitRows input (the tap route's GEMM stages the split rows directly) into an ``out`` view; and the split pre-pass
    itself on an input view with NaN neighbours."""
    from arseg_amd import ops

    pc = packed32("c5", dev)
    x, _ = on_dev("c5", dev)
    prev = ops.set_conv_math("f16x3")
    try:
        assert ops.gemm_x3_enabled()
        xs = ops.split_rows(x)
        for vname in ("A", "B"):
            wx, vx = boxed(x, *V32[vname]["inp"], NAN)
            assert torch.equal(bits(ops.split_rows(vx).t), bits(xs.t)), vname
        n_run = sweep([("taps(x3)", lambda x_, r, o: ops.conv2d(ops.SplitRows(x_), pc, out=o, up2=True))], xs.t, None, case32("c5")["oshape"],
                      {"inp": None, "out": V32["A"]["out"]}, refs={"taps(x3)": near("c5", TOL_TAPS)})
        assert n_run == 1
    finally:
        ops.set_conv_math(prev)


def test_conv2d_rejects_strided_channels(dev):
    """Views with a non-unit channel stride are not NHWC slices: refused on the host, before any launch."""
    from arseg_amd import _lib, ops

    x, _ = on_dev("c4", dev)
    wide = torch.zeros((1, 5, 7, 72), device=dev)
    with pytest.raises(_lib.ArsegError):
        ops.conv2d(wide[..., ::2], packed32("c4", dev))
    with pytest.raises(_lib.ArsegError):
        ops.conv2d(x, packed32("c4", dev), out=wide[..., :20:2])


# ------------------------------------------------------------------------------------------------ 16-bit cases
#        N, H,  W,  Cin, Cout, k, pad, dil, act,     bn,   bias,  res,   up2
CASES16 = {
    "c6": (2, 9, 50, 64, 72, 3, 2, 2, "prelu", True, True, True, False),
    # c6 at W = 40: at W = 50 the 64-wide default tile of plans 5..8 does not hold a dil-2 halo (they refuse, dense and view alike);
    # here the tile is 32 wide and they run, so that every plan id executes under view A somewhere
    "c6n": (2, 9, 40, 64, 72, 3, 2, 2, "prelu", True, True, True, False),
    "c7": (2, 7, 25, 64, 64, 3, 1, 1, "prelu", True, True, False, True),
    "c8": (2, 7, 9, 128, 128, 1, 0, 1, "relu", True, False, True, False),
}


@functools.lru_cache(maxsize=None)
def case16(name, dtype):
    """The layer and its 16-bit NHWC inputs; "ref"(xin) = fp64 on the same rounded operands (the fp64 block of test_conv2d16), NHWC."""
    N, H, W, Cin, Cout, k, pad, dil, act, use_bn, use_bias, use_res, up2 = CASES16[name]
    seed = 2000 + 10 * int(name[1])
    g = np.random.Generator(np.random.PCG64(seed))
    x = rnd(seed + 1, N, H, W, Cin).to(dtype)
    w = rnd(seed + 2, Cout, Cin, k, k, scale=(2.0 / (Cin * k * k)) ** 0.5)
    b = rnd(seed + 3, Cout, scale=0.1) if use_bias else None
    bn = (t(g.uniform(0.75, 1.25, Cout).astype(np.float32)), rnd(seed + 4, Cout, scale=0.1), rnd(seed + 5, Cout, scale=0.1),
          t(g.uniform(0.5, 1.5, Cout).astype(np.float32)))
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    res = rnd(seed + 6, N, Ho, Wo, Cout).to(dtype) if use_res else None

    def ref(xin):
        y = F.conv2d(xin.cpu().double().permute(0, 3, 1, 2), w.to(dtype).double(), None, padding=pad, dilation=dil)
        gam, bet, mu, var = (v.double() for v in bn)
        sc = gam / torch.sqrt(var + 1e-5)
        sh = bet - mu * sc + (b.double() * sc if use_bias else 0)
        y = y * sc[None, :, None, None] + sh[None, :, None, None]
        if res is not None:
            y = y + res.double().permute(0, 3, 1, 2)
        y = torch.relu(y) if act == "relu" else torch.where(y >= 0, y, SLOPE * y)
        return y.permute(0, 2, 3, 1).contiguous()

    return {"x": x, "w": w, "b": b, "bn": bn, "res": res, "ref": ref, "oshape": (N, Ho, Wo, Cout)}


@functools.lru_cache(maxsize=None)
def packed16(name, dev):
    from arseg_amd import _lib
    from arseg_amd.packing import PackedConv

    N, H, W, Cin, Cout, k, pad, dil, act, use_bn, use_bias, use_res, up2 = CASES16[name]
    c = case16(name, torch.float16)                       # (the fp32 parameters do not depend on the storage dtype)
    return PackedConv(c["w"], c["b"], c["bn"], 1, pad, dil, {"relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU}[act], SLOPE, dev)


def near16(want, dtype):
    return lambda got: close16(got, want, dtype, extra=2e-5 * float(want.abs().max()))


def conv16(pc, cfg, sk=0, up2=False):
    from arseg_amd import ops

    return lambda x, r, o: ops.conv2d(x, pc, residual=r, out=o, tile_cfg=cfg, split_k=sk, up2=up2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["c6", "c6n"])
def test_conv16_dilated_views(dev, name, dtype):
    """Case 6: 3x3 dil 2 pad 2, 64 -> 72, N=2, 9 x 50, bias + BN + PReLU, residual, view A: the automatic plan (cfg 0), tiles 1..4, the
    patch plans 5..8 and 10..13, split-K.  At W = 50 plans 5..8 refuse (the dil-2 halo of their 64-wide tile does not fit) and are held
    to refusing the view as well; the same layer at W = 40 runs them."""
    c, pc = case16(name, dtype), packed16(name, dev)
    x, res = c["x"].to(dev), c["res"].to(dev)
    plans = [(f"cfg{cfg}", conv16(pc, cfg)) for cfg in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13)]
    plans += [(f"cfg{cfg}/{sk}", conv16(pc, cfg, sk)) for cfg, sk in SPLIT_K16]
    refuse = {"c6": ("cfg5", "cfg6", "cfg7", "cfg8"), "c6n": ("cfg10", "cfg12")}[name]       # c6n: the 32-wide tiles 10 / 12 are the default there
    want = c["ref"](c["x"])
    refs = {k: near16(want, dtype) for k in ("cfg0", "cfg1", "cfg5", "cfg11", "cfg3/3")}
    n_run = sweep(plans, x, res, c["oshape"], V16["A"], refs=refs, refuse=refuse)
    assert n_run == {"c6": 12, "c6n": 14}[name]


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv16_up2_views(dev, dtype):
    """Case 7: 3x3 d1, 64 -> 64 on the x2 upsample of [2,7,25,64], view A on x_low and on out: the fused patch plans 5, 7, 10, 11, 13, the
    automatic plan and a pinned tile 1 (resize16 + conv2d16).  Reference: fp64 on the rounded materialised upsample, as the dense test."""
    from arseg_amd import _lib, ops

    c, pc = case16("c7", dtype), packed16("c7", dev)
    x = c["x"].to(dev)
    N, h, w = CASES16["c7"][:3]
    want = c["ref"](ops.resize_nhwc(x, 2 * h, 2 * w, _lib.BILINEAR, False))
    plans = [(f"cfg{cfg}", conv16(pc, cfg, up2=True)) for cfg in (0, 5, 7, 10, 11, 13, 1)]
    refs = {k: near16(want, dtype) for k in ("cfg0", "cfg7", "cfg1")}
    n_run = sweep(plans, x, None, c["oshape"], V16["A"], refs=refs)
    assert n_run == 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv16_1x1_views(dev, dtype):
    """Case 8: 1x1, 128 -> 128, N=2, 7 x 9, BN + ReLU, residual: tiles 1..4 and the automatic plan on view A; the LDS-DMA GEMM
    (gemm_rows16, every tile shape; dense rows are its contract) with an ``out`` and a ``residual`` view.  The automatic plan may be
    "gemm16" for the dense call and falls back to the conv16 kernel for an input view: it is held to the reference, not to dense's bits."""
    from arseg_amd import ops

    c, pc = case16("c8", dtype), packed16("c8", dev)
    x, res = c["x"].to(dev), c["res"].to(dev)
    want = c["ref"](c["x"])
    plans = [(f"cfg{cfg}", conv16(pc, cfg)) for cfg in (0, 1, 2, 3, 4)]
    n_run = sweep(plans, x, res, c["oshape"], V16["A"], refs={k: near16(want, dtype) for k in ("cfg0", "cfg1")}, loose=("cfg0",))
    assert n_run == 5
    rows = [(f"rows{cfg}", (lambda cfg: lambda x_, r, o: ops.gemm_rows16(x_, pc, residual=r, out=o, cfg=cfg))(cfg)) for cfg in range(12)]
    n_run = sweep(rows, x, res, c["oshape"], dict(V16["A"], inp=None), refs={k: near16(want, dtype) for k in ("rows3", "rows9")})
    assert n_run == 12


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv16_refuses_unaligned_out_view(dev, dtype):
    """An ``out`` slice at 4 halves (8 bytes) is not a 16-bit NHWC view the library takes: ArsegError, and nothing written."""
    from arseg_amd import _lib, ops

    c, pc = case16("c8", dtype), packed16("c8", dev)
    x, res = c["x"].to(dev), c["res"].to(dev)
    for cfg in (0, 1):
        wide = torch.full(c["oshape"][:3] + (c["oshape"][3] + 8,), SENTINEL, dtype=dtype, device=dev)
        with pytest.raises(_lib.ArsegError):
            ops.conv2d(x, pc, residual=res, out=wide[..., 4:4 + c["oshape"][3]], tile_cfg=cfg)
        assert bool((wide == SENTINEL).all()), cfg


# ------------------------------------------------------------------------------------------------ cached routes meet a view
def key32(name, dev, math):
    from arseg_amd import _lib

    N, H, W, Cin, Cout, k, pad, dil, act, use_bn, use_bias, use_res, up2 = CASES32[name]
    H, W = (2 * H, 2 * W) if up2 else (H, W)
    return (dev.index, N, H, W, Cin, Cout, k, k, 1, pad, dil, up2, {"f32": _lib.MATH_F32, "f16x3": _lib.MATH_F16X3}[math])


def call_view(name, dev, vname, up2=False):
    """ops.conv2d of case ``name`` on the automatic (cached) plan with view ``vname`` on input, residual and output -> (view result, wide out)."""
    from arseg_amd import ops

    x, res = on_dev(name, dev)
    v = V32[vname]
    _, vx = boxed(x, *v["inp"], NAN)
    vr = None if res is None else boxed(res, *v["res"], NAN)[1]
    wo, vo = boxed(torch.full(case32(name)["oshape"], NAN, device=dev), *v["out"], SENTINEL)
    ops.conv2d(vx, packed32(name, dev), residual=vr, out=vo, up2=up2)
    assert neighbours_intact(wo, v["out"][0], vo.shape[3]), f"view {vname}: wrote outside the output slice"
    return vo


def test_cached_x3_route_meets_views(dev):
    """fp32, "x3" cached for case 3's shape (as a dense first call would): view B is the route's own (16-byte aligned, pitch % 4 == 0) and
    returns dense's bits; view C it refuses -- the call runs the library's heuristic plan for that layout instead of raising."""
    from arseg_amd import ops

    prev = ops.set_conv_math("f16x3")
    try:
        assert ops.gemm_x3_enabled()
        x, res = on_dev("c3", dev)
        with pinned(key32("c3", dev, "f16x3"), "x3"):
            dense = ops.conv2d(x, packed32("c3", dev), residual=res)
            assert torch.equal(call_view("c3", dev, "B"), dense)
            near("c3", TOL)(call_view("c3", dev, "C"))
            assert ops._conv_plans[key32("c3", dev, "f16x3")] == "x3"          # the cached plan stays
    finally:
        ops.set_conv_math(prev)


def test_cached_taps_route_meets_views(dev, conv_math):
    """fp32 up2, "taps" cached for case 5's shape: view B returns dense's bits; view C (odd output pitch; the gather stores 16-byte
    pieces) runs the heuristic plan instead of raising."""
    from arseg_amd import ops

    x, _ = on_dev("c5", dev)
    assert ops._config.sw.UP2_TAPS
    with pinned(key32("c5", dev, conv_math), "taps"):
        dense = ops.conv2d(x, packed32("c5", dev), up2=True)
        near("c5", TOL_TAPS)(dense)
        assert torch.equal(call_view("c5", dev, "B", up2=True), dense)
        near("c5", TOL)(call_view("c5", dev, "C", up2=True))
        assert ops._conv_plans[key32("c5", dev, conv_math)] == "taps"


def test_cached_up2_c64_plan_meets_odd_pitch(dev):
    """fp32 up2, (23, 1) cached for case 5's shape (up_3's persistent kernel stores 16-byte pieces): an ``out`` view of odd pitch runs the
    heuristic plan instead of raising."""
    from arseg_amd import ops

    prev = ops.set_conv_math("f16x3")
    try:
        x, _ = on_dev("c5", dev)
        with pinned(key32("c5", dev, "f16x3"), (23, 1)):
            near("c5", TOL)(ops.conv2d(x, packed32("c5", dev), up2=True))
            near("c5", TOL)(call_view("c5", dev, "C", up2=True))
            assert ops._conv_plans[key32("c5", dev, "f16x3")] == (23, 1)
    finally:
        ops.set_conv_math(prev)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cached_gemm16_route_meets_views(dev, dtype):
    """16-bit, "gemm16" cached for case 8's shape: an input view (in_ld != Cin; the LDS-DMA kernel wants dense rows) takes the conv16
    kernel's heuristic plan and returns the right numbers; an ``out`` view at 4 halves raises, because no 16-bit plan takes it."""
    from arseg_amd import _lib, ops

    c, pc = case16("c8", dtype), packed16("c8", dev)
    N, H, W, Cin, Cout = CASES16["c8"][:5]
    x, res = c["x"].to(dev), c["res"].to(dev)
    key = ("conv16", dev.index, ops._DT16[dtype], N, H, W, Cin, Cout, 1, 1, 1, 0, 1)
    with pinned(key, "gemm16"):
        wx, vx = boxed(x, *V16["A"]["inp"], NAN)
        near16(c["ref"](c["x"]), dtype)(ops.conv2d(vx, pc, residual=res))
        near16(c["ref"](c["x"]), dtype)(ops.conv2d(x, pc, residual=res))
        wide = torch.full((N, H, W, Cout + 8), SENTINEL, dtype=dtype, device=dev)
        with pytest.raises(_lib.ArsegError):
            ops.conv2d(x, pc, residual=res, out=wide[..., 4:4 + Cout])
        assert bool((wide == SENTINEL).all())
        assert ops._conv_plans[key] == "gemm16"
