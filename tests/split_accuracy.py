"""Accuracy of the split-fp16 back end (ARSEG_MATH_F16X3), plain helper: no pytest, no GPU.

Every operand of that back end is split into hi + lo fp16 halves, a product is three fp16 MFMAs accumulated in fp32, and include/arseg_hip.h
promises fp32-grade results.  This module holds what a test needs to hold a kernel to that promise:

* the table of cases (CASES) and their seeded inputs under two distributions, "normal" and "wide";
* ``reference(case, ins, torch.float64)``: the whole operation (optional x2 bilinear upsample, conv, folded BN and bias, residual,
  activation) from the fp32 operands; ``reference32`` is the same in float32, the yardstick: its error against fp64 is ``e32``;
* ``emulate(case, ins, defect)``: the split arithmetic on the CPU (the round-toward-zero split of arseg_split_f16, the weight split of
  arseg_split_weight_f16x3_host, a*b = a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulation in K steps of 16), with the switches D1..D4
  that seed the defects the bound has to catch;
* ``wino(case, ins, ...)``: Winograd F(4x4,3x3) in float32 numpy (the route's own yardstick: its rounding belongs to the algorithm) and
  with its 36 GEMMs in the split arithmetic;
* ``check(got, want64, e32, what, margin)``: e = max|got - want| / max|want| <= margin * e32;
* ``accepted(case, tile_cfg, split_k, math)``: what the library's device-free plan query says about a launch.

tests/test_split_accuracy.py proves on the CPU that the bound tells right from wrong on every case; tests/test_gpu_split_accuracy.py holds
every plan and route to it.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------------------------- the bound
# bound = margin * e32, e32 = the error of the float32 arithmetic on the same inputs (reference32), computed when the test runs.  MARGIN covers
# what a correct kernel may differ by: another accumulation order (three chains of K / 16 steps against one of K) and the 2^-21 per product
# of the round-toward-zero split.  No bound may exceed a third of the smallest error the seeded defects D1, D2, D3 give on the case
# (test_split_accuracy.py asserts it).
#
# Measured on an MI355X: max e / e32 over the cases of a route and both distributions (e32 = 2.0e-7 .. 1.8e-6, 4.7e-6 on case a; the Winograd
# route against its own e32 = 2.6e-6 .. 4.1e-6).  Nothing missed the bound.
#   route                                               margin-4 cases        margin-8 cases (a, j)
#   tile_cfg 1..23, split_k 1                            2.70 (f wide)         3.40 (a wide)
#   the split-K pairs                                    2.70                  3.54
#   f32 back end, ids 0..12                              1.20                  1.21
#   Winograd on plan 7 / 100..106                        1.74, fused up2 1.84  -
#   _conv1x1_x3 fp32 output / split-row output           2.70 / -              3.31 / 2.23
#   taps from split rows / split-row output / fp32 in    0.80 / 0.94 / 0.64    -
#   conv_up2_c64, max_wgs 0 and 3                        0.95                  -
#   psp_bottleneck_x3 fp32 / split-row output            1.88 / 2.24           -
# The CPU emulation of the correct arithmetic: 0.33 .. 1.88 on the margin-4 cases, 2.2 and 3.6 on j and a.
MARGIN = 4.0
# Cases whose margin is larger, with the reason.  Both are 1x1 convs with K = 64: the fp32 loop rounds 64 times, e32 is as small as 2e-7,
# and what is left is the split's own rounding, which is one-sided -- hi and lo are both rounded toward zero, so every product is short by
# up to 2^-21 = 4.8e-7 of itself and the shortfall does not average out over K as round-to-nearest errors do.  The CPU emulation of the
# correct arithmetic -- no kernel -- is at 2.2 and 3.6 x e32 on them (at or below 1.9 on every other case); twice that, to the next
# power of two, is still 30 times below a third of the smallest seeded defect.
_ONE_SIDED = "K = 64: e32 is 64 roundings, the one-sided rtz split (2^-21 per product) dominates; the correct CPU emulation is at {:.1f} x e32"
CASE_MARGINS = {"a": (8.0, _ONE_SIDED.format(3.6) + "; the sigmoid passes the absolute error of the high-gain channels on"),
                "j": (8.0, _ONE_SIDED.format(2.2))}
# (case id or "*", route) -> (margin, reason): the routes whose larger error is inherent to their algorithm.
ROUTE_MARGINS = {}
OLD_TOL = 2e-4          # the absolute tolerance of the older conv tests (test_conv2d and friends): geometry, not precision
SLOPE = 0.2
BN_EPS = 1e-5
DISTS = ("normal", "wide")

Case = collections.namedtuple("Case", "id N H W Cin Cout k stride pad dil act bn bias res up2 psp", defaults=(False, False))
#      id   N  H   W   Cin Cout k  s  p  d  act        bn     bias   res     (up2: H, W are the low-resolution size; the conv runs at 2H x 2W)
CASES = [
    Case("a", 2, 9, 15, 64, 72, 1, 1, 0, 1, "sigmoid", True, False, False),       # K = 64: one 64-step, M = 270, channel tail
    Case("b", 1, 13, 21, 32, 72, 3, 1, 1, 1, "relu", True, False, True),         # K = 288 = 4.5 steps of 64; patch plans at Cin % 32
    Case("c", 1, 11, 26, 64, 136, 3, 1, 2, 2, "prelu", True, True, False),       # dilation, tail against 128-channel tiles
    Case("d", 1, 17, 19, 64, 72, 3, 2, 1, 1, "none", False, True, False),        # stride 2
    Case("e", 1, 33, 47, 3, 64, 7, 2, 3, 1, "relu", True, False, False),         # stem, padded RGB
    Case("f", 1, 13, 21, 64, 264, 1, 1, 0, 1, "none", True, False, True),        # tail against the 256-channel tiles 18, 19
    Case("g", 1, 9, 11, 256, 72, 3, 1, 1, 1, "relu", True, False, True),         # K = 2304, split_k 2 and 3
    Case("h", 1, 6, 50, 32, 72, 3, 1, 1, 1, "prelu", False, True, False),        # map >= 48 wide: the forced-width patch plans 20..22
    Case("i64", 2, 7, 20, 64, 64, 3, 1, 1, 1, "prelu", True, True, False, True),  # fused x2 upsample, up_3's shape class (plan 23)
    Case("i96", 2, 7, 20, 64, 96, 3, 1, 1, 1, "relu", True, False, False, True),  # fused x2 upsample, channel tail
    Case("j", 2, 9, 15, 64, 96, 1, 1, 0, 1, "relu", False, True, True),          # 1x1 with Cout % 32 == 0: the split-row epilogue (out_split)
    Case("p", 2, 9, 13, 64, 64, 1, 1, 0, 1, "relu", False, True, False, False, True),   # folded PSP bottleneck, pyramid (1, 2, 3, 6)
]
BY_ID = {c.id: c for c in CASES}
PSP_SIZES = (1, 2, 3, 6)
PSP_ROWS = sum(s * s for s in PSP_SIZES)
K2304 = "g"
SPLIT_K_PAIRS = ((3, 3), (7, 3), (1, 2), (5, 2), (11, 2), (9, 3), (19, 2))          # the pairs of test_conv2d
DEFECTS = ("D1", "D2", "D3", "D4")


def margin(case_id, route=""):
    """The margin of a route ("tile", "splitk", "f32", "wino", "x3", "x3split", "taps", "tapssplit", "up2_c64", "psp") on a case."""
    r = ROUTE_MARGINS.get((case_id, route), ROUTE_MARGINS.get(("*", route), (MARGIN, "")))[0]
    if route == "wino":          # held to the Winograd yardstick, which the case margins (about torch's direct conv) say nothing about
        return max(MARGIN, r)
    return max(MARGIN, CASE_MARGINS.get(case_id, (MARGIN, ""))[0], r)


def max_margin(case_id, wino=False):
    """The largest margin any route of the case is held to (wino: the Winograd route, which has its own e32)."""
    routes = {route for cid, route in ROUTE_MARGINS if cid in (case_id, "*") and (route == "wino") == wino}
    return max([margin(case_id, "wino" if wino else "tile")] + [margin(case_id, r) for r in routes])


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(case, dist, item):
    return np.random.Generator(np.random.PCG64([ord(ch) for ch in case.id] + [DISTS.index(dist), item]))


def activations(g, dist, shape):
    x = g.standard_normal(shape)
    if dist == "wide":      # the distribution of test_conv2d_f16x3_accuracy: fp16-subnormal low halves, far below the 65504 range limit
        x = x * np.exp(g.uniform(-7, 4.6, shape))
    return torch.from_numpy(x.astype(np.float32))


def out_hw(case):
    H, W = (2 * case.H, 2 * case.W) if case.up2 else (case.H, case.W)
    f = lambda v: (v + 2 * case.pad - case.dil * (case.k - 1) - 1) // case.stride + 1      # noqa: E731
    return f(H), f(W)


@functools.lru_cache(maxsize=None)
def inputs(case_id, dist, gain=True):
    """x NCHW, w OIHW (He-scaled times a per-output-channel gain exp(U(-3, 3))), bn (gamma, beta, mean, var) or None, b or None, res NCHW or
    None; case p: also t [N, rows, Cout], the pyramid terms (they carry the gain of their channel, as W_s . Wconv_s does in the model).
    All float32 torch CPU tensors; shared, never written."""
    c = BY_ID[case_id]
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))      # noqa: E731
    ins = {"x": activations(_gen(c, dist, 0), dist, (c.N, c.Cin, c.H, c.W))}
    g = _gen(c, dist, 1)
    gain = np.exp(g.uniform(-3, 3, (c.Cout, 1, 1, 1))) if gain else np.ones((c.Cout, 1, 1, 1))      # (gain=False: as the older tests draw weights)
    ins["w"] = f32(g.standard_normal((c.Cout, c.Cin, c.k, c.k)) * np.sqrt(2.0 / (c.Cin * c.k * c.k)) * gain)
    g = _gen(c, dist, 2)
    ins["bn"] = (f32(g.uniform(0.5, 1.5, c.Cout)), f32(0.1 * g.standard_normal(c.Cout)), f32(0.1 * g.standard_normal(c.Cout)),
                 f32(g.uniform(0.5, 1.5, c.Cout))) if c.bn else None
    ins["b"] = f32(0.1 * g.standard_normal(c.Cout)) if c.bias else None
    Ho, Wo = out_hw(c)
    ins["res"] = f32(_gen(c, dist, 3).standard_normal((c.N, c.Cout, Ho, Wo))) if c.res else None
    if c.psp:
        ins["t"] = activations(_gen(c, dist, 4), dist, (c.N, PSP_ROWS, c.Cout)) * f32(0.3 * gain.reshape(1, 1, c.Cout))
    return ins


def folded(ins, cout, dtype):
    """(scale, bias) of the folded epilogue in ``dtype`` from the fp32 parameters (arseg_fold_bn_host)."""
    scale, bias = torch.ones(cout, dtype=dtype), torch.zeros(cout, dtype=dtype)
    if ins["b"] is not None:
        bias = ins["b"].to(dtype)
    if ins["bn"] is not None:
        gamma, beta, mean, var = (v.to(dtype) for v in ins["bn"])
        scale = gamma / torch.sqrt(var + BN_EPS)
        bias = beta + (bias - mean) * scale
    return scale, bias


def _act(y, act):
    if act == "relu":
        return F.relu(y)
    if act == "prelu":
        return torch.where(y >= 0, y, y * SLOPE)
    if act == "sigmoid":
        return torch.sigmoid(y)
    return y


def _prior(t, H, W):
    """sum over the pyramid levels of the bilinear (align_corners=False) upsamples of t [N, rows, C] -> NCHW"""
    N, _, C = t.shape
    out, off = torch.zeros(N, C, H, W, dtype=t.dtype), 0
    for s in PSP_SIZES:
        out = out + F.interpolate(t[:, off:off + s * s].reshape(N, s, s, C).permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=False)
        off += s * s
    return out


def _conv_input(c, ins, dtype):
    x = ins["x"].to(dtype)
    return F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=False) if c.up2 else x


def _finish(y, c, ins, dtype):
    """conv result NCHW -> (+ pyramid sum) folded BN and bias, residual, activation -> NHWC"""
    scale, bias = folded(ins, c.Cout, dtype)
    if c.psp:
        y = y + _prior(ins["t"].to(dtype), c.H, c.W)
    y = y * scale.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)
    if ins["res"] is not None:
        y = y + ins["res"].to(dtype)
    return _act(y, c.act).permute(0, 2, 3, 1).contiguous()


def reference(case_id, ins, dtype=torch.float64):
    """The whole operation with torch's own ops in ``dtype`` on the CPU -> NHWC.  float64: what is wanted.  (float32: torch's conv, which
    must itself pass the bound; it is not the yardstick, see reference32.)"""
    c = BY_ID[case_id]
    return _finish(F.conv2d(_conv_input(c, ins, dtype), ins["w"].to(dtype), None, c.stride, c.pad, c.dil), c, ins, dtype)


def fma_chain(A, B):
    """A [M, K] . B [N, K]^T as the plain float32 loop acc = fma(a_k, b_k, acc), k ascending -> float32 [M, N]"""
    A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    acc = np.zeros((A64.shape[0], B64.shape[0]), dtype=np.float32)
    for k in range(A64.shape[1]):
        acc = (acc + np.outer(A64[:, k], B64[:, k])).astype(np.float32)      # (the product of two float32 is exact in float64)
    return acc


def reference32(case_id, ins):
    """The fp32 reference arithmetic, whose error against fp64 is e32: the same operation in float32 on the CPU, the conv as the plain FMA
    loop over K in the order of the packed weights, everything around it torch float32.  The loop, not F.conv2d, because a yardstick has to
    be the same number on every host: on the 1x1 cases and the stem F.conv2d is this loop bit for bit, on the others torch picks blocked
    kernels by the CPU it runs on and its error moved by up to 2.3x between two hosts (1.5e-7 / 3.3e-7 on case b).  The f32 MFMA back end
    lands at 0.75 .. 1.2 x this loop's error on every case."""
    c = BY_ID[case_id]
    A, _ = im2col(_conv_input(c, ins, torch.float32), c)
    Ho, Wo = out_hw(c)
    y = torch.from_numpy(fma_chain(A, pack_weight(ins["w"])).reshape(c.N, Ho, Wo, c.Cout)).permute(0, 3, 1, 2)
    return _finish(y, c, ins, torch.float32)


def stat(got, want64):
    got = got.detach().cpu().double() if torch.is_tensor(got) else torch.from_numpy(np.asarray(got)).double()
    return float(((got - want64).abs().max() / want64.abs().max()).item())      # (a NaN anywhere gives NaN, which passes no bound)


@functools.lru_cache(maxsize=None)
def yardstick(case_id, dist):
    """(want64 NHWC, e32) of a case: computed once, shared."""
    ins = inputs(case_id, dist)
    want = reference(case_id, ins, torch.float64)
    return want, stat(reference32(case_id, ins), want)


def check(got, want64, e32, what, m=MARGIN):
    """e = max|got - want| / max|want| (the statistic of test_conv2d_f16x3_accuracy) must not exceed m * e32 -> e."""
    e = stat(got, want64)
    assert e <= m * e32, f"{what}: e = {e:.3g} > {m:g} x e32 = {m * e32:.3g} (e32 = {e32:.3g})"
    return e


# ---------------------------------------------------------------------------------------------------------------- the split arithmetic
def f16_rtz(x):
    """float32 -> float16 rounded toward zero (v_cvt_pkrtz_f16_f32; f32_to_f16_rtz of the host packer): never reaches infinity."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    h = np.where(np.isinf(h), np.copysign(np.float16(65504.0), h), h).astype(np.float16)
    away = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(away, np.nextafter(h, np.float16(0.0)), h).astype(np.float16)


def split_f16(x):
    """x = hi + lo as arseg_split_f16 forms them: hi = rtz(x), lo = rtz(x - hi) (the difference is exact in fp32)."""
    x = np.asarray(x, dtype=np.float32)
    hi = f16_rtz(x)
    return hi, f16_rtz(x - hi.astype(np.float32))


def weight_exponents(rows):
    """The per-row power of two of arseg_split_weight_f16x3_host: max|row| * 2^e in [16, 32), so that the low halves of the significant
    weights are normal fp16 numbers; undone in the epilogue's scale.  rows [Cout, K]."""
    mx = np.abs(rows).max(axis=1)
    e = 5 - np.frexp(np.where(mx > 0, mx, 1.0))[1]
    return np.where(mx > 0, np.clip(e, -100, 100), 0).astype(np.int32)


def split_gemm(A, B, exps, defect=None, d1_step=None, kreal=None):
    """A [M, K] . (B [N, K] * 2^exps)^T in the split arithmetic -> fp32 [M, N]: three fp16 products per a*b, every product exact, summed in
    fp32 in K steps of 16.  K % 32 == 0; kreal: the part of K that holds data (the rest is padding).

    defect: D1 the activations' low half is lost in one 32-wide K step (``d1_step``, default the middle one);
            D2 the weights' low half is lost in the last K step for the upper half of the output channels;
            D3 the a_lo * b_hi term is lost for the pixels of the last, ragged 64-pixel tile;
            D4 plain fp16 operands (rounded to nearest), one product."""
    A, B = np.asarray(A, dtype=np.float32), np.ldexp(np.asarray(B, dtype=np.float32), np.asarray(exps, dtype=np.int32)[:, None]).astype(np.float32)
    M, K = A.shape
    N = B.shape[0]
    assert K % 32 == 0 and B.shape[1] == K
    kreal = K if kreal is None else kreal
    if defect == "D4":
        ah, al, bh, bl = A.astype(np.float16), None, B.astype(np.float16), None
    else:
        (ah, al), (bh, bl) = split_f16(A), split_f16(B)
    if defect == "D1":
        s = (kreal + 31) // 32 // 2 if d1_step is None else d1_step
        al = al.copy()
        al[:, 32 * s:32 * s + 32] = 0
    elif defect == "D2":
        s = (kreal - 1) // 32
        bl = bl.copy()
        bl[N // 2:, 32 * s:32 * s + 32] = 0
    elif defect == "D3":
        al = al.copy()
        al[(M - 1) // 64 * 64:] = 0
    terms = [(ah.astype(np.float64), bh.astype(np.float64))]
    if defect != "D4":
        terms += [(terms[0][0], bl.astype(np.float64)), (al.astype(np.float64), terms[0][1])]
    acc = np.zeros((M, N), dtype=np.float32)
    for k0 in range(0, K, 16):
        for a, b in terms:
            acc += (a[:, k0:k0 + 16] @ b[:, k0:k0 + 16].T).astype(np.float32)
    return acc


def im2col(x, c):
    """x NCHW float32 (the conv's input) -> A [M, Kpad] with k = (r * S + s) * Cin_pad + ci, the K order of the packed weights (Cin padded to
    4, K padded to 32) -> (A, Kreal)"""
    N, C, H, W = x.shape
    cp = (C + 3) // 4 * 4
    x = F.pad(x, (0, 0, 0, 0, 0, cp - C))
    cols = F.unfold(x, c.k, c.dil, c.pad, c.stride)                                   # [N, cp * k * k, L], (ci, r, s)
    A = cols.reshape(N, cp, c.k * c.k, -1).permute(0, 3, 2, 1).reshape(-1, c.k * c.k * cp).numpy()
    K = A.shape[1]
    return np.pad(A, ((0, 0), (0, -K % 32))), K


def pack_weight(w):
    """w OIHW float32 -> [Cout, Kpad] in the same K order"""
    co, ci, R, S = w.shape
    cp = (ci + 3) // 4 * 4
    B = F.pad(w, (0, 0, 0, 0, 0, cp - ci)).permute(0, 2, 3, 1).reshape(co, R * S * cp).numpy()
    return np.pad(B, ((0, 0), (0, -B.shape[1] % 32)))


def _epilogue32(acc, c, ins, exps):
    """acc [N, Ho, Wo, Cout] fp32 of the pre-scaled weights -> the fp32 epilogue the kernels apply (scale holds 2^-e) -> NHWC tensor"""
    scale, bias = folded(ins, c.Cout, torch.float32)
    y = torch.from_numpy(acc) * (scale * torch.from_numpy(np.ldexp(np.float32(1.0), -exps).astype(np.float32))) + bias
    if ins["res"] is not None:
        y = y + ins["res"].permute(0, 2, 3, 1)
    return _act(y, c.act)


@functools.lru_cache(maxsize=None)
def psp_interp(H, W):
    """B [H * W, 64]: the bilinear interpolation matrix of the pooled rows (what psp_prior_sum applies to an identity), fp32"""
    eye = torch.zeros(1, 64, 64)
    eye[0, torch.arange(PSP_ROWS), torch.arange(PSP_ROWS)] = 1.0
    return _prior(eye[:, :PSP_ROWS], H, W).permute(0, 2, 3, 1).reshape(H * W, 64).numpy()


def emulate(case_id, ins, defect=None):
    """The operation in the split arithmetic on the CPU (the x2 upsample in fp32 before the split) -> NHWC float32 tensor.  Case p: the
    pyramid sum as 64 more K columns of the bottleneck GEMM, [f | B] . [W ; T]^T per image, T un-scaled by the weights' power of two."""
    c = BY_ID[case_id]
    A, kreal = im2col(_conv_input(c, ins, torch.float32), c)
    Bw = pack_weight(ins["w"])
    exps = weight_exponents(Bw)
    Ho, Wo = out_hw(c)
    if not c.psp:
        acc = split_gemm(A, Bw, exps, defect, kreal=kreal)
    else:
        Bi, hw, accs = psp_interp(c.H, c.W), c.H * c.W, []
        for n in range(c.N):
            T = np.zeros((c.Cout, 64), dtype=np.float32)
            T[:, :PSP_ROWS] = ins["t"][n].numpy().T
            accs.append(split_gemm(np.concatenate([A[n * hw:(n + 1) * hw], Bi], axis=1), np.concatenate([Bw, T], axis=1), exps, defect,
                                   kreal=A.shape[1] + PSP_ROWS))
        acc = np.concatenate(accs)
    return _epilogue32(acc.reshape(c.N, Ho, Wo, c.Cout), c, ins, exps)


# ---------------------------------------------------------------------------------------------------------------- Winograd F(4x4, 3x3)
_BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
_G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)
_AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
WINO_SEEDED_GEMM = 7
WINO_VSCALE = 2.0 ** -4          # ops._conv_wino stores the transformed activations scaled by 2^-4 under f16x3 (exact)


def has_wino(c):
    """the convs packing.PackedConv builds Winograd weights for"""
    return c.k == 3 and c.stride == 1 and c.pad == c.dil and c.Cin % 32 == 0 and c.Cin >= 64 and c.Cout % 4 == 0 and not c.psp


def _wino_plane(x, U, gemm):
    """conv3x3 pad 1 of x [N, H, W, C] float32 with transformed weights U [36, Cout, C] -> [N, H, W, Cout] float32, every step in float32"""
    f = np.float32
    N, H, W, C = x.shape
    th, tw = (H + 3) // 4, (W + 3) // 4
    xp = np.zeros((N, 4 * th + 2, 4 * tw + 2, C), dtype=f)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.stack([np.stack([xp[:, i:i + 4 * th:4, j:j + 4 * tw:4] for j in range(6)], axis=0) for i in range(6)], axis=0)      # [6, 6, N, th, tw, C]
    d = d.reshape(6, 6, -1, C)
    BT = _BT.astype(f)
    V = np.einsum("ai,ijtc->ajtc", BT, d).astype(f)
    V = np.einsum("ajtc,bj->abtc", V, BT).astype(f).reshape(36, -1, C)
    Mm = np.stack([gemm(i, V[i], U[i]) for i in range(36)]).reshape(6, 6, -1, U.shape[1])
    AT = _AT.astype(f)
    Y = np.einsum("ai,ijtc->ajtc", AT, Mm).astype(f)
    Y = np.einsum("ajtc,bj->abtc", Y, AT).astype(f)                                   # [4, 4, T, Cout]
    Y = Y.reshape(4, 4, N, th, tw, -1).transpose(2, 3, 0, 4, 1, 5).reshape(N, 4 * th, 4 * tw, -1)
    return Y[:, :H, :W]


def wino(case_id, ins, split=False, defect=None):
    """The conv as Winograd F(4x4,3x3) with the standard matrices, float32 numpy: input transform, 36 GEMMs, output transform; a dilated conv
    on its dil^2 phase images.  split=False: the GEMMs in float32 (the route's own e32).  split=True: the GEMMs in the split arithmetic
    (the transformed activations scaled by 2^-4, the weights by their channel's power of two over the 36 slices); defect "D1" seeds GEMM
    WINO_SEEDED_GEMM of every phase.  -> NHWC float32 tensor"""
    c = BY_ID[case_id]
    assert has_wino(c)
    x = _conv_input(c, ins, torch.float32).permute(0, 2, 3, 1).numpy()
    g = ins["w"].double().numpy()                                                     # [Cout, Cin, 3, 3]
    U = np.einsum("ai,ocij,bj->aboc", _G, g, _G).astype(np.float32).reshape(36, c.Cout, c.Cin)
    exps = np.zeros(c.Cout, dtype=np.int32)
    if split:
        exps = weight_exponents(U.transpose(1, 0, 2).reshape(c.Cout, -1))

        def gemm(i, v, u):
            return split_gemm(v * np.float32(WINO_VSCALE), u, exps, defect if i == WINO_SEEDED_GEMM else None) * np.float32(1.0 / WINO_VSCALE)
    else:
        def gemm(i, v, u):
            return fma_chain(v, u)
    N, H, W, _ = x.shape
    acc = np.zeros((N, H, W, c.Cout), dtype=np.float32)
    for py in range(c.dil):
        for px in range(c.dil):
            acc[:, py::c.dil, px::c.dil] = _wino_plane(np.ascontiguousarray(x[:, py::c.dil, px::c.dil]), U, gemm)
    return _epilogue32(acc, c, ins, exps)


@functools.lru_cache(maxsize=None)
def wino_yardstick(case_id, dist):
    """e32 of the Winograd route on a case: the float32 Winograd's error against fp64"""
    return stat(wino(case_id, inputs(case_id, dist)), yardstick(case_id, dist)[0])


# ---------------------------------------------------------------------------------------------------------------- plan query
def conv_desc(c, tile_cfg, split_k, math):
    """The descriptor ops.conv2d launches for a pinned plan: a plan that does not upsample itself runs on the materialised upsample."""
    from arseg_amd import _lib

    d = _lib.ConvDesc()
    cp = (c.Cin + 3) // 4 * 4
    d.N, d.H, d.W = c.N, (2 * c.H if c.up2 else c.H), (2 * c.W if c.up2 else c.W)
    d.Cin, d.in_ld, d.Cout, d.out_ld, d.res_ld = cp, cp, c.Cout, c.Cout, c.Cout
    d.R, d.S, d.stride, d.pad, d.dil = c.k, c.k, c.stride, c.pad, c.dil
    d.tile_cfg, d.split_k, d.math = tile_cfg, split_k, math
    d.upsample2x = 1 if c.up2 and _lib.conv_plan_row(_lib.CONV_ENGINE_F32, tile_cfg).fuses_upsample else 0
    return d


def accepted(case_id, tile_cfg, split_k, math):
    """Does the library's device-free query (arseg_conv_plan_query) accept the launch?"""
    import ctypes

    from arseg_amd import _lib

    info = _lib.ConvPlanInfo()
    st = _lib.load().arseg_conv_plan_query(_lib.CONV_ENGINE_F32, ctypes.byref(conv_desc(BY_ID[case_id], tile_cfg, split_k, math)), ctypes.byref(info))
    assert st in (_lib.ARSEG_OK, _lib.ARSEG_EUNSUPPORTED, _lib.ARSEG_EINVAL), (case_id, tile_cfg, split_k, math, st)      # (EINVAL: id 23 off its shape class)
    return st == _lib.ARSEG_OK


def conv_cases():
    return [c for c in CASES if not c.psp]
