"""Accuracy of the CReFF kernels ("fp32 on fp16 MFMAs"), plain helper: no pytest, no GPU.

Four of the five CReFF kernels (creff_mfma.hip <16> and <8>, creff_rr.hip, creff_roll.hip) split every operand of both contractions and of
the fused classifier into hi + lo fp16 halves (arseg_split_f16, round toward zero) and promise fp32-grade results; creff.hip is the fp32
arithmetic itself.  This module holds what a test needs to hold a kernel to that promise, on the pattern of tests/split_accuracy.py (whose
``stat``, ``f16_rtz`` and ``split_f16`` it uses):

* the cases (CASES), their seeded inputs under five distributions (DISTS) and two conv gains (GAINS), the heads (HEADS);
* ``yardstick(case, dist, gain)``: ``want`` = the fp64 evaluation of oracle.cpu_ref.my_attention followed by an fp64 1x1 head (and log_softmax
  where the head has one), and ``e32`` = the error against it of the plain float32 loop (``reference32``: both contractions and the head as
  sequential fp32 chains), computed when the test runs;
* ``emulate(case, dist, gain, defect)``: the split arithmetic on the CPU, with the switches DK .. DX that seed the defects the bounds have to catch;
* ``problem(...)``: the bound of a distribution applied to a result.

tests/test_creff_accuracy.py proves on the CPU that the bounds tell right from wrong; tests/test_gpu_creff_accuracy.py holds every route to them.

The distributions.  "normal": standard normal features.  "wide": per-channel powers of two 2^-6 .. 2^6 on both features.  "high": the features
scaled so that max|v| of the fp64 oracle is 5.5e4 (the keyframe feature by s, the LR feature by s / 16 so that the fused feature lr_up + a,
which the classifier splits, stays inside 65504 as well), the key and query conv weights shrunk by the same factors so that the scores are those
of "normal".  "low": features, conv biases and head bias times 2^-8.  "over": as "high" with the value conv replaced by the identity (centre
tap 1, bias 0), so that V is the keyframe feature itself and "V clamped to +-65504 beforehand" is an input one can hand to a kernel (the
feature clamped); a quarter of |V| lies in (65504, 131008], a few values beyond; the LR feature is scaled by s / 512 so that the fused feature
passes 131008, where the classifier's split would clamp it a second time, by less than 2^-10 of it.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import split_accuracy as sa
from split_accuracy import f16_rtz, split_f16, stat  # noqa: F401  (one definition of the split and of the statistic)

# ---------------------------------------------------------------------------------------------------------------- the bounds
# In range ("normal", "wide", "high"): e = max|got - want| / max|want| <= margin * e32, for p and for the logits separately.
# "low":  max|got - want| <= margin * e32 * max|want| + the absolute floor of the format (low_floor).
# "over": against want with V clamped to +-131008, e <= 2^-10 + margin * e32; the same call on the feature clamped to +-65504 meets the
#         in-range bound; nothing is NaN or Inf.
# MARGIN is the conv engine's (split_accuracy.MARGIN): another accumulation order and the one-sided 2^-21 per product of the rtz split.
#
# No margin may exceed half the smallest ratio a seeded defect gives where tests/test_creff_accuracy.py names it on the case.
#
# The CPU emulation of the correct arithmetic, max e / e32 over both gains and both chunk orders (p | logits; e32 = 1.1e-7 .. 1.4e-4), and
# the smallest ratio of a defect named on that case and distribution:
#   case    normal                    wide                       high
#   w64     1.29 | 1.54   DP 156      3.82 | 2.23   DX 12.9      1.25 | 1.56   DV 132
#   w128    0.64 | 0.74   DP 63       5.21 | 1.96   DV 5019      0.62 | 0.72   DW 67
#   f64     1.05 | 1.61   DW 171      2.77 | 2.77   (none named) 1.00 | 1.83   DW 178
# "low": the correct emulation uses at most 0.33 of the bound on p, 0.33 on the 12-class logits, 0.45 on the 19-class logits; DV and DP are
# 8 .. 16 times outside it on p and 1.4 .. 4 times outside it on the 19-class logits.
# "over": at most 0.39 of the bound (0.73 on the fused case's logits), DV 260 .. 520 times outside; clamped to 65504: 0.5 .. 1.6 x e32.
# (The figures measured on an MI355X are in DESIGN.md 5.2.)
MARGIN = sa.MARGIN
# (case id, distribution, gain) -> (margin, reason): holds for p on the kernels that split, not for the logits and not for the fp32 VALU kernel.
# "Half the smallest defect ratio on that case" reads: of the defects NAMED on that case in tests/test_creff_accuracy.py.  On this very row
# (saturated softmax) DK, DQ and DX cannot be seen at any margin -- they emulate at 4.6, 4.7 and 3.8 x e32 against 3.9 for the correct
# arithmetic, the scores' low bits do not reach a one-hot softmax -- and are named on the other distributions of the case.
CASE_MARGINS = {
    ("w128", "wide", 1.0): (8.0, "saturated softmax: p is one value of V plus lr_up, e32 = 1.2e-7 is a single rounding, and what is left is the split's own one-sided "
                                 "rounding, twice -- V's, and that of the un-normalised weight 2^(residue of fl(max log2e)), which 1 / sum only cancels in full "
                                 "precision: up to 2 x 2^-21 = 8.2 x e32.  The CPU emulation of the correct arithmetic is at 3.95 x e32 with the channel chunks "
                                 "ascending and at 5.21 with them descending (another draw of the residues); creff_mfma lands on 5.21."),
}
ROUTE_MARGINS = {}         # (case id or "*", route) -> (margin, reason)
F16_MAX, LO_MAX, FLOOR = 65504.0, 131008.0, 2.0 ** -24
OVER_TERM = 2.0 ** -10     # the 11-bit lo half under round toward zero: a value in (65504, 131008] keeps hi = 65504 and 11 bits of the rest

DISTS = ("normal", "wide", "high", "low", "over")
IN_RANGE = ("normal", "wide", "high")
GAINS = (0.35, 1.0)
HEADS = (0, 12, 19)        # 19: two classifier row blocks
LOGSM = {0: False, 12: True, 19: False}
DEFECTS = ("DK", "DV", "DP", "DQ", "DW", "DX")
WEIGHT_SEED = 7

Case = collections.namedtuple("Case", "id entry C Hp Wp hp wp B")
CASES = [
    Case("w64", "creff", 64, 19, 33, 10, 17, 1),       # ragged against the 16x16 and 8x16 tiles, two tiles each way
    Case("w128", "creff", 128, 19, 33, 10, 17, 1),     # 8 channel chunks, creff_mfma's own range
    Case("f64", "warp", 64, 33, 47, 17, 24, 3),        # the fused kernels: 3 frames, frames 0 and 2 share a keyframe, MVs within +-9 px
]
BY_ID = {c.id: c for c in CASES}


def margin(case_id, dist, gain, route="", out=0):
    """The margin of an output (0: p, else the logits of that head) of a route on a (case, distribution, gain)."""
    r = ROUTE_MARGINS.get((case_id, route), ROUTE_MARGINS.get(("*", route), (MARGIN, "")))[0]
    c = CASE_MARGINS.get((case_id, dist, gain), (MARGIN, ""))[0] if out == 0 and route != "creff:valu" else MARGIN
    return max(MARGIN, c, r)


def max_margin(case_id):
    """The largest margin anything on the case is held to: what every seeded defect has to exceed twice over."""
    return max([MARGIN] + [m for (cid, _, _), (m, _) in CASE_MARGINS.items() if cid == case_id] + [m for (cid, _), (m, _) in ROUTE_MARGINS.items() if cid in (case_id, "*")])


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(case, dist, item):
    return np.random.Generator(np.random.PCG64([ord(ch) for ch in case.id] + [DISTS.index(dist), item]))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))


@functools.lru_cache(maxsize=None)
def _weights(C, gain):
    from arseg_amd import synth
    from arseg_amd.model import MyAttention

    m = synth.load_synth_weights(MyAttention(C, kW=7, kH=7), WEIGHT_SEED, attn_gain=gain)
    return {k: v.clone() for k, v in m.state_dict().items()}


def _warped(c, refs, mvq):
    """the keyframe features [B, C, Hp, Wp] warped as the existing tests do it: the oracle's MV resize and warp, float32"""
    from oracle import cpu_ref

    return torch.cat([cpu_ref.warp_feature(refs[i:i + 1], cpu_ref.mv_resize(cpu_ref.mv_from_int16(mvq[i:i + 1]), c.Hp, c.Wp)) for i in range(c.B)])


def _parts64(sd, hr, lr):
    from oracle import cpu_ref

    return cpu_ref.my_attention({k: v.double() for k, v in sd.items()}, "", hr.double(), lr.double(), 7, 7, return_parts=True)


@functools.lru_cache(maxsize=None)
def inputs(case_id, dist, gain, clamp=False):
    """sd: the float32 state dict of MyAttention; hr [B, C, Hp, Wp]: the (warped) keyframe feature; lr [B, C, hp, wp]; heads {n_cls: (wf, bf)};
    the fused case also refs [B, C, Hp, Wp] (un-warped; frames 0 and 2 share theirs) and mvq int16 [B, Hp, Wp, 2].  clamp ("over" only): the
    keyframe feature clamped to +-65504.  All float32 torch CPU tensors; shared, never written."""
    c = BY_ID[case_id]
    assert dist == "over" or not clamp
    sd = dict(_weights(c.C, gain))
    refs = _gen(c, dist, 0).standard_normal((c.B, c.C, c.Hp, c.Wp))
    lr = _gen(c, dist, 1).standard_normal((c.B, c.C, c.hp, c.wp))
    g = _gen(c, dist, 2)
    heads = {n: (_f32(0.2 * g.standard_normal((n, c.C))), _f32(0.1 * g.standard_normal(n))) for n in HEADS if n}
    mvq = None
    if c.entry == "warp":
        refs[2] = refs[0]
        mvq = (_gen(c, dist, 3).integers(-9, 10, (c.B, c.Hp, c.Wp, 2)) * 4).astype(np.int16)
        mvq[1, : c.Hp // 2] = mvq[1, 0, 0]                        # a block-constant region
        mvq = torch.from_numpy(mvq)
    if dist == "wide":
        scale = np.exp2(_gen(c, dist, 4).integers(-6, 7, (1, c.C, 1, 1)).astype(np.float64))
        refs, lr = refs * scale, lr * scale
    refs, lr = _f32(refs), _f32(lr)
    warp = (lambda r: _warped(c, r, mvq)) if c.entry == "warp" else (lambda r: r)      # noqa: E731
    if dist == "low":
        refs, lr = refs * 2.0 ** -8, lr * 2.0 ** -8
        sd = {k: (v * 2.0 ** -8 if k.endswith(".bias") else v) for k, v in sd.items()}
        heads = {n: (wf, bf * 2.0 ** -8) for n, (wf, bf) in heads.items()}
    if dist in ("high", "over"):
        if dist == "over":
            wv = torch.zeros_like(sd["hr_value_conv.weight"])
            wv[:, 0, 1, 1] = 1.0
            sd["hr_value_conv.weight"], sd["hr_value_conv.bias"] = wv, torch.zeros_like(sd["hr_value_conv.bias"])
            s = F16_MAX / float(np.quantile(warp(refs).abs().numpy(), 0.73))
        else:
            s = 5.5e4 / float(_parts64(sd, warp(refs), lr)[1]["v"].abs().max())
        sl = s / (512.0 if dist == "over" else 16.0)
        refs, lr = _f32(refs.double() * s), _f32(lr.double() * sl)
        sd["hr_key_conv.weight"] = _f32(sd["hr_key_conv.weight"].double() / s)
        sd["lr_query_conv.weight"] = _f32(sd["lr_query_conv.weight"].double() / sl)
    if clamp:
        refs = refs.clamp(-F16_MAX, F16_MAX)
    ins = {"sd": sd, "hr": warp(refs), "lr": lr, "heads": heads}
    if c.entry == "warp":
        ins["refs"], ins["mvq"] = refs, mvq
    if dist in ("high", "over"):
        out, parts = _parts64(sd, ins["hr"], lr)
        av = parts["v"].abs()
        assert float(max(parts["q"].abs().max(), parts["k"].abs().max())) <= 3e4, "keys and queries stay in range"
        if dist == "high" or clamp:          # (clamped: the float32 blend of the warp may pass 65504 by an ulp, the fused feature by lr_up, a few hundred; a low half holds either exactly)
            assert 3e4 < float(av.max()) <= F16_MAX * (1 + 1e-6) and float(out.abs().max()) <= (LO_MAX if clamp else F16_MAX), (float(av.max()), float(out.abs().max()))
        else:
            mid, far = float(((av > F16_MAX) & (av <= LO_MAX)).double().mean()), float((av > LO_MAX).double().mean())
            assert 0.15 <= mid <= 0.35 and 0.0 < far <= 0.06, (mid, far)
    return ins


# ---------------------------------------------------------------------------------------------------------------- want, e32
def _head(p, ins, n_cls, dtype):
    wf, bf = ins["heads"][n_cls]
    lg = F.conv2d(p, wf.to(dtype)[:, :, None, None], bf.to(dtype))
    return F.log_softmax(lg, dim=1) if LOGSM[n_cls] else lg


def reference64(ins, v_clamp=None):
    """{0: p, 12: logits, 19: logits} NCHW float64, max|v|.  v_clamp: V clamped to +-v_clamp before the weighting."""
    from oracle import cpu_ref

    out, parts = _parts64(ins["sd"], ins["hr"], ins["lr"])
    if v_clamp is not None:
        out = parts["lr_up"] + cpu_ref.local_weighting(parts["v"].clamp(-v_clamp, v_clamp), parts["w"], 7, 7)
    res = {0: out}
    for n in HEADS:
        if n:
            res[n] = _head(out, ins, n, torch.float64)
    return res, float(parts["v"].abs().max())


def _fma32(acc, a, b):
    """float32 fma(a, b, acc) on numpy arrays (the product of two float32 is exact in float64)"""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def _upsample32(lr, H, W):
    """bilinear(align_corners=True) of lr [B, C, h, w] to (H, W), every operation a float32 numpy operation"""
    def taps(n_out, n_in):
        src = np.arange(n_out, dtype=np.float32) * (np.float32((n_in - 1) / (n_out - 1)) if n_out > 1 else np.float32(0.0))
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), src - i0.astype(np.float32)

    (y0, y1, ly), (x0, x1, lx) = taps(H, lr.shape[2]), taps(W, lr.shape[3])
    ly, lx, one = ly[:, None], lx[None, :], np.float32(1.0)
    top = (one - lx) * lr[:, :, y0][:, :, :, x0] + lx * lr[:, :, y0][:, :, :, x1]
    bot = (one - lx) * lr[:, :, y1][:, :, :, x0] + lx * lr[:, :, y1][:, :, :, x1]
    return ((one - ly) * top + ly * bot).astype(np.float32)


def _dw32(x, w, b):
    """depthwise 3x3 conv + bias as the kernels run it: acc = bias, then fma over the nine taps in order; numpy float32 [B, C, H, W]"""
    H, W = x.shape[-2:]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.broadcast_to(b.numpy()[None, :, None, None], x.shape).astype(np.float32)
    for t in range(9):
        acc = _fma32(acc, w.numpy()[None, :, 0, t // 3, t % 3, None, None], xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W])
    return acc


def _convs32(ins):
    """lr_up, q, k, v in float32, numpy [B, C, Hp, Wp].  Written out in numpy, not torch's conv and interpolate, because a yardstick has to be
    the same number on every host (torch picks its CPU kernels by the machine it runs on)."""
    sd, hr = ins["sd"], ins["hr"].numpy()
    lr_up = _upsample32(ins["lr"].numpy(), hr.shape[2], hr.shape[3])
    dw = lambda name, x: _dw32(x, sd[name + ".weight"], sd[name + ".bias"])      # noqa: E731
    return lr_up, dw("lr_query_conv", lr_up), dw("hr_key_conv", hr), dw("hr_value_conv", hr)


def _win(x, c0, c1):
    """the zero-padded 7 x 7 windows of channels c0:c1 as float64 [B, c1 - c0, H, W, 49], tap index dy * 7 + dx"""
    xp = np.pad(x[:, c0:c1].astype(np.float64), ((0, 0), (0, 0), (3, 3), (3, 3)))
    w = np.lib.stride_tricks.sliding_window_view(xp, (7, 7), axis=(2, 3))
    return w.reshape(w.shape[:4] + (49,))


def _softmax32(s):
    return torch.softmax(torch.from_numpy(s), dim=-1).numpy()


def _head32(o, ins, n_cls, chain):
    """o [B, C, H, W] float32 numpy -> logits NCHW float32 tensor; chain(A [M, K], B [N, K]) -> [M, N] float32"""
    wf, bf = ins["heads"][n_cls]
    B, C, H, W = o.shape
    lg = chain(o.transpose(0, 2, 3, 1).reshape(-1, C), wf.numpy())
    lg = torch.from_numpy(lg.reshape(B, H, W, n_cls)).permute(0, 3, 1, 2) + bf.view(1, -1, 1, 1)
    return F.log_softmax(lg, dim=1) if LOGSM[n_cls] else lg


def reference32(ins, v_clamp=None):
    """The plain float32 loop, whose error against ``want`` is e32: the convs and the upsample in float32, the scores as the chain
    acc = fma(q_c, k_c, acc) over the channels, torch's float32 softmax, the weighting as the chain over the 49 taps, the head as the chain
    over the channels (split_accuracy.fma_chain).  Torch's pairwise sums would make the yardstick stricter than the plain fp32 loop."""
    lr_up, q, k, v = _convs32(ins)
    if v_clamp is not None:
        v = np.clip(v, -v_clamp, v_clamp)
    B, C, H, W = q.shape
    s = np.zeros((B, H, W, 49), dtype=np.float32)
    for ch in range(C):
        s = (s + q[:, ch, :, :, None].astype(np.float64) * _win(k, ch, ch + 1)[:, 0]).astype(np.float32)
    p = _softmax32(s).astype(np.float64)
    vw = _win(v, 0, C)
    a = np.zeros((B, C, H, W), dtype=np.float32)
    for t in range(49):
        a = (a + p[:, None, :, :, t] * vw[..., t]).astype(np.float32)
    o = lr_up + a
    res = {0: torch.from_numpy(o)}
    for n in HEADS:
        if n:
            res[n] = _head32(o, ins, n, sa.fma_chain)
    return res


Yard = collections.namedtuple("Yard", "want e32 vmax")


@functools.lru_cache(maxsize=None)
def yardstick(case_id, dist, gain, clamp=False, split=True):
    """(want {head: NCHW float64}, e32 {head: float}, max|v|) of a (case, distribution, gain): computed once, shared.  "over": V clamped to
    +-131008 in both (clamp: the feature clamped to +-65504 instead, nothing else; split=False: for a kernel that does not split -- the
    fp32 VALU kernel -- nothing is clamped: "over" is in range for it)."""
    ins = inputs(case_id, dist, gain, clamp)
    vc = LO_MAX if dist == "over" and split and not clamp else None
    want, vmax = reference64(ins, vc)
    got = reference32(ins, vc)
    return Yard(want, {n: stat(got[n], want[n]) for n in HEADS}, vmax)


def low_floor(case_id, gain, n_cls):
    """The absolute term of the "low" bound, from the format alone.
    p, and the logits behind log_softmax (12 classes): 2^-24 (1 + 49 max|v|) -- V's low half has step 2^-24, weighted by sum p = 1; P's low
    half has step 2^-24 against at most 49 taps of |v|.
    Raw logits (19 classes, about 6e-3): the same term plus the head's own splits, which the emulation of the correct arithmetic shows it
    needs.  The fused feature's low half is fp16-subnormal here and is cut toward zero by less than 2^-24 per channel, so a logit moves by
    less than 2^-24 times the larger one-signed part of sum_c |wf[class, c]| (the channels where wf . p is positive, or negative: about
    0.6 of the sum), the largest over pixels and classes; Wf's low half has step 2^-24 against sum_c |p_c|."""
    y = yardstick(case_id, "low", gain)
    fp = FLOOR * (1.0 + 49.0 * y.vmax)
    if n_cls == 0 or LOGSM[n_cls]:
        return fp
    wf, p = inputs(case_id, "low", gain)["heads"][n_cls][0].double(), y.want[0]
    signed = torch.einsum("nc,bchw->bnhw", wf, torch.sign(p)).abs()                      # |S+ - S-| per pixel and class; S+ + S- = sum_c |wf|
    one_signed = float((0.5 * (wf.abs().sum(dim=1).view(1, -1, 1, 1) + signed)).max())
    return fp + FLOOR * (one_signed + float(p.abs().sum(dim=1).max()))


def problem(dist, got, want64, e32, m, floor=0.0, in_range=False):
    """The bound of a distribution applied to one output -> (e, "" or what is wrong).  in_range: "over" on the clamped feature, or on a
    kernel that does not split."""
    got = got.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("nan"), "NaN or Inf in the output"
    e = stat(got, want64)
    if dist == "low":
        err, bound = float((got - want64).abs().max()), m * e32 * float(want64.abs().max()) + floor
        return e, "" if err <= bound else f"max|got - want| = {err:.3g} > {m:g} x e32 x max|want| + floor = {bound:.3g} (floor {floor:.3g})"
    if dist == "over" and not in_range:
        bound = OVER_TERM + m * e32
        return e, "" if e <= bound else f"e = {e:.3g} > 2^-10 + {m:g} x e32 = {bound:.3g}"
    return e, "" if e <= m * e32 else f"e = {e:.3g} > {m:g} x e32 = {m * e32:.3g}"


def bound_of(dist, want64, e32, m, floor=0.0, in_range=False):
    """The bound problem() applies, in the units of e (for the printed tables)."""
    if dist == "low":
        return m * e32 + floor / float(want64.abs().max())
    return (OVER_TERM if dist == "over" and not in_range else 0.0) + m * e32


# ---------------------------------------------------------------------------------------------------------------- the split arithmetic
def _halves(x):
    hi, lo = split_f16(x)
    return hi.astype(np.float64), lo.astype(np.float64)


def _split_chain(A, B, drop_b_lo=False):
    """A [M, K] . B [N, K]^T with both operands split, as the classifier's MFMAs run it: per 16 k, one instruction for a_hi b_hi + a_lo b_lo
    and one for the two cross terms, each an exact sum added to the fp32 accumulator -> float32 [M, N]"""
    (ah, al), (bh, bl) = _halves(A), _halves(B)
    if drop_b_lo:
        bl = np.zeros_like(bl)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for k0 in range(0, A.shape[1], 16):
        s = slice(k0, k0 + 16)
        acc = (acc + (ah[:, s] @ bh[:, s].T + al[:, s] @ bl[:, s].T)).astype(np.float32)
        acc = (acc + (ah[:, s] @ bl[:, s].T + al[:, s] @ bh[:, s].T)).astype(np.float32)
    return acc


LOG2E = np.float32(1.4426950408889634)


def emulate(case_id, dist, gain, defect=None, clamp=False, descending=False):
    """The kernels' arithmetic on the CPU -> {0: p, 12: logits, 19: logits} NCHW float32 tensors.  Q, K, V come from float32 depthwise convs
    and are split by f16_rtz into hi + lo; a product is the four terms hi.hi + lo.lo (one MFMA) and hi.lo + lo.hi (a second one) of
    creff_mfma.hip's header, every MFMA an exact sum added to a float32 accumulator: the scores per chunk of 16 channels, the weighting per
    window row (creff_rr / creff_roll group the same keys into blocks of 16 flat slots: another order of the same sums; descending: the channel chunks
    in descending order, one more order a correct kernel may use).  The softmax is the
    kernels': P = exp2(fma(s, log2e, -fl(max log2e))) in float32, split un-normalised, 1 / sum applied to the weighted sum; then + lr_up, and the head
    with split Wf and a split fused feature.
    defect: DK, DV, DP, DQ, DW: the low half of K, V, P, Q or Wf is lost; DX: the cross term q_lo . k_hi of the scores is dropped."""
    assert defect is None or defect in DEFECTS
    ins = inputs(case_id, dist, gain, clamp)
    lr_up, q, k, v = _convs32(ins)
    B, C, H, W = q.shape
    zero = lambda d, x: np.zeros_like(x) if defect == d else x      # noqa: E731
    (qh, ql), (kh, kl), (vh, vl) = _halves(q), _halves(k), _halves(v)
    ql, kl, vl = zero("DQ", ql), zero("DK", kl), zero("DV", vl)
    s = np.zeros((B, H, W, 49), dtype=np.float32)
    for c0 in (range(C - 16, -1, -16) if descending else range(0, C, 16)):
        qh_, ql_ = qh[:, c0:c0 + 16, :, :, None], ql[:, c0:c0 + 16, :, :, None]
        kh_, kl_ = _win(kh, c0, c0 + 16), _win(kl, c0, c0 + 16)
        s = (s + (qh_ * kh_ + ql_ * kl_).sum(axis=1)).astype(np.float32)
        s = (s + (qh_ * kl_ + (0.0 if defect == "DX" else 1.0) * ql_ * kh_).sum(axis=1)).astype(np.float32)
    m = s.max(axis=-1, keepdims=True)
    with np.errstate(under="ignore"):          # fma(s, log2e, -ml) with ml = fl(max log2e): the largest weight is 2^(rounding residue of ml), not 1
        P = np.exp2((s.astype(np.float64) * np.float64(LOG2E) - (m * LOG2E).astype(np.float64)).astype(np.float32)).astype(np.float32)
    z = P.sum(axis=-1, dtype=np.float32)
    ph, pl = _halves(P)
    pl = zero("DP", pl)
    ph, pl = ph.reshape(B, 1, H, W, 7, 7), pl.reshape(B, 1, H, W, 7, 7)
    vhw, vlw = _win(vh, 0, C).reshape(B, C, H, W, 7, 7), _win(vl, 0, C).reshape(B, C, H, W, 7, 7)
    acc = np.zeros((B, C, H, W), dtype=np.float32)
    for dy in range(7):
        acc = (acc + (ph[..., dy, :] * vhw[..., dy, :] + pl[..., dy, :] * vlw[..., dy, :]).sum(axis=-1)).astype(np.float32)
        acc = (acc + (ph[..., dy, :] * vlw[..., dy, :] + pl[..., dy, :] * vhw[..., dy, :]).sum(axis=-1)).astype(np.float32)
    o = lr_up + acc * (np.float32(1.0) / z)[:, None]
    res = {0: torch.from_numpy(o)}
    for n in HEADS:
        if n:
            res[n] = _head32(o, ins, n, lambda a, b: _split_chain(a, b, defect == "DW"))
    return res
