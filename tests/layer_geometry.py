"""Edge geometries for the small NHWC layers of csrc/layers.hip, plain helper: no pytest, no GPU.

The layer tests elsewhere check a handful of model-like shapes, nearly always on the same side of every host predicate.  This module holds what
a test needs to hold every kernel form of layers.hip to an independent reference at the shapes where such kernels go wrong:

* the table of cases (CASES), each one op in one hazard class (CLASSES), with the storages it runs in and its seeded inputs;
* ``want(case_id, dtype)``: the operation in float64 on the CPU with torch's own operators, on operands rounded to the storage type first;
  ``reference(case_id, dtype, defect=)``: the same from explicit taps and bins (a second statement of it), optionally with one of seven
  value-only models of the indexing bugs the table is there to catch (DEFECTS);
* ``route(case, dtype)``: the labels of the kernel forms the host code of layers.hip picks for the case -- from the library's device-free
  workspace queries where one decides it, otherwise a mirror of the predicate (each mirror names the function it restates);
* ``bound(case, dtype, want)``: the bound of the op's older test (tests/test_gpu_ops.py, test_gpu_16bit.py, test_gpu_psp16.py), and for the
  heads the derived one.

tests/test_layer_geometry.py proves on the CPU that the table has teeth and that the sweep cannot pass vacuously;
tests/test_gpu_layer_geometry.py runs it on the device."""
import collections
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

CLASSES = ("thresholds", "tiny", "image_straddle", "views", "nonsquare_ratio", "grid_wrap")
DEFECTS = ("seg_offset", "image_straddle", "ld_as_c", "floor_bin", "no_clamp", "band_tail", "sibling_unwritten")
DEFECT_CLASS = {"seg_offset": "thresholds", "image_straddle": "image_straddle", "ld_as_c": "views", "floor_bin": "nonsquare_ratio",
                "no_clamp": "nonsquare_ratio", "band_tail": "thresholds", "sibling_unwritten": "thresholds"}
DTYPES = {"f32": None, "fp16": torch.float16, "bf16": torch.bfloat16}
ALL, F32, D16 = ("f32", "fp16", "bf16"), ("f32",), ("fp16", "bf16")
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}          # tests/test_gpu_16bit.py
U8_MEAN, U8_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MIB = 1 << 20
MAX_TENSOR_BYTES = 64 * MIB
# The two capped grids whose second trip starts exactly at a 64 MiB fp32 tensor (cap x 256 threads x 16 or 32 bytes per thread): their cases
# are a few rows past it.
OVERSIZE = {"gw_nchw_x4": 64 << 10, "gw_cast16": 16 << 10, "gw_cast32": 16 << 10}
# arseg_grid_for's caps (csrc/arseg_common.h: 8192 by default) as the launches of layers.hip set them, in work items of one thread each
GRID_CAP = 8192

# the ops a class applies to: every class holds every one of its ops (tests/test_layer_geometry.py)
APPLIES = {
    "thresholds": ("adaptive_avgpool", "psp_pool_matrix", "psp_prior_sum", "global_reduce", "resize_nhwc", "resize_nchw", "head", "frame_ingest"),
    "tiny": ("maxpool3x3s2", "adaptive_avgpool", "psp_pool_matrix", "psp_prior_sum", "global_reduce", "resize_nhwc", "resize_nchw", "scale_add", "head",
             "frame_ingest", "frame_u8_to_nhwc4", "to_nhwc", "to_nchw_contiguous", "cast"),
    "image_straddle": ("global_reduce", "resize_nhwc", "resize_nchw", "scale_add", "head", "to_nhwc", "to_nchw_contiguous"),
    "views": ("adaptive_avgpool", "psp_pool_matrix", "global_reduce", "resize_nhwc", "head"),
    "nonsquare_ratio": ("maxpool3x3s2", "adaptive_avgpool", "psp_pool_matrix", "psp_prior_sum", "resize_nhwc", "resize_nchw", "frame_ingest", "frame_u8_to_nhwc4"),
    "grid_wrap": ("maxpool3x3s2", "psp_prior_sum", "resize_nhwc", "resize_nchw", "scale_add", "head", "frame_ingest", "frame_u8_to_nhwc4", "cast"),
}
OPS = tuple(dict.fromkeys(op for ops_ in APPLIES.values() for op in ops_))

Case = collections.namedtuple("Case", "id op cls dtypes p")


def _c(id_, op, cls, dtypes, **p):
    return Case(id_, op, cls, dtypes, p)


def _table():
    t = []
    PSP = (1, 2, 3, 6)
    # ------------------------------------------------------------------------------------------------ thresholds: both sides of every host predicate
    # arseg_global_reduce_fwd: N * ceil(C / 16) < 256 takes the 256-lane form, otherwise the 64-lane one
    for rop in ("mean", "max"):
        t += [_c(f"gr_w255_{rop}", "global_reduce", "thresholds", ALL, N=3, H=3, W=5, C=1360, rop=rop),
              _c(f"gr_w256_{rop}", "global_reduce", "thresholds", ALL, N=4, H=3, W=5, C=1024, rop=rop),
              # global_parts: two stages need H W >= 2048 (2047 = 23 x 89) and N * ceil(C / 16) < 64; 45 x 47 = 2115 pixels in 8 uneven bands
              _c(f"gr_hw2047_{rop}", "global_reduce", "thresholds", ALL, N=1, H=23, W=89, C=64, rop=rop),
              _c(f"gr_hw2048_{rop}", "global_reduce", "thresholds", ALL, N=1, H=32, W=64, C=64, rop=rop),
              _c(f"gr_b63_{rop}", "global_reduce", "thresholds", ALL, N=1, H=45, W=47, C=1008, rop=rop),
              _c(f"gr_b64_{rop}", "global_reduce", "thresholds", ALL, N=1, H=45, W=47, C=1024, rop=rop),
              # mean16_slices: one slice (H W <= 64) and several; C = 264 and 512: more than one block of 256 channels, one of them partial
              _c(f"gr_c264_{rop}", "global_reduce", "thresholds", ALL, N=2, H=9, W=13, C=264, rop=rop),
              _c(f"gr_c512_{rop}", "global_reduce", "thresholds", ALL, N=1, H=5, W=7, C=512, rop=rop)]
    # arseg_adaptive_avgpool_fwd: a grid of 255 against 256 workgroups (bins x ceil(C / 16) x N)
    t += [_c("ap_g255", "adaptive_avgpool", "thresholds", F32, N=1, H=7, W=9, C=272, oh=3, ow=5),
          _c("ap_g256", "adaptive_avgpool", "thresholds", F32, N=1, H=7, W=9, C=256, oh=4, ow=4)]
    # ops.psp_pool_matrix: one pass up to 4 levels of size <= 6, the block-row fallback beyond; arseg_adaptive_avgpool_blockrow_fwd's four forms
    t += [_c("pm_op", "psp_pool_matrix", "thresholds", ALL, N=2, H=9, W=13, C=64, sizes=PSP),
          _c("pm_op6", "psp_pool_matrix", "thresholds", ALL, N=1, H=4, W=4, C=32, sizes=(6,)),
          _c("pm_fb64", "psp_pool_matrix", "thresholds", F32, N=1, H=9, W=13, C=64, sizes=(1, 2, 3, 6, 8)),
          _c("pm_fb512", "psp_pool_matrix", "thresholds", F32, N=1, H=9, W=13, C=512, sizes=(8,)),
          _c("pm_fb68", "psp_pool_matrix", "thresholds", F32, N=1, H=9, W=13, C=68, sizes=(8,)),
          _c("pm_s7c64", "psp_pool_matrix", "thresholds", F32, N=2, H=9, W=13, C=64, sizes=(7,)),
          _c("pm_s7c512", "psp_pool_matrix", "thresholds", F32, N=2, H=9, W=13, C=512, sizes=(7,)),
          _c("pm_s7c68", "psp_pool_matrix", "thresholds", F32, N=2, H=9, W=13, C=68, sizes=(7,))]
    # psp_prior_sum: the fp32 row walk from N * H * (C / 4) = 49152; W = 1; a map smaller than the largest level; fewer than four levels
    t += [_c("pr_rw", "psp_prior_sum", "thresholds", ALL, N=2, H=96, W=5, C=1024, sizes=PSP),
          _c("pr_px", "psp_prior_sum", "thresholds", ALL, N=2, H=95, W=5, C=1024, sizes=PSP),
          _c("pr_w1", "psp_prior_sum", "thresholds", ALL, N=2, H=96, W=1, C=1024, sizes=PSP),
          _c("pr_small", "psp_prior_sum", "thresholds", ALL, N=48, H=4, W=5, C=1024, sizes=PSP),
          _c("pr_rw2", "psp_prior_sum", "thresholds", ALL, N=2, H=96, W=7, C=1024, sizes=(2, 5))]
    # arseg_head_fwd: C % 8 and C <= 64 / <= 128 (the two matrix-core kernels), n_cls <= 12 / <= 19 / <= 32 (the generic one)
    for i, (C, n_cls, lsm) in enumerate(((8, 1, False), (64, 12, True), (72, 13, False), (128, 19, True), (136, 20, False), (12, 32, True), (512, 19, True),
                                         (12, 12, False), (12, 13, True), (20, 1, True), (64, 32, False), (136, 19, True), (20, 20, False))):
        t.append(_c(f"hd_c{C}n{n_cls}", "head", "thresholds", F32, N=1 if C == 512 else 2, H=5, W=7, C=C, n_cls=n_cls, lsm=lsm))
    # arseg_head16_fwd: C % 64 and C <= 512 (the chunked matrix-core kernel)
    for C, n_cls, lsm in ((64, 19, True), (128, 12, False), (512, 32, True), (576, 20, False), (24, 5, True), (24, 13, False), (576, 12, True)):
        t.append(_c(f"h16_c{C}n{n_cls}", "head", "thresholds", D16, N=1 if C >= 512 else 2, H=5, W=7, C=C, n_cls=n_cls, lsm=lsm))
    # arseg_resize_fwd, NHWC: the x2 fast path against Hout = 2 Hin with Wout = 2 Win +- 1, and align_corners at x2
    t += [_c("rs_x2", "resize_nhwc", "thresholds", ALL, N=2, Hin=5, Win=7, C=8, Hout=10, Wout=14, mode="bilinear", align=False),
          _c("rs_x2p", "resize_nhwc", "thresholds", ALL, N=2, Hin=5, Win=7, C=8, Hout=10, Wout=15, mode="bilinear", align=False),
          _c("rs_x2m", "resize_nhwc", "thresholds", ALL, N=2, Hin=5, Win=7, C=8, Hout=10, Wout=13, mode="bilinear", align=False),
          _c("rs_x2a", "resize_nhwc", "thresholds", ALL, N=2, Hin=5, Win=7, C=8, Hout=10, Wout=14, mode="bilinear", align=True)]
    # ... NCHW: Wout = 8 Win, 16 Win (runs), 4 k (four outputs per thread), 4 k + 1 (one), each under both align_corners
    for name, Hin, Win, Hout, Wout in (("r8", 3, 5, 7, 40), ("r16", 2, 3, 5, 48), ("4k", 5, 7, 6, 12), ("4k1", 5, 7, 6, 13)):
        for al in (False, True):
            t.append(_c(f"rn_{name}{'a' if al else ''}", "resize_nchw", "thresholds", F32, N=2, C=3, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, mode="bilinear", align=al))
    # arseg_frame_to_nhwc4_fwd / arseg_frame_to_nhwc8_16_fwd: W % 4, h, w == H, W, the staged span 255 sx + 8 <= 1056 (sx = 1051 / 256 under,
    # 1055 / 256 over), 256-pixel segments (w = 255, 256, 257, 513), upscales.
    # WIDE RATIOS.  The kernels form the source coordinate in fp32, as ATen does: scale x dst carries the rounding of the scale (2^-24 relative)
    # and of the product (half an ulp of the coordinate), 3e-5 of a pixel at a coordinate of 600 -- times the difference of two unit-normal
    # neighbours, that alone is several times the 1e-5 of the older tests, which never left maps 48 pixels wide (first run on an MI355X:
    # W = 600 -> w = 255 and 256 missed it by 5.7 x and 8.2 x in fp32 storage, W = 600 -> 257, whose ratio 599 / 256 is exact, met it).  The
    # float64 reference cannot follow the fp32 coordinate, so every case wider than a hundred pixels or so, here and in grid_wrap, has a
    # ratio that fp32 holds exactly (a denominator that is a power of two, or 2.5, 1, 0.5, 0.25): the coordinates are then exact in
    # both precisions and the bound measures the blend alone.
    t += [_c("fi_w4", "frame_ingest", "thresholds", ALL, N=2, H=12, W=16, h=6, w=8),
          _c("fi_w4n", "frame_ingest", "thresholds", ALL, N=2, H=12, W=18, h=6, w=9),
          _c("fi_same", "frame_ingest", "thresholds", ALL, N=2, H=6, W=8, h=6, w=8),
          _c("fi_span_u", "frame_ingest", "thresholds", ALL, N=1, H=3, W=1052, h=2, w=257),
          _c("fi_span_o", "frame_ingest", "thresholds", ALL, N=1, H=3, W=1056, h=2, w=257),
          _c("fi_w255", "frame_ingest", "thresholds", ALL, N=1, H=4, W=636, h=3, w=255),
          _c("fi_w256", "frame_ingest", "thresholds", ALL, N=1, H=4, W=256, h=3, w=256),
          _c("fi_w257", "frame_ingest", "thresholds", ALL, N=1, H=4, W=600, h=3, w=257),
          _c("fi_w513", "frame_ingest", "thresholds", ALL, N=2, H=5, W=1200, h=3, w=513),
          _c("fi_up", "frame_ingest", "thresholds", ALL, N=1, H=5, W=8, h=9, w=20),
          _c("fi_up_px", "frame_ingest", "thresholds", ALL, N=1, H=5, W=7, h=9, w=20),
          _c("fi_up2seg", "frame_ingest", "thresholds", ALL, N=1, H=3, W=40, h=4, w=313),
          _c("fi_up3seg", "frame_ingest", "thresholds", ALL, N=1, H=2, W=64, h=3, w=513)]
    # ------------------------------------------------------------------------------------------------ tiny: one pixel, one vector, sizes of 1
    t += [_c("mp_1x1", "maxpool3x3s2", "tiny", ALL, N=1, H=1, W=1, C=8), _c("mp_1x5", "maxpool3x3s2", "tiny", ALL, N=2, H=1, W=5, C=8),
          _c("mp_c4", "maxpool3x3s2", "tiny", F32, N=2, H=2, W=1, C=4),
          _c("ap_t", "adaptive_avgpool", "tiny", F32, N=1, H=1, W=1, C=4, oh=1, ow=1),
          _c("ap_tbig", "adaptive_avgpool", "tiny", F32, N=1, H=2, W=3, C=8, oh=4, ow=5),
          _c("pm_t", "psp_pool_matrix", "tiny", ALL, N=1, H=1, W=1, C=8, sizes=PSP),          # a map smaller than the pyramid level
          _c("pm_t7", "psp_pool_matrix", "tiny", F32, N=1, H=2, W=2, C=4, sizes=(7,)),
          _c("pr_t", "psp_prior_sum", "tiny", ALL, N=1, H=1, W=1, C=8, sizes=PSP),
          _c("pr_t2", "psp_prior_sum", "tiny", ALL, N=1, H=2, W=3, C=8, sizes=(6,)),
          _c("gr_t_mean", "global_reduce", "tiny", ALL, N=1, H=1, W=1, C=8, rop="mean"), _c("gr_t_max", "global_reduce", "tiny", ALL, N=1, H=1, W=1, C=8, rop="max"),
          _c("gr_t4_max", "global_reduce", "tiny", F32, N=1, H=1, W=3, C=4, rop="max"),
          _c("rs_t11", "resize_nhwc", "tiny", ALL, N=1, Hin=1, Win=1, C=8, Hout=1, Wout=1, mode="bilinear", align=True),
          _c("rs_t1up", "resize_nhwc", "tiny", ALL, N=1, Hin=1, Win=1, C=8, Hout=3, Wout=5, mode="bilinear", align=False),
          _c("rs_t1a", "resize_nhwc", "tiny", ALL, N=1, Hin=3, Win=4, C=8, Hout=1, Wout=1, mode="bilinear", align=True),          # align_corners scale 0
          _c("rs_t1w", "resize_nhwc", "tiny", ALL, N=1, Hin=3, Win=4, C=8, Hout=5, Wout=1, mode="bilinear", align=True),
          _c("rs_tn", "resize_nhwc", "tiny", ALL, N=1, Hin=1, Win=1, C=8, Hout=2, Wout=3, mode="nearest", align=False),
          _c("rs_t1x2", "resize_nhwc", "tiny", ALL, N=1, Hin=1, Win=1, C=8, Hout=2, Wout=2, mode="bilinear", align=False),
          _c("rs_tc4", "resize_nhwc", "tiny", F32, N=1, Hin=1, Win=2, C=4, Hout=2, Wout=4, mode="bilinear", align=False),
          _c("rn_t", "resize_nchw", "tiny", F32, N=1, C=1, Hin=1, Win=1, Hout=1, Wout=1, mode="bilinear", align=True),
          _c("rn_t8", "resize_nchw", "tiny", F32, N=1, C=1, Hin=1, Win=1, Hout=3, Wout=8, mode="bilinear", align=False),
          _c("rn_t16", "resize_nchw", "tiny", F32, N=1, C=1, Hin=2, Win=1, Hout=1, Wout=16, mode="bilinear", align=False),
          _c("rn_t4", "resize_nchw", "tiny", F32, N=1, C=1, Hin=3, Win=5, Hout=1, Wout=4, mode="bilinear", align=True),
          _c("rn_tn", "resize_nchw", "tiny", F32, N=1, C=2, Hin=1, Win=1, Hout=2, Wout=3, mode="nearest", align=False),
          _c("sa_t", "scale_add", "tiny", ALL, N=1, H=1, W=1, C=8, full=True, vec=True), _c("sa_t2", "scale_add", "tiny", ALL, N=2, H=1, W=1, C=8, full=False, vec=False),
          _c("sa_tc4", "scale_add", "tiny", F32, N=1, H=1, W=2, C=4, full=False, vec=True),
          _c("hd_t64", "head", "tiny", ALL, N=1, H=2, W=3, C=64, n_cls=12, lsm=True),          # N H W < 32: one partial tile
          _c("hd_t128", "head", "tiny", ALL, N=1, H=1, W=1, C=128, n_cls=19, lsm=False),
          _c("hd_t12", "head", "tiny", F32, N=1, H=1, W=5, C=12, n_cls=5, lsm=True), _c("hd_t4", "head", "tiny", F32, N=1, H=1, W=1, C=4, n_cls=20, lsm=False),
          _c("hd_t4n13", "head", "tiny", F32, N=1, H=3, W=1, C=4, n_cls=13, lsm=True),
          _c("h16_t8", "head", "tiny", D16, N=1, H=1, W=1, C=8, n_cls=3, lsm=True), _c("h16_t24", "head", "tiny", D16, N=1, H=1, W=5, C=24, n_cls=32, lsm=False),
          _c("h16_t8n19", "head", "tiny", D16, N=1, H=3, W=1, C=8, n_cls=19, lsm=True),
          _c("fi_t11", "frame_ingest", "tiny", ALL, N=1, H=1, W=1, h=1, w=1), _c("fi_th1", "frame_ingest", "tiny", ALL, N=1, H=3, W=4, h=1, w=1),
          _c("fi_tw1", "frame_ingest", "tiny", ALL, N=1, H=4, W=5, h=3, w=1), _c("fi_tW1", "frame_ingest", "tiny", ALL, N=2, H=1, W=1, h=2, w=3),
          _c("fu_t11", "frame_u8_to_nhwc4", "tiny", F32, N=1, H=1, W=1, h=1, w=1), _c("fu_t", "frame_u8_to_nhwc4", "tiny", F32, N=1, H=3, W=4, h=1, w=1),
          _c("fu_same", "frame_u8_to_nhwc4", "tiny", F32, N=2, H=1, W=5, h=1, w=5), _c("fu_tW1", "frame_u8_to_nhwc4", "tiny", F32, N=2, H=1, W=1, h=2, w=3),
          _c("tn_t", "to_nhwc", "tiny", F32, N=1, C=3, H=1, W=5), _c("tn_t1", "to_nhwc", "tiny", F32, N=2, C=5, H=1, W=1),
          _c("tc_t", "to_nchw_contiguous", "tiny", F32, N=1, C=3, H=1, W=5), _c("tc_t1", "to_nchw_contiguous", "tiny", F32, N=2, C=1, H=1, W=1),
          _c("ct_t16", "cast", "tiny", D16, count=8, to="16"), _c("ct_t32", "cast", "tiny", D16, count=8, to="32")]
    # ------------------------------------------------------------------------------------------------ image_straddle: N >= 3, H W coprime to 32 and 256
    t += [_c("gr_s33_mean", "global_reduce", "image_straddle", ALL, N=3, H=3, W=11, C=16, rop="mean"),
          _c("gr_s143_max", "global_reduce", "image_straddle", ALL, N=3, H=11, W=13, C=24, rop="max"),
          _c("gr_s257_max", "global_reduce", "image_straddle", ALL, N=5, H=1, W=257, C=832, rop="max"),          # 5 x 52 = 260 workgroups: the 64-lane max
          _c("gr_s257_mean", "global_reduce", "image_straddle", ALL, N=5, H=1, W=257, C=832, rop="mean"),
          _c("rs_s33", "resize_nhwc", "image_straddle", ALL, N=3, Hin=2, Win=5, C=8, Hout=3, Wout=11, mode="bilinear", align=False),
          _c("rs_s143", "resize_nhwc", "image_straddle", ALL, N=3, Hin=6, Win=7, C=8, Hout=11, Wout=13, mode="bilinear", align=True),
          _c("rs_s257", "resize_nhwc", "image_straddle", ALL, N=3, Hin=3, Win=90, C=8, Hout=1, Wout=257, mode="nearest", align=False),
          _c("rs_sup2", "resize_nhwc", "image_straddle", ALL, N=3, Hin=3, Win=5, C=8, Hout=6, Wout=10, mode="bilinear", align=False),
          _c("rn_s33", "resize_nchw", "image_straddle", F32, N=3, C=1, Hin=2, Win=5, Hout=3, Wout=11, mode="bilinear", align=False),
          _c("rn_s143", "resize_nchw", "image_straddle", F32, N=2, C=2, Hin=6, Win=7, Hout=11, Wout=13, mode="bilinear", align=True),
          _c("rn_s257", "resize_nchw", "image_straddle", F32, N=3, C=1, Hin=3, Win=90, Hout=1, Wout=257, mode="nearest", align=False),
          _c("rn_sx4", "resize_nchw", "image_straddle", F32, N=3, C=2, Hin=3, Win=5, Hout=7, Wout=12, mode="bilinear", align=False),
          _c("rn_sr8", "resize_nchw", "image_straddle", F32, N=3, C=2, Hin=3, Win=3, Hout=5, Wout=24, mode="bilinear", align=False),
          _c("rn_sr16", "resize_nchw", "image_straddle", F32, N=3, C=1, Hin=3, Win=2, Hout=5, Wout=32, mode="bilinear", align=False),
          _c("sa_s33", "scale_add", "image_straddle", ALL, N=3, H=3, W=11, C=8, full=True, vec=True),
          _c("sa_s257", "scale_add", "image_straddle", ALL, N=3, H=1, W=257, C=8, full=False, vec=True),
          _c("tn_s33", "to_nhwc", "image_straddle", F32, N=3, C=33, H=3, W=11), _c("tc_s33", "to_nchw_contiguous", "image_straddle", F32, N=3, C=33, H=3, W=11),
          # every head route: the two matrix-core kernels of fp32 storage, the chunked one of 16-bit storage at C = 64 and above, the generic ones
          _c("hd_s33c64", "head", "image_straddle", ALL, N=3, H=3, W=11, C=64, n_cls=19, lsm=True),
          _c("hd_s143c128", "head", "image_straddle", ALL, N=3, H=11, W=13, C=128, n_cls=19, lsm=True),
          _c("hd_s257c72", "head", "image_straddle", F32, N=3, H=1, W=257, C=72, n_cls=12, lsm=False),
          _c("hd_s33c12", "head", "image_straddle", F32, N=3, H=3, W=11, C=12, n_cls=5, lsm=True),
          _c("hd_s143c20", "head", "image_straddle", F32, N=3, H=11, W=13, C=20, n_cls=19, lsm=False),
          _c("hd_s33c12n32", "head", "image_straddle", F32, N=3, H=3, W=11, C=12, n_cls=32, lsm=True),
          _c("h16_s33c512", "head", "image_straddle", D16, N=3, H=3, W=11, C=512, n_cls=12, lsm=False),
          _c("h16_s257c192", "head", "image_straddle", D16, N=3, H=1, W=257, C=192, n_cls=19, lsm=True),
          _c("h16_s33c24", "head", "image_straddle", D16, N=3, H=3, W=11, C=24, n_cls=5, lsm=True),
          _c("h16_s143c24", "head", "image_straddle", D16, N=3, H=11, W=13, C=24, n_cls=19, lsm=False),
          _c("h16_s33c24n32", "head", "image_straddle", D16, N=3, H=3, W=11, C=24, n_cls=32, lsm=True)]
    # ------------------------------------------------------------------------------------------------ views: channel slices of wider buffers
    t += [_c("ap_v", "adaptive_avgpool", "views", F32, N=2, H=6, W=7, C=16, oh=2, ow=3, wide=True),          # into rows of a wider matrix
          _c("ap_v64", "adaptive_avgpool", "views", F32, N=2, H=6, W=7, C=256, oh=3, ow=3, wide=True),
          _c("ap_vd", "adaptive_avgpool", "views", F32, N=2, H=5, W=4, C=8, oh=2, ow=2),
          _c("pm_v", "psp_pool_matrix", "views", ALL, N=2, H=7, W=5, C=16, sizes=PSP),
          _c("pm_vfb", "psp_pool_matrix", "views", F32, N=2, H=7, W=5, C=64, sizes=(2, 7)),
          _c("gr_v_mean", "global_reduce", "views", ALL, N=2, H=5, W=7, C=16, rop="mean"), _c("gr_v_max", "global_reduce", "views", ALL, N=2, H=5, W=7, C=16, rop="max"),
          _c("gr_v2_mean", "global_reduce", "views", ALL, N=1, H=45, W=47, C=64, rop="mean"),          # the two-stage form on a slice
          _c("rs_v", "resize_nhwc", "views", ALL, N=2, Hin=5, Win=7, C=8, Hout=9, Wout=11, mode="bilinear", align=False),
          _c("rs_va", "resize_nhwc", "views", ALL, N=2, Hin=5, Win=7, C=16, Hout=4, Wout=11, mode="bilinear", align=True),
          _c("rs_vup2", "resize_nhwc", "views", ALL, N=2, Hin=3, Win=5, C=8, Hout=6, Wout=10, mode="bilinear", align=False),
          _c("rs_vn", "resize_nhwc", "views", ALL, N=2, Hin=3, Win=5, C=8, Hout=7, Wout=4, mode="nearest", align=False),
          _c("hd_v64", "head", "views", ALL, N=2, H=5, W=7, C=64, n_cls=19, lsm=True),
          _c("hd_v128", "head", "views", ALL, N=3, H=3, W=11, C=128, n_cls=12, lsm=False),
          _c("hd_v12", "head", "views", F32, N=2, H=5, W=7, C=12, n_cls=5, lsm=True),
          _c("h16_v24", "head", "views", D16, N=2, H=5, W=7, C=24, n_cls=13, lsm=True)]
    # ------------------------------------------------------------------------------------------------ nonsquare_ratio: a ratio per axis, overlapping bins
    t += [_c("mp_n1", "maxpool3x3s2", "nonsquare_ratio", ALL, N=2, H=7, W=10, C=8), _c("mp_n2", "maxpool3x3s2", "nonsquare_ratio", ALL, N=1, H=10, W=3, C=16),
          _c("ap_n1", "adaptive_avgpool", "nonsquare_ratio", F32, N=2, H=7, W=10, C=8, oh=3, ow=4),
          _c("ap_n2", "adaptive_avgpool", "nonsquare_ratio", F32, N=1, H=3, W=4, C=8, oh=5, ow=6),          # more bins than pixels
          _c("pm_n1", "psp_pool_matrix", "nonsquare_ratio", ALL, N=2, H=7, W=10, C=8, sizes=(2, 5)),
          _c("pm_n2", "psp_pool_matrix", "nonsquare_ratio", ALL, N=1, H=5, W=11, C=16, sizes=PSP),
          _c("pm_n7", "psp_pool_matrix", "nonsquare_ratio", F32, N=1, H=10, W=5, C=8, sizes=(3, 7)),
          _c("pr_n1", "psp_prior_sum", "nonsquare_ratio", ALL, N=2, H=7, W=10, C=8, sizes=(2, 5)),
          _c("pr_n2", "psp_prior_sum", "nonsquare_ratio", ALL, N=1, H=13, W=4, C=16, sizes=PSP),
          _c("rs_n1", "resize_nhwc", "nonsquare_ratio", ALL, N=2, Hin=7, Win=10, C=8, Hout=4, Wout=23, mode="bilinear", align=False),
          _c("rs_n2", "resize_nhwc", "nonsquare_ratio", ALL, N=1, Hin=9, Win=4, C=8, Hout=13, Wout=3, mode="bilinear", align=True),
          _c("rs_n3", "resize_nhwc", "nonsquare_ratio", ALL, N=2, Hin=5, Win=9, C=8, Hout=7, Wout=4, mode="nearest", align=False),
          _c("rn_n1", "resize_nchw", "nonsquare_ratio", F32, N=2, C=3, Hin=7, Win=10, Hout=4, Wout=23, mode="bilinear", align=False),
          _c("rn_n2", "resize_nchw", "nonsquare_ratio", F32, N=1, C=2, Hin=9, Win=4, Hout=13, Wout=3, mode="bilinear", align=True),
          _c("rn_n3", "resize_nchw", "nonsquare_ratio", F32, N=1, C=2, Hin=5, Win=9, Hout=7, Wout=4, mode="nearest", align=False),
          _c("rn_n4", "resize_nchw", "nonsquare_ratio", F32, N=1, C=2, Hin=9, Win=3, Hout=4, Wout=24, mode="bilinear", align=False),
          _c("fi_n1", "frame_ingest", "nonsquare_ratio", ALL, N=2, H=9, W=16, h=5, w=30), _c("fi_n2", "frame_ingest", "nonsquare_ratio", ALL, N=1, H=7, W=10, h=11, w=4),
          _c("fu_n1", "frame_u8_to_nhwc4", "nonsquare_ratio", F32, N=2, H=9, W=16, h=5, w=30),
          _c("fu_n2", "frame_u8_to_nhwc4", "nonsquare_ratio", F32, N=1, H=7, W=10, h=11, w=4)]
    # ------------------------------------------------------------------------------------------------ grid_wrap: just past cap x 256 work items
    # at the narrowest channel count, one case per capped grid (and storage width).  Resize ratios: see WIDE RATIOS below.
    t += [_c("gw_maxpool_f32", "maxpool3x3s2", "grid_wrap", F32, N=1048600, H=1, W=3, C=4), _c("gw_maxpool_16", "maxpool3x3s2", "grid_wrap", D16, N=1048600, H=1, W=3, C=8),
          _c("gw_prior_f32", "psp_prior_sum", "grid_wrap", F32, N=1, H=1024, W=2049, C=4, sizes=(1, 2)),
          _c("gw_prior_16", "psp_prior_sum", "grid_wrap", D16, N=1, H=1024, W=2049, C=8, sizes=(1, 2)),
          _c("gw_resize_f32", "resize_nhwc", "grid_wrap", F32, N=1, Hin=50, Win=1025, C=4, Hout=1024, Wout=2050, mode="bilinear", align=False),
          _c("gw_resize_16", "resize_nhwc", "grid_wrap", D16, N=1, Hin=50, Win=1025, C=8, Hout=1024, Wout=2050, mode="bilinear", align=False),
          _c("gw_nchw_scalar", "resize_nchw", "grid_wrap", F32, N=1, C=1, Hin=40, Win=50, Hout=2049, Wout=2049, mode="bilinear", align=True),
          _c("gw_nchw_x4", "resize_nchw", "grid_wrap", F32, N=1, C=1, Hin=40, Win=1025, Hout=4096, Wout=4100, mode="bilinear", align=False),
          _c("gw_sa_f32", "scale_add", "grid_wrap", F32, N=1, H=1024, W=2049, C=4, full=True, vec=False),
          _c("gw_sa_16", "scale_add", "grid_wrap", D16, N=1, H=1024, W=2049, C=8, full=True, vec=False),
          _c("gw_head_g_f32", "head", "grid_wrap", F32, N=1, H=724, W=725, C=4, n_cls=2, lsm=True),
          _c("gw_head_g_16", "head", "grid_wrap", D16, N=1, H=724, W=725, C=8, n_cls=2, lsm=True),
          _c("gw_head_m_f32", "head", "grid_wrap", F32, N=1, H=512, W=513, C=8, n_cls=2, lsm=False),
          _c("gw_head_m_16", "head", "grid_wrap", D16, N=1, H=512, W=513, C=64, n_cls=2, lsm=False),
          _c("gw_fi", "frame_ingest", "grid_wrap", ALL, N=1, H=37, W=53, h=1025, w=2049),
          _c("gw_fu", "frame_u8_to_nhwc4", "grid_wrap", F32, N=1, H=37, W=53, h=1025, w=2049),
          _c("gw_cast16", "cast", "grid_wrap", D16, count=16781312, to="16"), _c("gw_cast32", "cast", "grid_wrap", D16, count=16781312, to="32")]
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# Every threshold of the issue's list: (dtype name, case below, its route, case above, its route)
THRESHOLDS = [
    ("f32", "gr_w255_mean", "mean:pl256", "gr_w256_mean", "mean:pl64"), ("f32", "gr_w255_max", "max:pl256", "gr_w256_max", "max:pl64"),
    ("f32", "gr_hw2047_mean", "mean:pl256", "gr_hw2048_mean", "mean:parts"), ("f32", "gr_hw2047_max", "max:pl256", "gr_hw2048_max", "max:parts"),
    ("f32", "gr_b63_mean", "mean:parts", "gr_b64_mean", "mean:pl256"), ("f32", "gr_b63_max", "max:parts", "gr_b64_max", "max:pl256"),
    ("fp16", "gr_c512_mean", "mean16:s1", "gr_c264_mean", "mean16:sN"), ("bf16", "gr_c512_max", "max16:s1", "gr_c264_max", "max16:sN"),
    ("f32", "ap_g255", "pool:pl256", "ap_g256", "pool:pl64"),
    ("f32", "pm_op", "psp:onepass", "pm_fb64", "blockrow:c64t1024"), ("f32", "pm_op6", "psp:onepass", "pm_s7c64", "blockrow:c64t1024"),
    ("f32", "pm_fb64", "blockrow:c16t1024", "pm_fb68", "blockrow:c16t256"), ("f32", "pm_s7c64", "blockrow:c64t1024", "pm_fb512", "blockrow:c64t256"),
    ("f32", "pr_px", "prior:px", "pr_rw", "prior:rowwalk"), ("f32", "pr_px", "prior:px", "pr_w1", "prior:rowwalk"), ("f32", "pr_px", "prior:px", "pr_small", "prior:rowwalk"),
    ("f32", "hd_c64n12", "head:mfma8", "hd_c72n13", "head:mfma16"), ("f32", "hd_c128n19", "head:mfma16", "hd_c136n20", "head:g32"),
    ("f32", "hd_c8n1", "head:mfma8", "hd_c12n32", "head:g32"), ("f32", "hd_c12n12", "head:g12", "hd_c12n13", "head:g19"),
    ("f32", "hd_c136n19", "head:g19", "hd_c20n20", "head:g32"), ("f32", "hd_c512n19", "head:g19", "hd_c64n32", "head:mfma8"),
    ("fp16", "h16_c512n32", "head16:mfma", "h16_c576n20", "head16:g32"), ("bf16", "h16_c64n19", "head16:mfma", "h16_c24n5", "head16:g12"),
    ("bf16", "h16_c128n12", "head16:mfma", "h16_c24n13", "head16:g19"),
    ("f32", "rs_x2", "resize:up2", "rs_x2p", "resize:generic"), ("f32", "rs_x2", "resize:up2", "rs_x2m", "resize:generic"), ("f32", "rs_x2", "resize:up2", "rs_x2a", "resize:generic"),
    ("f32", "rn_r8", "nchw:runs8", "rn_r8a", "nchw:x4"), ("f32", "rn_r16", "nchw:runs16", "rn_r16a", "nchw:x4"), ("f32", "rn_4k", "nchw:x4", "rn_4k1", "nchw:scalar"),
    ("f32", "rn_4ka", "nchw:x4", "rn_4k1a", "nchw:scalar"),
] + [(d, a, ra, b, rb) for d in ALL for a, ra, b, rb in (
    ("fi_w4n", "ingest:px", "fi_w4", "ingest:rows1"), ("fi_same", "ingest:same", "fi_w4", "ingest:rows1"), ("fi_span_o", "ingest:px", "fi_span_u", "ingest:rows2"),
    ("fi_w255", "ingest:rows1", "fi_w257", "ingest:rows2"), ("fi_w256", "ingest:rows1", "fi_w513", "ingest:rows3"), ("fi_up_px", "ingest:px", "fi_up", "ingest:rows1"),
    ("fi_up_px", "ingest:px", "fi_up2seg", "ingest:rows2"))]


def of_class(cls, op=None):
    return [c for c in CASES if c.cls == cls and op in (None, c.op)]


def vec(dname):
    """channels per 16-byte lane vector: the granule of a view either storage takes"""
    return 4 if dname == "f32" else 8


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rnd(c, item, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64([ord(ch) for ch in c.id] + [item]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def make_inputs(case_id):
    """The seeded float32 CPU operands of a case (uint8 for frame_u8_to_nhwc4), by name."""
    c, p = BY_ID[case_id], BY_ID[case_id].p
    if c.op in ("maxpool3x3s2", "adaptive_avgpool", "psp_pool_matrix"):
        return {"x": _rnd(c, 0, p["N"], p["H"], p["W"], p["C"])}
    if c.op == "global_reduce":
        x = _rnd(c, 0, p["N"], p["H"], p["W"], p["C"])
        x[:, :, :, 0] = -x[:, :, :, 0].abs() - 1.0          # an all-negative channel: a max that starts from 0 shows
        x[:, -1, -1, 1] = 50.0                              # the maximum of channel 1 is the last pixel: a dropped tail shows in the max too
        return {"x": x}
    if c.op == "psp_prior_sum":
        return {"t": _rnd(c, 0, p["N"], sum(s * s for s in p["sizes"]), p["C"])}
    if c.op == "resize_nhwc":
        return {"x": _rnd(c, 0, p["N"], p["Hin"], p["Win"], p["C"])}
    if c.op == "resize_nchw":
        return {"x": _rnd(c, 0, p["N"], p["C"], p["Hin"], p["Win"])}
    if c.op == "scale_add":
        return {"x": _rnd(c, 0, p["N"], p["H"], p["W"], p["C"]), "scale": _rnd(c, 1, p["N"], 1, 1, p["C"]),
                "full": _rnd(c, 2, p["N"], p["H"], p["W"], p["C"]) if p["full"] else None, "vec": _rnd(c, 3, p["N"], 1, 1, p["C"]) if p["vec"] else None}
    if c.op == "head":
        return {"x": _rnd(c, 0, p["N"], p["H"], p["W"], p["C"]), "wf": _rnd(c, 1, p["n_cls"], p["C"], scale=1.6 / p["C"] ** 0.5), "bf": _rnd(c, 2, p["n_cls"], scale=0.1)}
    if c.op == "frame_ingest":
        return {"img": _rnd(c, 0, p["N"], 3, p["H"], p["W"])}
    if c.op == "frame_u8_to_nhwc4":
        g = np.random.Generator(np.random.PCG64([ord(ch) for ch in c.id]))
        return {"img": torch.from_numpy(g.integers(0, 256, (p["N"], p["H"], p["W"], 3), dtype=np.uint8))}
    if c.op == "to_nhwc":
        return {"x": _rnd(c, 0, p["N"], p["C"], p["H"], p["W"])}
    if c.op == "to_nchw_contiguous":
        return {"x": _rnd(c, 0, p["N"], p["H"], p["W"], p["C"])}
    assert c.op == "cast", c.op
    return {"x": _rnd(c, 0, p["count"], scale=3.0)}


@functools.lru_cache(maxsize=None)
def _inputs_cached(case_id):
    return make_inputs(case_id)


def inputs(case_id):
    """shared, never written; a grid_wrap case is built per call (its tensors are tens of megabytes)"""
    return make_inputs(case_id) if BY_ID[case_id].cls == "grid_wrap" else _inputs_cached(case_id)


ROUNDED = ("x", "t", "scale", "full", "vec")          # what lives in the storage type; head weights and bias, and the frames, stay fp32


def operands(case_id, dtype=None, ins=None):
    """The operands as the kernels see them, float64: dtype None = fp32 storage; a 16-bit dtype = the stored tensors rounded to it."""
    c = BY_ID[case_id]
    ins = inputs(case_id) if ins is None else ins
    out = {}
    for k, v in ins.items():
        if v is None:
            out[k] = None
        elif dtype is not None and (k in ROUNDED or c.op == "cast"):
            out[k] = v.to(dtype).double()
        else:
            out[k] = v.double()
    return out


# ---------------------------------------------------------------------------------------------------------------- explicit taps and bins
def _axis(n_in, n_out, align, no_clamp=False):
    """include/arseg_hip.h: src = align ? dst (in - 1) / (out - 1) : max((dst + 0.5) in / out - 0.5, 0); i0 = min(floor(src), in - 1),
    i1 = min(i0 + 1, in - 1), l = src - i0 -> (i0, i1, l) float64.  no_clamp: the defect -- a negative src keeps i0 = 0 and its negative l."""
    dst = torch.arange(n_out, dtype=torch.float64)
    if align:
        src = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        src = (dst + 0.5) * (n_in / n_out) - 0.5
        if not no_clamp:
            src = src.clamp(min=0.0)
    i0 = src.clamp(min=0.0).floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0


def _bilerp(x, Hout, Wout, align, no_clamp=False, xmap=None):
    """x NCHW float64 -> NCHW [.., Hout, Wout], the four-tap blend.  xmap: the defect seg_offset's column map (x0, x1 are passed through it)."""
    y0, y1, ly = _axis(x.shape[2], Hout, align, no_clamp)
    x0, x1, lx = _axis(x.shape[3], Wout, align, no_clamp)
    if xmap is not None:
        x0, x1 = xmap(x0), xmap(x1)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def _nearest(x, Hout, Wout):
    """include/arseg_hip.h: i = min(floor(dst * in / out), in - 1), the ratio in float32 as the kernels (and ATen) form it"""
    H, W = x.shape[2], x.shape[3]
    iy = (np.arange(Hout, dtype=np.float32) * (np.float32(H) / np.float32(Hout))).astype(np.int64).clip(max=H - 1)
    ix = (np.arange(Wout, dtype=np.float32) * (np.float32(W) / np.float32(Wout))).astype(np.int64).clip(max=W - 1)
    return x[:, :, torch.from_numpy(iy)][:, :, :, torch.from_numpy(ix)]


def _pool(x, oh, ow, floor_end=False):
    """x NHWC float64 -> [N, oh, ow, C]: the mean over rows floor(b H / oh) .. ceil((b + 1) H / oh) (floor_bin: .. floor) and the same columns.
    An empty bin divides by zero."""
    N, H, W, C = x.shape
    end = (lambda b, n, s: (b + 1) * n // s) if floor_end else (lambda b, n, s: -(-(b + 1) * n // s))
    out = torch.empty(N, oh, ow, C, dtype=torch.float64)
    for by in range(oh):
        for bx in range(ow):
            y0, y1, x0, x1 = by * H // oh, end(by, H, oh), bx * W // ow, end(bx, W, ow)
            out[:, by, bx] = x[:, y0:y1, x0:x1].sum(dim=(1, 2)) / float((y1 - y0) * (x1 - x0))
    return out


def _pool_matrix(x, sizes, pool, prefill=0.0):
    N, H, W, C = x.shape
    out = torch.full((N, sum(s * s for s in sizes), len(sizes) * C), prefill, dtype=torch.float64)
    off = 0
    for i, s in enumerate(sizes):
        out[:, off:off + s * s, i * C:(i + 1) * C] = pool(x, s).reshape(N, s * s, C)
        off += s * s
    return out


def _prior_sum(t, sizes, H, W, up):
    N, _, C = t.shape
    out, off = torch.zeros(N, C, H, W, dtype=torch.float64), 0
    for s in sizes:
        out += up(t[:, off:off + s * s].reshape(N, s, s, C).permute(0, 3, 1, 2))
        off += s * s
    return out.permute(0, 2, 3, 1).contiguous()


def misread_as_dense(x, lead=4, trail=4):
    """The defect ld_as_c on an NHWC operand: the view [1 : N + 1, :, :, lead : lead + C] of the guarded buffer [N + 2, H, W, lead + C + trail]
    (NaN outside the view, as the GPU test builds it) read with a pixel stride of C instead of lead + C + trail."""
    N, H, W, C = x.shape
    wide = torch.full((N + 2, H, W, lead + C + trail), float("nan"), dtype=torch.float64)
    wide[1:N + 1, :, :, lead:lead + C] = x
    flat = wide.reshape(-1)[H * W * (lead + C + trail) + lead:]
    return flat[:N * H * W * C].reshape(N, H, W, C).clone()


def head_bound(c, dtype=None, ins=None):
    """The derived bound of the heads, elementwise [N, n_cls, H, W]: C 2^-23 (sum_c |w| |x| + |b|) per logit -- the standard bound of an fp32 dot
    product of C terms, with a factor 2 for the unknown summation order -- plus, under LogSoftmax, the same for the row's largest logit;
    never below the 1e-4 of the older tests."""
    o = operands(c.id, dtype, ins)
    xc = o["x"].permute(0, 3, 1, 2)
    mag = F.conv2d(xc.abs(), o["wf"].abs()[:, :, None, None], o["bf"].abs()) * (c.p["C"] * 2.0 ** -23)
    if c.p["lsm"]:
        top = F.conv2d(xc, o["wf"][:, :, None, None], o["bf"]).argmax(dim=1, keepdim=True)
        mag = mag + mag.gather(1, top)
    return mag.clamp(min=1e-4)


# ---------------------------------------------------------------------------------------------------------------- reference
def _ingest_xmap(c, dname):
    """seg_offset: a pixel of segment s >= 1 of a staged row takes its taps at its own offsets into segment 0's staging window (which starts at
    column 0): column x of the source becomes x - xs4(s), xs4 the 4-aligned first staged column of its own segment."""
    p = c.p
    if not route(c, dname)[0].startswith("ingest:rows") or p["w"] <= 256:
        return None
    x0 = _axis(p["W"], p["w"], True)[0]
    xs4 = (x0[(torch.arange(p["w"]) // 256) * 256] // 4) * 4          # per output pixel: its segment's first staged column

    def xmap(x):
        return x - xs4
    return xmap


def reference(case_id, dtype=None, defect=None, ins=None):
    """The operation in float64 on the CPU.  defect None: torch's own operators.  Otherwise from the explicit taps and bins above -- "none": the
    operation itself, a second statement of it; a name of DEFECTS: that indexing bug, where it applies to the case (elsewhere: the operation).

    seg_offset         the second and later 256-pixel segments of a staged frame row blend from the first segment's staging window;
    image_straddle     a 32-pixel head tile takes its image from its first pixel: the pixels of a tile that lie in the next image are written
                       behind the first image's plane, the elements they should have reached keep the NaN they start with;
    ld_as_c            the row pitch of an input view is taken as C (the guarded buffer of the GPU test, NaN around the view);
    floor_bin          an adaptive bin ends at floor((b + 1) H / s), not at the ceiling;
    no_clamp           a negative half-pixel source coordinate is not clamped to 0 (and neither is its weight);
    band_tail          the two-stage reduce cuts H W pixels into bands of floor(H W / parts) and drops the remainder;
    sibling_unwritten  the zero blocks of the pool matrix are left as found (NaN)."""
    c, p = BY_ID[case_id], BY_ID[case_id].p
    dname = {None: "f32", torch.float16: "fp16", torch.bfloat16: "bf16"}[dtype]
    o = operands(case_id, dtype, ins)
    plain = defect is None
    x = o.get("x")
    if defect == "ld_as_c" and c.cls == "views":
        x = misread_as_dense(x)
    nc = defect == "no_clamp"
    if c.op == "maxpool3x3s2":
        return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    if c.op == "adaptive_avgpool":
        if plain:
            return F.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), (p["oh"], p["ow"])).permute(0, 2, 3, 1).contiguous()
        return _pool(x, p["oh"], p["ow"], defect == "floor_bin")
    if c.op == "psp_pool_matrix":
        if plain:
            return _pool_matrix(x, p["sizes"], lambda v, s: F.adaptive_avg_pool2d(v.permute(0, 3, 1, 2), s).permute(0, 2, 3, 1))
        return _pool_matrix(x, p["sizes"], lambda v, s: _pool(v, s, s, defect == "floor_bin"), float("nan") if defect == "sibling_unwritten" else 0.0)
    if c.op == "psp_prior_sum":
        H, W = p["H"], p["W"]
        up = (lambda m: F.interpolate(m, (H, W), mode="bilinear", align_corners=False)) if plain else (lambda m: _bilerp(m, H, W, False, nc))
        return _prior_sum(o["t"], p["sizes"], H, W, up)
    if c.op == "global_reduce":
        flat = x.reshape(p["N"], p["H"] * p["W"], p["C"])
        parts = reduce_parts(c, dname)
        if defect == "band_tail" and parts > 1:
            flat = flat[:, :(flat.shape[1] // parts) * parts]
        return flat.sum(dim=1) / float(p["H"] * p["W"]) if p["rop"] == "mean" else flat.amax(dim=1)
    if c.op in ("resize_nhwc", "resize_nchw"):
        xc = x.permute(0, 3, 1, 2) if c.op == "resize_nhwc" else x
        if p["mode"] == "nearest":
            y = F.interpolate(xc, (p["Hout"], p["Wout"]), mode="nearest") if plain else _nearest(xc, p["Hout"], p["Wout"])
        elif plain:
            y = F.interpolate(xc, (p["Hout"], p["Wout"]), mode="bilinear", align_corners=p["align"])
        else:
            y = _bilerp(xc, p["Hout"], p["Wout"], p["align"], nc)
        return (y.permute(0, 2, 3, 1) if c.op == "resize_nhwc" else y).contiguous()
    if c.op == "scale_add":
        y = x * o["scale"]
        y = y if o["full"] is None else y + o["full"]
        return y if o["vec"] is None else y + o["vec"]
    if c.op == "head":
        y = F.conv2d(x.permute(0, 3, 1, 2), o["wf"][:, :, None, None], o["bf"])
        y = F.log_softmax(y, dim=1) if p["lsm"] else y
        if defect == "image_straddle":
            N, K, HW = p["N"], p["n_cls"], p["H"] * p["W"]
            pix = torch.arange(N * HW)
            n0 = (pix // 32 * 32) // HW                                  # the image of the tile's first pixel
            idx = (n0.view(-1, 1) * K + torch.arange(K).view(1, -1)) * HW + (pix - n0 * HW).view(-1, 1)          # [pixel, class]
            vals = y.reshape(N, K, HW).permute(0, 2, 1).reshape(N * HW, K)
            out = torch.full((N * K * HW,), float("nan"), dtype=torch.float64)
            ok = idx < out.numel()
            out[idx[ok]] = vals[ok]
            y = out.reshape(y.shape)
        return y.contiguous()
    if c.op in ("frame_ingest", "frame_u8_to_nhwc4"):
        if c.op == "frame_ingest":
            img = o["img"]
        else:
            img = ((o["img"] / 255.0 - torch.tensor(U8_MEAN, dtype=torch.float64)) / torch.tensor(U8_STD, dtype=torch.float64)).permute(0, 3, 1, 2)
        if (p["h"], p["w"]) == (p["H"], p["W"]):
            y = img
        elif plain:
            y = F.interpolate(img, (p["h"], p["w"]), mode="bilinear", align_corners=True)
        else:
            y = _bilerp(img, p["h"], p["w"], True, xmap=_ingest_xmap(c, dname) if defect == "seg_offset" and c.op == "frame_ingest" else None)
        return y.permute(0, 2, 3, 1).contiguous()
    if c.op == "to_nhwc":
        return x.permute(0, 2, 3, 1).contiguous()
    if c.op == "to_nchw_contiguous":
        return x.permute(0, 3, 1, 2).contiguous()
    assert c.op == "cast" and dtype is not None
    return x          # to 16 bits: the fp32 tensor rounded to nearest even (``operands``); to fp32: the rounded tensor, widened exactly


@functools.lru_cache(maxsize=None)
def _want_cached(case_id, dtype):
    return reference(case_id, dtype)


def want(case_id, dtype=None, ins=None):
    """reference(case, dtype): computed once, shared, never written (a grid_wrap case: per call, from the ``ins`` of the caller)"""
    return reference(case_id, dtype, ins=ins) if BY_ID[case_id].cls == "grid_wrap" else _want_cached(case_id, dtype)


def cast_input(case_id, dtype, ins=None):
    """what ops.cast is given: the fp32 tensor (to 16 bits), or it rounded to the 16-bit type (to fp32)"""
    x = (inputs(case_id) if ins is None else ins)["x"]
    return x if BY_ID[case_id].p["to"] == "16" else x.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- bounds
EXTRA16 = {"psp_pool_matrix": 1e-6, "global_reduce": 1e-6, "resize_nhwc": 1e-5, "scale_add": 1e-6, "frame_ingest": 1e-6}          # close16's ``extra``
TOL32 = {"adaptive_avgpool": 1e-5, "psp_pool_matrix": 1e-6, "psp_prior_sum": 1e-5, "global_reduce": 2e-6, "resize_nhwc": 1e-5, "resize_nchw": 1e-5,
         "scale_add": 1e-6, "frame_ingest": 1e-5, "frame_u8_to_nhwc4": 1e-5}


def is_exact(c):
    """a selection or a move of bits: max, maxpool, nearest resize, a frame at its own size in fp32 storage (per dtype: see bound), layouts, casts"""
    return (c.op in ("maxpool3x3s2", "to_nhwc", "to_nchw_contiguous", "cast") or (c.op == "global_reduce" and c.p["rop"] == "max")
            or (c.op in ("resize_nhwc", "resize_nchw") and c.p["mode"] == "nearest"))


def bound(c, dtype, w64, ins=None):
    """The bound on |got - want|: 0.0 = exact, a float = absolute (fp32 storage), a tensor = elementwise.  Inherited from the op's older test:
    1e-5 for resizes, pooling and frames (1e-6 for the pool matrix), 2e-6 for means, 1e-6 for scale_add, close16 with the same ``extra`` in
    16-bit storage (the prior sum: 1e-5 max|want|).  Derived: the heads (head_bound), and the fp32 prior sum, which had no value test -- the
    1e-5 of the resizes it is a sum of (at most four blends of unit-normal maps: 4 x 3 roundings of 6e-8 x |4| is 3e-6)."""
    if c.op == "head":
        return head_bound(c, dtype, ins)
    if is_exact(c) or (c.op == "frame_ingest" and dtype is None and (c.p["h"], c.p["w"]) == (c.p["H"], c.p["W"])):          # (uint8 frames are normalised in fp32)
        return 0.0
    if dtype is None:
        return TOL32[c.op]
    extra = 1e-5 * float(w64.abs().max()) if c.op == "psp_prior_sum" else EXTRA16[c.op]
    return ULP[dtype] * 0.51 * w64.abs() + extra + 1e-6


def within(got64, w64, b, factor=1.0):
    """elementwise: |got - want| <= factor x bound (exact: equal); a NaN on one side only is a miss"""
    if isinstance(b, float) and b == 0.0:
        return (got64 == w64) | (torch.isnan(got64) & torch.isnan(w64))
    return (got64 - w64).abs() <= factor * b


# ---------------------------------------------------------------------------------------------------------------- routes
def _lib():
    from arseg_amd import _lib as lib

    return lib.load()


def reduce_parts(c, dname):
    """The bands (fp32 storage) or pixel slices (16-bit storage) of a global reduce: from the library's device-free workspace queries,
    arseg_global_reduce_workspace_bytes / arseg_global_mean16_workspace_bytes = N x parts x C x 4 bytes (0: the one-launch form)."""
    p = c.p
    q = _lib().arseg_global_reduce_workspace_bytes if dname == "f32" else _lib().arseg_global_mean16_workspace_bytes
    return int(q(p["N"], p["H"], p["W"], p["C"])) // (p["N"] * p["C"] * 4)


def _blockrow_form(N, C, s):
    # mirrors arseg_adaptive_avgpool_blockrow_fwd (csrc/layers.hip)
    if C % 64 == 0 and s * s * (C // 64) * N >= 64:
        return "blockrow:c64t1024" if s * s * (C // 64) * N < 512 else "blockrow:c64t256"
    return "blockrow:c16t1024" if s * s * -(-C // 16) * N < 256 else "blockrow:c16t256"


def ingest_rows(p):
    # mirrors arseg_frame_to_nhwc4_fwd / arseg_frame_to_nhwc8_16_fwd (csrc/layers.hip): float32 arithmetic, FRAME_SPAN = 1056
    sx = np.float32(p["W"] - 1) / np.float32(p["w"] - 1) if p["w"] > 1 else np.float32(0.0)
    return (p["h"], p["w"]) != (p["H"], p["W"]) and p["W"] % 4 == 0 and bool(np.float32(255.0) * sx + np.float32(8.0) <= np.float32(1056.0))


def route(c, dname):
    """The labels of the kernel forms the host code picks (one, but for the block-row fallback: one per level).  Queried: the two-stage and
    slice counts of the global reduces, whether the pool matrix is built in one pass.  Mirrored (may drift: DESIGN.md): everything else."""
    p, f32 = c.p, dname == "f32"
    if c.op == "maxpool3x3s2":
        return ("maxpool",)
    if c.op == "adaptive_avgpool":          # mirrors arseg_adaptive_avgpool_fwd
        return ("pool:pl256" if p["oh"] * p["ow"] * -(-p["C"] // 16) * p["N"] < 256 else "pool:pl64",)
    if c.op == "psp_pool_matrix":           # ops.psp_pool_matrix asks arseg_psp_pool_matrix_workspace_bytes (and n <= 4, C % 4 == 0, N <= 65535)
        n = len(p["sizes"])
        arr = (ctypes.c_int * n)(*p["sizes"])
        if n <= 4 and _lib().arseg_psp_pool_matrix_workspace_bytes(p["N"], p["H"], p["W"], p["C"], n, arr):
            return ("psp:onepass",)
        assert f32, "16-bit storage has no fallback"
        return tuple(dict.fromkeys(_blockrow_form(p["N"], p["C"], s) for s in p["sizes"]))
    if c.op == "psp_prior_sum":             # mirrors psp_prior_sum<DT>
        return ("prior:rowwalk" if f32 and p["N"] * p["H"] * (p["C"] // 4) >= 49152 else "prior:px",)
    if c.op == "global_reduce":
        parts = reduce_parts(c, dname)
        if not f32:
            return (f"{p['rop']}16:{'s1' if parts == 1 else 'sN'}",)
        if parts:
            return (f"{p['rop']}:parts",)
        return (f"{p['rop']}:{'pl256' if p['N'] * -(-p['C'] // 16) < 256 else 'pl64'}",)          # mirrors arseg_global_reduce_fwd
    if c.op == "resize_nhwc":               # mirrors arseg_resize_fwd (NHWC) / arseg_resize16_fwd
        if p["mode"] == "nearest":
            return ("resize:nearest",)
        return ("resize:up2" if f32 and not p["align"] and (p["Hout"], p["Wout"]) == (2 * p["Hin"], 2 * p["Win"]) else "resize:generic",)
    if c.op == "resize_nchw":               # mirrors arseg_resize_fwd (NCHW); torch's allocations are 16-byte aligned
        if p["mode"] == "nearest":
            return ("nchw:nearest",)
        if not p["align"] and p["Wout"] in (8 * p["Win"], 16 * p["Win"]):
            return (f"nchw:runs{p['Wout'] // p['Win']}",)
        return ("nchw:x4" if p["Wout"] % 4 == 0 else "nchw:scalar",)
    if c.op == "scale_add":
        return ("scale_add",)
    if c.op == "head":                      # mirrors arseg_head_fwd / arseg_head16_fwd
        g = "g12" if p["n_cls"] <= 12 else "g19" if p["n_cls"] <= 19 else "g32"
        if f32:
            return ("head:" + (g if p["C"] % 8 or p["C"] > 128 else "mfma8" if p["C"] <= 64 else "mfma16"),)
        return ("head16:" + ("mfma" if p["C"] % 64 == 0 and p["C"] <= 512 else g),)
    if c.op == "frame_ingest":
        if (p["h"], p["w"]) == (p["H"], p["W"]):
            return ("ingest:same",)
        return (f"ingest:rows{-(-p['w'] // 256)}" if ingest_rows(p) else "ingest:px",)
    if c.op == "frame_u8_to_nhwc4":
        return ("u8:same" if (p["h"], p["w"]) == (p["H"], p["W"]) else "u8:px",)
    if c.op in ("to_nhwc", "to_nchw_contiguous"):
        return (c.op,)
    assert c.op == "cast"
    return (f"cast:to{p['to']}",)


ALL_ROUTES = (
    "maxpool", "pool:pl256", "pool:pl64", "psp:onepass", "blockrow:c64t1024", "blockrow:c64t256", "blockrow:c16t1024", "blockrow:c16t256", "prior:rowwalk", "prior:px",
    "mean:pl256", "mean:pl64", "mean:parts", "max:pl256", "max:pl64", "max:parts", "mean16:s1", "mean16:sN", "max16:s1", "max16:sN",
    "resize:nearest", "resize:up2", "resize:generic", "nchw:nearest", "nchw:runs8", "nchw:runs16", "nchw:x4", "nchw:scalar", "scale_add",
    "head:mfma8", "head:mfma16", "head:g12", "head:g19", "head:g32", "head16:mfma", "head16:g12", "head16:g19", "head16:g32",
    "ingest:same", "ingest:px", "ingest:rows1", "ingest:rows2", "ingest:rows3", "u8:same", "u8:px", "to_nhwc", "to_nchw_contiguous", "cast:to16", "cast:to32")


def grid_items(c, dname):
    """(work items, cap x 256) of the case's grid-stride launch -- threads' worth of work against the threads of a capped grid; None where the
    grid is not capped.  Mirrors the arseg_grid_for(...) arguments of the launches in csrc/layers.hip (the heads: 2048 workgroups)."""
    p, v = c.p, vec(dname)
    full = GRID_CAP * 256
    if c.op == "maxpool3x3s2":
        return p["N"] * ((p["H"] - 1) // 2 + 1) * ((p["W"] - 1) // 2 + 1) * (p["C"] // v), full
    if c.op == "psp_prior_sum" and route(c, dname) == ("prior:px",):
        return p["N"] * p["H"] * p["W"] * (p["C"] // v), full
    if c.op == "resize_nhwc" and route(c, dname) != ("resize:up2",):
        return p["N"] * p["Hout"] * p["Wout"] * (p["C"] // v), full
    if c.op == "resize_nchw":
        r, planes = route(c, dname)[0], p["N"] * p["C"]
        if r.startswith("nchw:runs"):
            return planes * p["Hout"] * (p["Win"] + 1), 65536 * 256
        return planes * p["Hout"] * (p["Wout"] // 4 if r == "nchw:x4" else p["Wout"]), 16384 * 256
    if c.op == "scale_add":
        return p["N"] * p["H"] * p["W"] * (p["C"] // v), full
    if c.op == "head":
        pix = p["N"] * p["H"] * p["W"]
        return (pix, 2048 * 4 * 32) if "mfma" in route(c, dname)[0] else (pix, 2048 * 256)          # 4 waves x 32-pixel tiles per workgroup
    if c.op == "frame_ingest" and not route(c, dname)[0].startswith("ingest:rows"):
        return p["N"] * p["h"] * p["w"], full
    if c.op == "frame_u8_to_nhwc4":
        return p["N"] * p["h"] * p["w"], full
    if c.op == "cast":
        return p["count"] // 8, full
    return None


def tensor_bytes(c, dname):
    """the bytes of the largest tensor a case allocates on the device"""
    p, e = c.p, 4 if dname == "f32" else 2
    if c.op == "maxpool3x3s2":
        return p["N"] * p["H"] * p["W"] * p["C"] * e
    if c.op in ("adaptive_avgpool", "psp_pool_matrix", "global_reduce", "scale_add", "to_nhwc", "to_nchw_contiguous"):
        return p["N"] * p["H"] * p["W"] * p["C"] * e
    if c.op == "psp_prior_sum":
        return p["N"] * max(p["H"] * p["W"], sum(s * s for s in p["sizes"])) * p["C"] * e
    if c.op in ("resize_nhwc", "resize_nchw"):
        return p["N"] * p["C"] * max(p["Hin"] * p["Win"], p["Hout"] * p["Wout"]) * e
    if c.op == "head":
        return p["N"] * p["H"] * p["W"] * max(p["C"] * e, p["n_cls"] * 4)
    if c.op in ("frame_ingest", "frame_u8_to_nhwc4"):
        return p["N"] * max(3 * p["H"] * p["W"] * 4, p["h"] * p["w"] * 16)          # NHWC4 fp32 and NHWC8 16-bit: 16 bytes per pixel
    assert c.op == "cast"
    return p["count"] * 4


# (case, storage) pairs per route label, pinned: a change of the table or of a host predicate shows up in tests/test_layer_geometry.py, and
# tests/test_gpu_layer_geometry.py holds what it launched to these numbers
ROUTE_COUNTS = {
    "maxpool": 16, "pool:pl256": 7, "pool:pl64": 2, "psp:onepass": 18, "blockrow:c64t1024": 3, "blockrow:c64t256": 2, "blockrow:c16t1024": 4, "blockrow:c16t256": 2,
    "prior:rowwalk": 4, "prior:px": 26, "mean:pl256": 8, "mean:pl64": 2, "mean:parts": 3, "max:pl256": 9, "max:pl64": 2, "max:parts": 2, "mean16:s1": 12, "mean16:sN": 14,
    "max16:s1": 10, "max16:sN": 14, "resize:nearest": 12, "resize:up2": 5, "resize:generic": 50, "nchw:nearest": 3, "nchw:runs8": 4, "nchw:runs16": 3, "nchw:x4": 7,
    "nchw:scalar": 8, "scale_add": 16, "head:mfma8": 7, "head:mfma16": 6, "head:g12": 6, "head:g19": 5, "head:g32": 5, "head16:mfma": 24, "head16:g12": 10, "head16:g19": 8,
    "head16:g32": 6, "ingest:same": 6, "ingest:px": 21, "ingest:rows1": 18, "ingest:rows2": 9, "ingest:rows3": 6, "u8:same": 2, "u8:px": 5, "to_nhwc": 3,
    "to_nchw_contiguous": 3, "cast:to16": 4, "cast:to32": 4,
}
