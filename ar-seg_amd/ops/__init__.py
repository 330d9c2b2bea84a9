"""Tensor-level wrappers over the C ABI (include/arseg_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation is a call into
libarseg_hip.so.  All functions raise if a tensor is not a float32 (or, on the 16-bit storage path, fp16 / bf16) CUDA(HIP) tensor --
there is no CPU or PyTorch fallback.

Internal activation layout is NHWC: tensors of shape ``[N, H, W, C]`` (C contiguous).  The helpers
``to_nhwc`` / ``to_nchw`` convert at the API boundary (the reference's interface is NCHW).

The package is split by concern:
  _config   the knobs (``config``, ``configure``), one validation for environment and run-time changes
  _profile  per-launch HIP-event timing (``profile``) and the launch funnel every wrapper goes through
  _plans    the per-shape plan cache + its JSON mirror, the plan tuner
  _base     pointer / stream marshalling, argument checks, workspace, the operand-range word
  layers    layout helpers, localAttention pair, ingest, small layers, evaluator tail, mergeMotion, the record chain and block motion estimation
  creff     warp + CReFF
  egress    labels8 / overlay / confidence / temporal-consistency planes and frame statistics out of the head logits, row-run codes, their connected regions, the regions' links to a reference frame and the absorption of small regions
  conv      the conv engine (route selection, split rows, Winograd, tap decomposition, 16-bit path, PSP bottleneck)
"""
from . import _base, _config, _plans, _profile
from ._base import _DT16, _need_gpu, _need_gpu16, _nhwc_ld, _ptr, _range_word, _stream, is16, range_tripped, workspace
from ._config import Config, config, configure, set_conv_math
from ._plans import _conv_plans, _time
from ._profile import profile
from .conv import (SplitRows, _conv1x1_x3, _conv2d16, _conv_up2_taps, _conv_wino, conv2d, conv_up2_c64, gemm_rows16, gemm_x3_enabled, psp_bottleneck_x3,
                   psp_x3_foldable, split_rows)
from .creff import creff, creff_warp, creff_warp_kernel, flow_resize, mv_resize, warp, warp_mvq
from .egress import contours_fill, contours_simplify, contours_simplify_shared, tolerance_q, labels_consistency, labels_consistency_linked, labels_rle, region_links, rle_absorb, rle_contours, rle_decode, rle_regions, segment_confidence, segment_consistency, segment_egress, segment_stabilise
from .layers import (_frame_ingest_planes, adaptive_avgpool, argmax_confusion, argmax_confusion_grouped, as_nchw, band_radii, block_motion, block_motion_anchor, block_motion_pyr, block_motion_split, boundary_iou, boundary_radii, boundary_radius, calibration, cast, contour_f, contour_radii, contour_radius, frame_ingest, frame_ingest8, frame_ingest_yuv, frame_to_nhwc4, frame_u8_to_nhwc4, from_c8, global_reduce, head, ingest_input,
                     is_nhwc_view, label_bands, local_similar, luma_pyramid, local_weighting, maxpool3x3s2, merge_motion, MV_BI_POLICIES, mv_link_reset, mv_records_bi_reset, mv_records_bi_step, mv_records_bi_step_link, mv_records_rasterize, mv_records_reset, mv_records_step,
                     mv_records_step_link, psp_pool_matrix, psp_prior_sum, resize_nchw, resize_nhwc,
                     mv_chain_heal, scale_add, to_c8, to_nchw_contiguous, to_nhwc)

_LEGACY_SWITCHES = {"_AUTOTUNE": "AUTOTUNE", "_math": "math", "_RANGE_MODE": "RANGE_MODE", "_RANGE_GUARD": "RANGE_GUARD", "_WINOGRAD": "WINOGRAD",
                    "_UP2_TAPS": "UP2_TAPS", "_GEMM_X3": "GEMM_X3", "_IGEMM3": "IGEMM3", "_PLAN_FILE": "PLAN_FILE"}


def __getattr__(name):
    """Read-only views of the switches under their former module-level names (tests, bench.py)."""
    if name in _LEGACY_SWITCHES:
        return getattr(_config.sw, _LEGACY_SWITCHES[name])
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
