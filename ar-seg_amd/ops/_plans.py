"""Per-shape launch plans (tile shape, LDS buffering, split-K, route): the cache, its optional JSON mirror, and the one tuner (``tuned``)
every conv route picks its plan with.

The library's built-in heuristic is good to ~10 %; the first time a conv shape is seen on a device the candidates are timed with HIP
events and the fastest is cached (what MIOpen calls "find").  ARSEG_CONV_AUTOTUNE=0 keeps the heuristic."""
from __future__ import annotations

import os

import torch

from .. import _lib
from . import _config
from ._config import sw


class _PlanCache(dict):
    """Plans keyed by shape tuples; optionally mirrored to a JSON file (``ops.configure(conv_plan_file=...)`` merges that file in)."""

    def __init__(self):
        super().__init__()
        self.load()

    def load(self):
        if sw.PLAN_FILE and os.path.exists(sw.PLAN_FILE):
            import json

            with open(sw.PLAN_FILE) as f:
                for k, v in json.load(f).items():
                    super().__setitem__(tuple(json.loads(k)), tuple(v) if isinstance(v, list) else v)

    def __setitem__(self, key, value):
        super().__setitem__(key, value)
        if sw.PLAN_FILE:
            import json

            with open(sw.PLAN_FILE, "w") as f:
                json.dump({json.dumps(list(k)): (list(v) if isinstance(v, tuple) else v) for k, v in self.items()}, f, indent=0)


_conv_plans = _PlanCache()
_config._plan_file_listeners.append(_conv_plans.load)


def fuses_up2(tile_cfg: int, engine: int = _lib.CONV_ENGINE_F32) -> bool:
    """Does plan ``tile_cfg`` of the engine apply desc.upsample2x itself (the patch-resident 3x3 plans, up_3's kernel)?  The library's plan table says."""
    return bool(_lib.conv_plan_row(engine, tile_cfg).fuses_upsample)


def _conv_candidates(ktiles: int, cout: int, m: int, patch_ok: bool = False):
    cands = []
    if patch_ok:                                   # patch-resident 3x3 kernel (13/14: 128-pixel tiles, 15/16: 256; BN 64/128)
        cands += [(15, 1), (13, 1), (20, 1), (21, 1), (22, 1)] + ([(16, 1), (14, 1)] if cout > 64 else [])      # 20..22: squarer 64-channel tiles (r6)
        if cout == 64 and ktiles == 18:            # up_3's persistent kernel: 64 -> 64; the library refuses it (skipped) without a fused upsample
            cands.append((23, 1))
    for cfg in (5, 6, 7, 8, 9, 10, 11, 12) + ((17, 18, 19) if sw.math == _lib.MATH_F16X3 else ()):
        row = _lib.conv_plan_row(_lib.CONV_ENGINE_F32, cfg)
        if (row.kind == _lib.PLAN_TILE_WIDE and cout < row.bn) or (row.bn == 128 and cout <= 64) or (row.bm == 128 and m <= 64):
            continue
        for sk in (1, 2, 3, 4, 6, 8):
            if sk > 1 and (ktiles // sk < 4 or cout % 4):
                continue
            cands.append((cfg, sk))
    return cands


def _time(fn, reps=6, rounds=2):
    """ms per call: the faster of ``rounds`` averages over ``reps`` calls (plans chosen from one short average were visibly noisy box to box)."""
    fn()
    best = float("inf")
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e) / reps)
    return best


def _capturing() -> bool:
    """Is a HIP-graph capture running on the current stream?  (Nothing may be timed inside one.)"""
    return torch.cuda.is_current_stream_capturing()


def _fastest(candidates, run, timer, margin=None):
    """The candidate whose ``timer(lambda: run(plan))`` (x ``margin[plan]``, default 1) is lowest; the first of equals wins.  A candidate
    that raises ArsegError is skipped; None if none launched."""
    best, best_t = None, float("inf")
    for plan in candidates:
        try:
            t = timer(lambda: run(plan))
        except _lib.ArsegError:
            continue
        if margin:
            t *= margin.get(plan, 1.0)
        if t < best_t:
            best, best_t = plan, t
    return best


def tuned(key, candidates, run, *, timer=_time, valid=None, untuned=None, margin=None):
    """The plan of ``key``: the cached one if ``valid`` accepts it (a rejected one -- a route switched off, a plan of an older round -- is
    re-tuned); ``untuned``, if given, while the tuner is off or a graph capture runs (not cached); else the fastest of ``candidates``
    launched by ``run(plan)`` (see _fastest), cached.  None if no candidate launched (never cached)."""
    plan = _conv_plans.get(key)
    if plan is not None and (valid is None or valid(plan)):
        return plan
    if untuned is not None and (not sw.AUTOTUNE or _capturing()):
        return untuned
    plan = _fastest(candidates, run, timer, margin)
    if plan is not None:
        _conv_plans[key] = plan
    return plan


def _tune_conv(run, pc, m, allow_patch=True):
    """The fastest (tile_cfg, split_k) of arseg_conv2d_fwd for ``pc`` on an M = ``m`` GEMM, launched by ``run(plan)``; None if none launched.
    allow_patch=False: the GEMM-tile plans only (the input of a fused x2 upsample is materialised for them)."""
    ktiles = (pc.R * pc.S * pc.cin_pad + 31) // 32
    patch_ok = allow_patch and (sw.math == _lib.MATH_F16X3 and pc.R == 3 and pc.S == 3 and pc.stride == 1 and pc.pad == pc.dil == 1 and pc.cin_pad % 32 == 0)
    return _fastest(([(0, 0)] if allow_patch else []) + _conv_candidates(ktiles, pc.cout, m, patch_ok), run,
                    lambda f: _time(f, reps=3, rounds=1))
