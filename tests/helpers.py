"""Shared helpers for tests: synthetic state_dicts from the committed manifest; channel-slice views and pinned plans for the conv tests."""
import contextlib

import numpy as np
import torch

from arseg_amd import synth

SENTINEL = -7.0          # what the neighbours of an output view hold: a store outside the view changes it


def sd_from_manifest(manifest, name, seed, attn_gain=0.12, res_gain=0.3):
    spec = [(k, tuple(s)) for k, s in manifest[name]["keys"]]
    sd = synth.resolve_aliases(synth.synth_state_dict(spec, seed, attn_gain, res_gain))
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def t(a):
    return torch.from_numpy(np.asarray(a))


def maxdiff(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b)).double()
    return float((a - b).abs().max())


def boxed(t_, lead, trail, fill):
    """(wide, view): ``wide`` [N,H,W,lead+C+trail] filled with ``fill``, ``view`` = wide[..., lead:lead+C] set to ``t_``."""
    n, h, w, c = t_.shape
    wide = torch.full((n, h, w, lead + c + trail), fill, dtype=t_.dtype, device=t_.device)
    view = wide[..., lead:lead + c]
    view.copy_(t_)
    return wide, view


def bits(wide):
    return wide.view(torch.int32)


def neighbours_intact(wide, lead, c):
    return bool((wide[..., :lead] == SENTINEL).all()) and bool((wide[..., lead + c:] == SENTINEL).all())


@contextlib.contextmanager
def pinned(key, plan):
    """``plan`` in the plan cache under ``key`` for the block; the entry found there (or its absence) is restored."""
    from arseg_amd import ops

    saved = ops._conv_plans.get(key)
    ops._conv_plans[key] = plan
    try:
        yield
    finally:
        if saved is None:
            ops._conv_plans.pop(key, None)
        else:
            ops._conv_plans[key] = saved
