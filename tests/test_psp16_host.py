"""CPU-side checks of the PSPNet 16-bit storage path: the CamVid PSPNet pair accepts set_storage(bf16 / fp16), the semseg pair still
refuses it, the new entry points (16-bit pyramid, 16-bit global max) are declared, bound and exported, and the 16-bit conv's fused x2
upsample refuses every plan and shape it does not cover before it launches anything."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

NEW = ("arseg_psp_pool_matrix16_workspace_bytes", "arseg_psp_pool_matrix16_fwd", "arseg_psp_prior_sum16_fwd", "arseg_global_max16_fwd")


def _psp_pair():
    from arseg_amd.model import PSPNet, PSPNetWithFuse

    kw = dict(sizes=(1, 2, 3, 6), n_classes=12, psp_size=512, deep_features_size=256, backend="resnet18")
    return PSPNet(**kw), PSPNetWithFuse(atten_k=7, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pspnet_pair_accepts_16bit_storage(dtype):
    for m in _psp_pair():
        assert m.SUPPORTS_16BIT
        assert m.set_storage(dtype) is m and m.storage_dtype == dtype
        assert m.set_storage(torch.float32).storage_dtype == torch.float32


def test_pspnet_semseg_still_refuses_16bit():
    from arseg_amd import _lib
    from arseg_amd.model import pspnet_semseg

    for cls in (pspnet_semseg.PSPNet, pspnet_semseg.PSPNetWithFuse):
        m = cls(bins=(1, 2, 3, 6), classes=19, feat_dim=512, layers=18)
        with pytest.raises(_lib.ArsegError, match="BiSeNet and CamVid PSPNet"):
            m.set_storage(torch.bfloat16)


def test_new_entry_points_declared_bound_and_exported():
    from arseg_amd import _lib

    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name + "(" in header
        assert name in _lib.PROTOTYPES
        assert hasattr(lib, name)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from arseg_amd import _lib

    lib = _lib.load()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)          # (never dereferenced: validation returns first)
    sizes = (ctypes.c_int * 4)(1, 2, 3, 6)
    bf = _lib.DT_BF16
    assert lib.arseg_psp_pool_matrix16_workspace_bytes(2, 32, 64, 64, 4, sizes) > 0
    assert lib.arseg_psp_pool_matrix16_workspace_bytes(2, 32, 64, 64, 5, sizes) == 0
    assert lib.arseg_psp_pool_matrix16_fwd(null, 64, fake, bf, fake, 1 << 20, 2, 32, 64, 64, 4, sizes, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_psp_pool_matrix16_fwd(fake, 64, fake, _lib.DT_F32, fake, 1 << 20, 2, 32, 64, 64, 4, sizes, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_psp_pool_matrix16_fwd(fake, 64, fake, bf, fake, 1 << 20, 2, 32, 64, 60, 4, sizes, null) == _lib.ARSEG_EINVAL   # C % 8
    assert lib.arseg_psp_pool_matrix16_fwd(fake, 64, fake, bf, fake, 16, 2, 32, 64, 64, 4, sizes, null) == _lib.ARSEG_EWORKSPACE
    assert lib.arseg_psp_prior_sum16_fwd(null, fake, bf, 2, 32, 64, 64, 4, sizes, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_psp_prior_sum16_fwd(fake, fake, bf, 2, 32, 64, 64, 5, sizes, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_psp_prior_sum16_fwd(fake, fake, 7, 2, 32, 64, 64, 4, sizes, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_global_max16_fwd(null, 64, fake, bf, 2, 8, 8, 64, fake, 1 << 20, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_global_max16_fwd(fake, 64, fake, _lib.DT_F32, 2, 8, 8, 64, fake, 1 << 20, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_global_max16_fwd(fake, 64, fake, bf, 2, 8, 8, 64, null, 0, null) == _lib.ARSEG_EWORKSPACE


def _up2_desc(tile_cfg, H=14, W=18, dil=1):
    from arseg_amd import _lib

    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.in_ld, d.Cout, d.out_ld, d.res_ld = 3, H, W, 64, 64, 64, 64, 64
    d.R, d.S, d.stride, d.pad, d.dil = 3, 3, 1, dil, dil
    d.act, d.tile_cfg, d.upsample2x = _lib.ACT_RELU, tile_cfg, 1
    return d


@pytest.mark.parametrize("case", ["plan1", "plan2", "plan3", "plan4", "plan9", "odd_h", "odd_w", "dil2", "split_k"])
def test_conv16_upsample2x_refuses_what_it_does_not_cover(case):
    """upsample2x is honoured by the patch-resident plans only; every other plan / shape is refused before a launch (ARSEG_EUNSUPPORTED),
    never silently ignored (which would read the half-resolution tensor as if it were H x W)."""
    from arseg_amd import _lib

    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    if case.startswith("plan"):
        d = _up2_desc(int(case[4:]))
    elif case == "odd_h":
        d = _up2_desc(7, H=15)
    elif case == "odd_w":
        d = _up2_desc(7, W=17)
    elif case == "dil2":
        d = _up2_desc(7, dil=2)
    else:
        d = _up2_desc(0)
        d.split_k = 2
    st = lib.arseg_conv2d16_fwd(ctypes.byref(d), _lib.DT_BF16, fake, fake, None, None, None, fake, None, 0, None)
    assert st == _lib.ARSEG_EUNSUPPORTED
