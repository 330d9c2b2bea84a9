"""up_3's persistent kernel (csrc/conv_up2_c64.hip, arseg_conv_up2_c64_fwd = tile_cfg 23): 3x3 conv, 64 -> 64 channels, on the x2 bilinear
upsample of its input, against the patch-resident plan it replaces and against the fp64 oracle of PSPUpsample (oracle/cpu_ref.py)."""
import functools

import numpy as np
import pytest
import torch

from helpers import maxdiff

pytestmark = pytest.mark.gpu

# The bound tests/test_gpu_ops.py::test_conv2d_fused_upsample holds the fused-upsample plans to under f16x3, on inputs drawn the same way
# (unit normal activations, He-scaled weights, BatchNorm statistics in [0.5, 1.5]).
BOUND = 2e-4
OLD_CFG = 13           # the patch-resident kernel on its default tile: admits every map size used here
SLOPE = {"none": 1.0, "relu": 0.0, "prelu": 0.3}      # the oracle's PSPUpsample always ends in a PReLU: slope 1 = no activation, 0 = ReLU

# (N, h, w) of the low-resolution input; the conv runs at 2h x 2w
#   16 x 32: one 8 x 16 tile per workgroup -- the first tile of a run is also its last
#   24 x 40: neither a multiple of the tile; partial tiles right and bottom, an image boundary inside a run
#   64 x 48: 72 tiles on a grid capped to 2 workgroups: 36 trips through the persistent loop, both patch buffers many times over
SHAPES = {"one_tile_each": (1, 8, 16, 0), "ragged": (2, 12, 20, 0), "long_runs": (3, 32, 24, 2)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib, ops

    _lib.load()
    prev = ops.set_conv_math("f16x3")
    yield torch.device("cuda:0")
    ops.set_conv_math(prev)


def _rnd(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _layer():
    g = np.random.Generator(np.random.PCG64(281))
    wt = _rnd(282, 64, 64, 3, 3, scale=float(np.sqrt(2.0 / (64 * 9))))
    b = _rnd(283, 64, scale=0.1)
    bn = (torch.from_numpy(g.uniform(0.5, 1.5, 64).astype(np.float32)), _rnd(284, 64, scale=0.1), _rnd(285, 64, scale=0.1),
          torch.from_numpy(g.uniform(0.5, 1.5, 64).astype(np.float32)))          # gamma, beta, mean, var
    return wt, b, bn


@functools.lru_cache(maxsize=None)
def _input(name):
    N, h, w, _ = SHAPES[name]
    return _rnd(280 + N, N, 64, h, w)


@functools.lru_cache(maxsize=None)
def _oracle(name, act):
    """fp64 PSPUpsample of the oracle (upsample -> conv3x3 -> BatchNorm -> PReLU), NCHW."""
    from oracle import cpu_ref

    wt, b, bn = _layer()
    sd = {"up.conv.0.weight": wt, "up.conv.0.bias": b, "up.conv.1.weight": bn[0], "up.conv.1.bias": bn[1], "up.conv.1.running_mean": bn[2],
          "up.conv.1.running_var": bn[3], "up.conv.2.weight": torch.tensor([SLOPE[act]])}
    return cpu_ref.psp_upsample({k: v.double() for k, v in sd.items()}, "up.", _input(name).double())


def _packed(act, dev):
    from arseg_amd import _lib
    from arseg_amd.packing import PackedConv

    wt, b, bn = _layer()
    code = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU}[act]
    return PackedConv(wt, b, bn, 1, 1, 1, code, SLOPE[act] if act == "prelu" else 0.0, dev)


@pytest.mark.parametrize("act", ["none", "relu", "prelu"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_up2_c64_matches_patch_plan_and_oracle(dev, name, act):
    from arseg_amd import ops

    N, h, w, cap = SHAPES[name]
    pc = _packed(act, dev)
    xd = _input(name).permute(0, 2, 3, 1).contiguous().to(dev)
    want = _oracle(name, act)
    old = ops.conv2d(xd, pc, up2=True, tile_cfg=OLD_CFG, split_k=1)
    new = torch.full((N, 2 * h, 2 * w, 64), float("nan"), device=dev)
    ops.conv_up2_c64(xd, pc, out=new, max_wgs=cap)
    e_ref, e_old = maxdiff(new.permute(0, 3, 1, 2), want), maxdiff(new, old)
    print(f"{name} {act}: max-abs against fp64 {e_ref:.3g}, against the patch plan {e_old:.3g}")
    assert e_ref <= BOUND, f"against fp64: {e_ref:.3g}"
    assert e_old <= BOUND, f"against tile_cfg {OLD_CFG}: {e_old:.3g}"
    # the same plan through the conv engine (tile_cfg 23), uncapped grid
    via = ops.conv2d(xd, pc, up2=True, tile_cfg=23, split_k=1)
    assert maxdiff(via, new) == 0.0, "the same kernel on another grid: a tile's arithmetic does not depend on who computes it"
    assert maxdiff(via.permute(0, 3, 1, 2), want) <= BOUND


def test_up2_c64_writes_a_channel_slice(dev):
    """out_ld = 96 > 64: the kernel writes channels 16..79 of a wider tensor and nothing else."""
    from arseg_amd import ops

    name, act = "ragged", "prelu"
    N, h, w, _ = SHAPES[name]
    pc = _packed(act, dev)
    xd = _input(name).permute(0, 2, 3, 1).contiguous().to(dev)
    wide = torch.full((N, 2 * h, 2 * w, 96), -7.0, device=dev)
    ops.conv_up2_c64(xd, pc, out=wide[..., 16:80])
    e_ref = maxdiff(wide[..., 16:80].permute(0, 3, 1, 2), _oracle(name, act))
    assert e_ref <= BOUND, f"against fp64: {e_ref:.3g}"
    assert bool((wide[..., :16] == -7.0).all()) and bool((wide[..., 80:] == -7.0).all())
    # a strided input (a channel slice of a wider tensor) as well
    xw = torch.zeros((N, h, w, 80), device=dev)
    xw[..., 8:72] = xd
    old = ops.conv2d(xw[..., 8:72], pc, up2=True, tile_cfg=OLD_CFG, split_k=1)
    e_old = maxdiff(ops.conv_up2_c64(xw[..., 8:72], pc), old)
    assert e_old <= BOUND, f"against tile_cfg {OLD_CFG}: {e_old:.3g}"


def test_up2_c64_range_watch_agrees_with_patch_plan(dev):
    """Activations beyond the split-fp16 range: both plans raise the range word; inside it neither does."""
    from arseg_amd import ops

    name = "one_tile_each"
    pc = _packed("none", dev)
    xd = _input(name).permute(0, 2, 3, 1).contiguous().to(dev)
    big = xd.clone()
    big[0, 3, 5, 17] = 2.0e5                                 # the conv multiplies the UPSAMPLED values: the nearest one is 0.5625 of this, still past 65504
    verdict = {}
    for label, x in (("in_range", xd), ("beyond", big)):
        for plan in ("old", "new"):
            ops.range_tripped()                              # clear
            if plan == "old":
                ops.conv2d(x, pc, up2=True, tile_cfg=OLD_CFG, split_k=1)
            else:
                ops.conv_up2_c64(x, pc)
            verdict[label, plan] = ops.range_tripped()
    assert verdict["in_range", "old"] is False and verdict["in_range", "new"] is False, verdict
    assert verdict["beyond", "old"] is True and verdict["beyond", "new"] is True, verdict


def test_up2_c64_refuses_other_shapes(dev):
    from arseg_amd import _lib, ops
    from arseg_amd.packing import PackedConv

    wt = _rnd(290, 32, 64, 3, 3, scale=0.05)
    pc = PackedConv(wt, None, None, 1, 1, 1, _lib.ACT_NONE, 0.0, dev)
    x = torch.zeros((1, 8, 16, 64), device=dev)
    with pytest.raises(_lib.ArsegError):
        ops.conv2d(x, pc, up2=True, tile_cfg=23, split_k=1)
