"""arseg_conv_plan_query against the launches it describes: for every id of both conv engines the query's verdict is the launch's outcome, a
launch given exactly the workspace bytes the query reports succeeds, and one byte fewer is ARSEG_EWORKSPACE.  (What the launches compute is
held by test_gpu_conv_views.py, test_gpu_ops.py, test_gpu_16bit.py, test_gpu_psp16.py and test_gpu_up2_c64.py; the operands here are zeros.)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

#         H,  W,  Cin, Cout, k, stride, pad, dil      (N = 1; every H x W is even, so each shape also runs as the x2 upsample of H/2 x W/2)
SHAPES = {
    "w50": (12, 50, 64, 64, 3, 1, 1, 1), "w24": (12, 24, 64, 64, 3, 1, 1, 1), "w16": (12, 16, 64, 64, 3, 1, 1, 1),      # the three patch-tile widths
    "dil2": (12, 50, 64, 64, 3, 1, 2, 2),
    "stem": (20, 40, 8, 64, 7, 2, 3, 1),
    "1x1": (12, 50, 96, 19, 1, 1, 0, 1),
    "deep": (8, 8, 512, 128, 3, 1, 1, 1),                 # K long enough for automatic split-K
}
ENGINES = {"f32": (0, 24, "math", 0), "f16x3": (0, 24, "math", 1), "fp16": (1, 14, "dtype", 1), "bf16": (1, 14, "dtype", 2)}


def descriptor(shape, tile_cfg, math, up2, split_k):
    from arseg_amd import _lib

    H, W, Cin, Cout, k, stride, pad, dil = SHAPES[shape]
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.in_ld, d.Cout = 1, H, W, Cin, Cin, Cout
    d.out_ld = d.res_ld = (Cout + 7) // 8 * 8
    d.R, d.S, d.stride, d.pad, d.dil = k, k, stride, pad, dil
    d.tile_cfg, d.math, d.upsample2x, d.split_k = tile_cfg, math, up2, split_k
    return d


@pytest.mark.parametrize("name", list(ENGINES))
def test_query_verdict_is_the_launch_outcome(name):
    from arseg_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib, dev = _lib.load(), torch.device("cuda:0")
    engine, n_ids, what, code = ENGINES[name]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_ok = n_ws = 0
    for shape, (H, W, Cin, Cout, k, stride, pad, dil) in SHAPES.items():
        kpad = (k * k * Cin + 63) // 64 * 64
        Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        # zeros of 4 bytes per element: large enough for either storage; `x` has the full-resolution size for the upsampled form too
        x = torch.zeros(H * W * Cin, dtype=torch.float32, device=dev)
        w = torch.zeros(Cout * kpad, dtype=torch.float32, device=dev)
        out = torch.zeros(Ho * Wo * ((Cout + 7) // 8 * 8), dtype=torch.float32, device=dev)

        def launch(d, ws, nbytes):
            p = ctypes.c_void_p(ws.data_ptr()) if ws is not None else None
            if engine == 0:
                return lib.arseg_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), p, nbytes, stream)
            return lib.arseg_conv2d16_fwd(ctypes.byref(d), code, x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), p, nbytes, stream)

        for up2 in (0, 1):
            for cfg in range(n_ids):
                for sk in (0, 2):
                    d = descriptor(shape, cfg, code if what == "math" else _lib.MATH_F32, up2, sk)
                    info = _lib.ConvPlanInfo()
                    verdict = lib.arseg_conv_plan_query(engine, ctypes.byref(d), ctypes.byref(info))
                    at = (shape, up2, cfg, sk)
                    assert verdict in (_lib.ARSEG_OK, _lib.ARSEG_EINVAL, _lib.ARSEG_EUNSUPPORTED), at
                    if verdict != _lib.ARSEG_OK:
                        assert launch(d, None, 0) == verdict, at
                        continue
                    assert (info.Ho, info.Wo) == (Ho, Wo), at
                    nbytes = info.workspace_bytes
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
                    if nbytes:
                        assert launch(d, ws, nbytes - 1) == _lib.ARSEG_EWORKSPACE, at
                        n_ws += 1
                    assert launch(d, ws, nbytes) == _lib.ARSEG_OK, at
                    n_ok += 1
    torch.cuda.synchronize()
    assert n_ok > 100 and n_ws > 10, (n_ok, n_ws)          # (the grid reaches accepted launches and split-K ones on every engine)
