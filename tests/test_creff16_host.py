"""Host-side checks of the 16-bit form of the fused warp + CReFF kernel (no GPU): the entry point arseg_creff_warp16_fwd_ex validates its
arguments before any launch, the ``creff_warp16`` knob is validated like every other knob, and ops.creff_warp has no CPU or mixed-dtype fallback."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(lib, *, null=False, dtype=None, n_cls=12, N=2, C=64, k=7, p_layout=None, with_head=True, seg_rows=0):
    from arseg_amd import _lib

    one = ctypes.c_void_p(0 if null else 4096)          # non-null, 16-byte aligned, never dereferenced: validation fails first
    refs = (ctypes.c_void_p * max(N, 1))(*([4096] * max(N, 1)))
    refs_arg = ctypes.c_void_p(0) if null else refs
    head = one if with_head else ctypes.c_void_p(0)
    return lib.arseg_creff_warp16_fwd_ex(refs_arg, one, _lib.DT_BF16 if dtype is None else dtype, one, 16, 16, one, one, one, one, one, one, one,
                                         _lib.C8 if p_layout is None else p_layout, head, head, n_cls, head, 1, N, C, 16, 16, 8, 8, k, k,
                                         seg_rows, 0, None)


def test_warp16_entry_point_rejects_bad_arguments_without_a_gpu():
    from arseg_amd import _lib

    lib = _lib.load()
    assert "arseg_creff_warp16_fwd_ex" in _lib.PROTOTYPES
    assert _call(lib, null=True) == _lib.ARSEG_EINVAL
    assert _call(lib, C=256) == _lib.ARSEG_EUNSUPPORTED                     # the rolling kernel is the 64-channel kernel
    assert _call(lib, k=5) == _lib.ARSEG_EUNSUPPORTED                       # 7 x 7 windows only
    assert _call(lib, n_cls=19) == _lib.ARSEG_EUNSUPPORTED                  # 17-32 classes: the tile kernel, which has no 16-bit form
    assert _call(lib, N=33) == _lib.ARSEG_EUNSUPPORTED                      # 32 frame pointers per launch
    for bad in (_lib.DT_F32, 3, -1):
        assert _call(lib, dtype=bad) == _lib.ARSEG_EINVAL                   # fp16 / bf16 only (fp32: arseg_creff_warp_fwd_ex)
    assert _call(lib, dtype=_lib.DT_F16, C=256) == _lib.ARSEG_EUNSUPPORTED
    assert _call(lib, p_layout=7) == _lib.ARSEG_EINVAL
    assert _call(lib, N=0) == _lib.ARSEG_EINVAL
    assert _call(lib, seg_rows=-2) == _lib.ARSEG_EINVAL
    assert _call(lib, n_cls=0) == _lib.ARSEG_EINVAL                         # logits given without classes
    assert lib.arseg_version() == 5                                         # a new entry point, the same ABI version


def test_creff_warp16_knob_is_validated_by_both_ways_in():
    from arseg_amd import _lib, ops
    from arseg_amd.ops._config import Config

    assert Config().creff_warp16 == ""
    before = ops.config.creff_warp16
    try:
        for v in ("direct", "cast", ""):
            ops.configure(creff_warp16=v)
            assert ops.config.creff_warp16 == v
        with pytest.raises(_lib.ArsegError):
            ops.configure(creff_warp16="dirct")
        assert ops.config.creff_warp16 == ""                                 # a refused value changes nothing
    finally:
        ops.configure(creff_warp16=before)
    from arseg_amd.ops import _config

    assert _config.WARP16_DEFAULT in ("direct", "cast")

    def env_run(value):
        env = {k: v for k, v in os.environ.items() if not k.startswith("ARSEG_")}
        env["ARSEG_CREFF_WARP16"] = value
        code = ("import sys; sys.path.insert(0, %r)\nfrom arseg_amd import ops\nfrom arseg_amd.ops._config import Config\n"
                "print('knob=' + repr(ops.config.creff_warp16))" % ROOT)
        return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)

    for v in ("direct", "cast", ""):
        r = env_run(v)
        assert r.returncode == 0 and f"knob={v!r}" in r.stdout, (v, r.stdout, r.stderr[-600:])
    r = env_run("dirct")
    assert r.returncode != 0 and "creff_warp16" in r.stderr, (r.stdout, r.stderr[-600:])


def test_default_config_equals_environment_config_with_nothing_set():
    from arseg_amd.ops._config import Config

    env = {k: v for k, v in os.environ.items() if not k.startswith("ARSEG_")}
    code = ("import sys; sys.path.insert(0, %r)\nfrom arseg_amd.ops._config import Config\nassert Config.from_env() == Config()\nprint('same')" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "same" in r.stdout, r.stderr[-600:]
    assert "creff_warp16" in {f for f in Config.__dataclass_fields__}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_creff_warp_refuses_cpu_and_mixed_dtype_tensors(dtype):
    """No CPU fallback and no silent conversion: 16-bit CPU tensors, and refs / lr of different element types, raise ArsegError."""
    from arseg_amd import _lib, ops

    class Attn:          # never read: the tensors are refused first
        wq = bq = wk = bk = wv = bv = None

    mv = torch.zeros(1, 8, 8, 2, dtype=torch.int16)
    ref, lr = torch.zeros(8, 8, 64, dtype=dtype), torch.zeros(1, 4, 4, 64, dtype=dtype)
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    for knob in ("direct", "cast", ""):
        prev = ops.configure(creff_warp16=knob)
        try:
            for r_, l_ in ((ref, lr), (ref.float(), lr), (ref, lr.float()), (ref.to(other), lr), (ref, lr.to(other))):
                with pytest.raises(_lib.ArsegError):
                    ops.creff_warp([r_], mv, l_, Attn())
        finally:
            ops.configure(**prev)
