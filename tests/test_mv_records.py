"""CPU-side checks of the motion-vector record path: the host converters (ingest.mv_to_records / records_to_dense, synth.make_record_chain)
against the numpy oracle (tests/mv_records_oracle.py), and the argument validation of the arseg_mv_records_* entry points, which happens
before any launch."""
import ctypes

import numpy as np
import pytest

import mv_records_oracle as oracle


@pytest.mark.parametrize("H,W,F_", [(720, 960, 2), (37, 53, 11), (8, 8, 1), (64, 96, 3)])
def test_records_round_trip_dense_fields(H, W, F_):
    """records_to_dense(mv_to_records(d)) == d on make_mv_chain frames; the records are aligned squares inside the frame that do not
    overlap, in raster order; make_record_chain is mv_to_records of each frame."""
    from arseg_amd import ingest, synth

    flows = synth.make_mv_chain(21 + F_, H, W, F_)
    chain = synth.make_record_chain(21 + F_, H, W, F_)
    assert len(chain) == F_
    for f in range(1, F_ + 1):
        rec = ingest.mv_to_records(flows[f])
        assert rec.dtype == np.int16 and rec.ndim == 2 and rec.shape[1] == 8 and np.array_equal(rec, chain[f - 1])
        x, y, w, h = (rec[:, i].astype(np.int64) for i in range(4))
        assert (w == h).all() and np.isin(w, (1, 2, 4, 8, 16, 32, 64)).all() and (x % w == 0).all() and (y % h == 0).all()
        assert (x >= 0).all() and (y >= 0).all() and (x + w <= W).all() and (y + h <= H).all() and not rec[:, 7].any()
        assert int((w * h).sum()) == H * W                                   # no overlap + full cover (with the round trip below)
        order = y * W + x
        assert (np.diff(order) > 0).all()                                    # raster order of the top-left corners
        back = ingest.records_to_dense(rec, H, W)
        assert back.dtype == np.int16 and np.array_equal(back, flows[f])
        assert np.array_equal(oracle.rasterize(rec, H, W), flows[f])


def test_mv_to_records_merges_constant_areas():
    """A field that is constant on big areas decomposes into few, large squares; a single odd pixel splits only its neighbourhood."""
    from arseg_amd import ingest

    d = np.zeros((128, 192, 3), dtype=np.int16)
    d[..., 2] = 1
    rec = ingest.mv_to_records(d)
    assert rec.shape[0] == 2 * 3 and (rec[:, 2] == 64).all()
    d[70, 130] = (5, -5, 0)
    rec = ingest.mv_to_records(d)
    assert rec.shape[0] == 5 + 3 * 6 + 1 and np.array_equal(ingest.records_to_dense(rec, 128, 192), d)        # 5 whole 64-blocks, 3 siblings per level, the pixel


@pytest.mark.parametrize("case", oracle.adversarial_cases(), ids=lambda c: c[0])
def test_records_to_dense_equals_the_oracle(case):
    from arseg_amd import ingest

    _, H, W, rec = case
    assert np.array_equal(ingest.records_to_dense(rec, H, W), oracle.rasterize(rec, H, W))


def test_adversarial_cases_exercise_the_rules():
    """The hand-made list does what its names say (so that a test over it means something)."""
    cases = {name: (H, W, rec) for name, H, W, rec in oracle.adversarial_cases()}
    a, b = (oracle.rasterize(cases[k][2], 24, 40) for k in ("overlap, small last", "overlap, small first"))
    assert not np.array_equal(a, b)                                                           # the index order decides
    H, W, rec = cases["empty list"]
    assert rec.shape == (0, 8) and (oracle.rasterize(rec, H, W) == np.array(oracle.INTRA, np.int16)).all()
    H, W, rec = cases["zero and negative sizes"]
    assert (oracle.rasterize(rec, H, W) == np.array((5, 5, 0), np.int16)).all()
    H, W, rec = cases["reference indices"]
    assert sorted(set(oracle.rasterize(rec, H, W)[..., 2].ravel().tolist())) == [-1, 0, 1, 2, 3, 5, 90]
    assert np.array_equal(oracle.rasterize(cases["padded buffer"][2], 24, 40), a)
    H, W, rec = cases["wholly off-frame"]
    assert int((oracle.rasterize(rec, H, W)[..., 2] != -1).sum()) == 16


def test_pad_records_and_converter_argument_checks():
    from arseg_amd import ingest

    rec = np.array([[1, 2, 3, 4, 5, 6, 0, 0]], dtype=np.int16)
    p = ingest.pad_records(rec, 4)
    assert p.shape == (4, 8) and p.dtype == np.int16 and np.array_equal(p[0], rec[0]) and not p[1:].any()
    assert np.array_equal(ingest.records_to_dense(p, 9, 9), ingest.records_to_dense(rec, 9, 9))
    with pytest.raises(ValueError):
        ingest.pad_records(np.zeros((5, 8), np.int16), 4)
    with pytest.raises(ValueError):
        ingest.mv_to_records(np.zeros((8, 8, 2), np.int16))
    with pytest.raises(ValueError):
        ingest.records_to_dense(np.zeros((3, 8), np.int32), 8, 8)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """ARSEG_EINVAL / ARSEG_EWORKSPACE come back before any launch: null pointers, H or W > 8192, max_ref outside 1..16, f outside
    [1, gop), a short or misaligned workspace."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)        # non-null pointers are never dereferenced
    EINVAL, EWS = _lib.ARSEG_EINVAL, _lib.ARSEG_EWORKSPACE
    H, W = 10, 12
    need = H * W * 4
    assert lib.arseg_mv_records_workspace_bytes(H, W) == need
    assert lib.arseg_mv_records_workspace_bytes(8192, 8192) == 4 * 8192 * 8192
    assert lib.arseg_mv_records_workspace_bytes(8193, 8) == 0 and lib.arseg_mv_records_workspace_bytes(8, 0) == 0
    step = lib.arseg_mv_records_step_fwd
    # (records, n_records, merged, f, gop, workspace, workspace_bytes, H, W, max_ref, stream)
    assert step(null, 4, one, 1, 12, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, null, 1, 12, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, null, need, H, W, 3, null) == EINVAL
    assert step(one, -1, one, 1, 12, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, one, 1 << 40, 8193, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, one, 1 << 40, H, 8193, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, one, need, 0, W, 3, null) == EINVAL
    for max_ref in (0, -1, 17):
        assert step(one, 4, one, 1, 12, one, need, H, W, max_ref, null) == EINVAL
    for f, gop in ((0, 12), (12, 12), (-1, 12), (1, 1), (13, 12)):
        assert step(one, 4, one, f, gop, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, one, need - 1, H, W, 3, null) == EWS
    assert step(one, 4, one, 1, 12, one, 0, H, W, 3, null) == EWS
    assert step(one, 4, one, 1, 12, odd, need, H, W, 3, null) == EINVAL                  # workspace not 16-byte aligned
    assert step(odd, 4, one, 1, 12, one, need, H, W, 3, null) == EINVAL                  # records not 16-byte aligned
    assert step(one, 4, ctypes.c_void_p(18), 1, 12, one, need, H, W, 3, null) == EINVAL  # merged not 4-byte aligned
    reset = lib.arseg_mv_records_reset                                                    # (merged, workspace, workspace_bytes, H, W, stream)
    assert reset(null, one, need, H, W, null) == EINVAL
    assert reset(one, null, need, H, W, null) == EINVAL
    assert reset(one, one, need, 8193, W, null) == EINVAL
    assert reset(one, one, need - 4, H, W, null) == EWS
    rast = lib.arseg_mv_records_rasterize_fwd                                             # (records, n_records, dense_out, workspace, workspace_bytes, H, W, stream)
    assert rast(null, 4, one, one, need, H, W, null) == EINVAL
    assert rast(one, 4, null, one, need, H, W, null) == EINVAL
    assert rast(one, 4, one, null, need, H, W, null) == EINVAL
    assert rast(one, 4, one, one, need, H, 8193, null) == EINVAL
    assert rast(one, 4, one, one, need - 1, H, W, null) == EWS
    assert lib.arseg_version() == 5


def test_host_layer_has_no_cpu_fallback():
    import torch

    from arseg_amd import _lib, ingest, ops

    rec = torch.zeros((4, 8), dtype=torch.int16)
    merged, idx = torch.zeros((3, 8, 8, 2), dtype=torch.int16), torch.zeros(64, dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):
        ops.mv_records_step(rec, merged, 1, idx)
    with pytest.raises(_lib.ArsegError):
        ops.mv_records_rasterize(rec, 8, 8)
    with pytest.raises(_lib.ArsegError):
        ops.mv_records_reset(merged, idx)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8, 8, device="cpu")
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8193, 8, device="cuda")
