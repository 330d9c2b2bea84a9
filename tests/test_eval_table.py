"""CPU-side checks of the per-distance evaluation: the result table in the reference's file format (EvalTable, table_filename), the argument
validation of the grouped evaluator tail (no GPU needed: it comes before any launch), the host wrapper's checks, and the all-reduce of
the [gop, n, n] histogram over gloo for every deal of the GOP runner."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "eval_table_camvid-psp18-AR-0.5x.txt")          # a result file of the reference, unchanged (recorded results)


def test_table_round_trip_is_byte_identical(tmp_path):
    from arseg_amd.evaluation import EvalTable

    table = EvalTable.load(FIXTURE)
    assert len(table.miou) == 12 and table.hist is None and table.iou is None
    assert table.as_array().shape == (13,)
    out = tmp_path / "table.txt"
    table.save(str(out))
    assert out.read_bytes() == open(FIXTURE, "rb").read()
    with pytest.raises(ValueError):
        table.pooled()


def test_table_filenames():
    from arseg_amd.evaluation import table_filename

    assert table_filename("camvid", "psp18", "AR", 0.5, 12, "3M") == "camvid-psp18-AR-0.5x-resolution-exp-GOP12-3M-evaluation.txt"
    assert table_filename("cityscapes", "bise18", "HR", 1.0, 12, "5M") == "cityscapes-bise18-1.0x-resolution-exp-GOP12-5M-evaluation.txt"
    assert table_filename("cityscapes", "bise18", "HR", 0.5, 12, "5M") == "cityscapes-bise18-1.0x-resolution-exp-GOP12-5M-evaluation.txt"   # HR runs at 1.0
    assert table_filename("camvid", "bise18", "LR", 0.5, 12, "3M") == "camvid-bise18-0.5x-resolution-exp-GOP12-3M-evaluation.txt"
    with pytest.raises(ValueError):
        table_filename("camvid", "psp18", "XR", 0.5, 12, "3M")


def _ref_miou(h):
    """evaluation.py:136-137 on one confusion matrix, float32."""
    h = h.float()
    ious = h.diag() / (h.sum(dim=0) + h.sum(dim=1) - h.diag())
    return ious, ious.mean().item()


def test_histogram_to_table(tmp_path):
    from arseg_amd.evaluation import EvalTable

    g = torch.Generator().manual_seed(5)
    hist = torch.randint(0, 100000, (12, 12, 12), generator=g, dtype=torch.int64)
    table = EvalTable(hist)
    assert torch.equal(table.hist, hist) and table.iou.shape == (12, 12) and len(table.miou) == 12
    for d in range(12):
        ious, miou = _ref_miou(hist[d])
        assert isinstance(table.miou[d], float) and table.miou[d] == miou
        assert torch.equal(table.iou[d], ious)
    assert table.mean == np.array(table.miou).mean() and table.mean.dtype == np.float64
    assert np.array_equal(table.as_array(), np.array(table.miou + [np.array(table.miou).mean()]))
    assert table.pooled() == _ref_miou(hist.sum(0))[1]
    assert table.pooled(range(1, 12)) == _ref_miou(hist[1:].sum(0))[1]
    # save -> load keeps the 13 numbers
    path = str(tmp_path / "t.txt")
    table.save(path)
    assert np.array_equal(np.loadtxt(path), table.as_array())
    assert EvalTable.load(path).miou == table.miou
    # a class absent from label and prediction in one group: NaN there (the reference's semantics), and only there
    hist[4, 7, :] = 0
    hist[4, :, 7] = 0
    t2 = EvalTable(hist)
    assert np.isnan(t2.miou[4]) and bool(torch.isnan(t2.iou[4, 7])) and int(torch.isnan(t2.iou).sum()) == 1
    assert not any(np.isnan(t2.miou[d]) for d in range(12) if d != 4)
    assert np.isnan(t2.mean) and not np.isnan(t2.pooled())
    with pytest.raises(ValueError):
        EvalTable(torch.zeros(12, 12, dtype=torch.int64))


def test_grouped_entry_point_rejects_bad_arguments_without_a_gpu():
    from arseg_amd import _lib

    lib = _lib.load()
    fn = lib.arseg_argmax_confusion_grouped_fwd
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # `one`: non-null, never dereferenced -- validation fails first
    shape = (12, 8, 8, 8, 8, 255, 1, null)                       # n_cls, h, w, H, W, ignore_label, align_corners, stream
    assert fn(null, one, one, one, one, 2, 12, *shape) == _lib.ARSEG_EINVAL          # logits
    assert fn(one, one, null, one, one, 2, 12, *shape) == _lib.ARSEG_EINVAL          # hist without group
    assert fn(one, one, one, one, one, 2, 0, *shape) == _lib.ARSEG_EINVAL            # n_groups
    assert fn(one, one, one, one, one, 2, -3, *shape) == _lib.ARSEG_EINVAL
    assert fn(one, one, one, one, one, 0, 12, *shape) == _lib.ARSEG_EINVAL           # N
    assert fn(one, one, one, one, one, 2, 12, 33, *shape[1:]) == _lib.ARSEG_EINVAL   # n_cls beyond the LDS histogram
    assert fn(one, one, one, one, one, 2, 12, 0, *shape[1:]) == _lib.ARSEG_EINVAL
    assert fn(one, null, one, null, one, 2, 12, *shape) == _lib.ARSEG_EINVAL         # neither pred nor label + hist
    assert fn(one, one, one, null, null, 2, 12, *shape) == _lib.ARSEG_EINVAL


def test_host_wrapper_checks():
    from arseg_amd import _lib, ops

    logits, label = torch.zeros(3, 12, 4, 4), torch.zeros(3, 4, 4, dtype=torch.int64)
    with pytest.raises(_lib.ArsegError):
        ops.argmax_confusion_grouped(logits, label, [0, 1, 2], 3, 4, 4)                 # CPU tensors: no fallback
    with pytest.raises(_lib.ArsegError):
        ops.argmax_confusion_grouped(logits, label, torch.tensor([0, 1, 2], dtype=torch.int32), 3, 4, 4)
    with pytest.raises(ValueError):
        ops.argmax_confusion_grouped(logits, label, [0, 1, 3], 3, 4, 4)                 # id outside [0, 3)
    with pytest.raises(ValueError):
        ops.argmax_confusion_grouped(logits, label, [0, -1, 2], 3, 4, 4)
    with pytest.raises(ValueError):
        ops.argmax_confusion_grouped(logits, label, [0, 0, 0], 0, 4, 4)


def test_plan_groups():
    from arseg_amd.gop import GopRunner, frame_plan, neighbor_plan, plan_groups

    runner = GopRunner(None, None, n_gops=1)
    assert plan_groups(runner) == plan_groups(runner.plan) == list(range(1, 12))
    for world in (2, 4):
        for plan in (frame_plan(world, 12, world), neighbor_plan(world, 12, world)):
            assert sorted(d for r in plan for d in plan_groups(r)) == sorted(list(range(1, 12)) * world)
    assert plan_groups(neighbor_plan(2, 12, 2)[0]) == list(range(6, 12)) + list(range(1, 6))


# ---------------------------------------------------------------------------------------------- multi-GPU: the histogram is all that is reduced
N_CLS, GOP, HW = 5, 12, 6 * 8


def _frame_data(n_gops):
    """Per frame (gop index, d): integer labels and "predictions" -- torch.bincount stands in for the GPU tail."""
    g = torch.Generator().manual_seed(11)
    return {(i, d): (torch.randint(0, N_CLS, (HW,), generator=g), torch.randint(0, N_CLS, (HW,), generator=g))
            for i in range(n_gops) for d in range(1, GOP)}


def _grouped_hist(data, frames, groups):
    hist = torch.zeros(GOP, N_CLS, N_CLS, dtype=torch.int64)
    for f, d in zip(frames, groups):
        label, pred = data[f]
        hist[d] += torch.bincount(label * N_CLS + pred, minlength=N_CLS * N_CLS).view(N_CLS, N_CLS)
    return hist


def _hist_worker(rank, world, port, q, deal):
    from arseg_amd.gop import GopRunner, plan_groups

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    runner = GopRunner(None, None, n_gops=world, gop=GOP, local=deal == "local", deal="neighbor" if deal == "neighbor" else "round_robin")
    hist = _grouped_hist(_frame_data(world), runner.plan, plan_groups(runner))
    dist.all_reduce(hist, dist.ReduceOp.SUM)
    q.put((rank, hist.numpy().copy(), len(runner.plan)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("deal", ["round_robin", "neighbor", "local"])
def test_grouped_histogram_all_reduce_matches_single_process(world, deal):
    """Every deal shards by frame, so the all-reduced [gop, n, n] histogram is the single-process one, on every rank."""
    from arseg_amd.evaluation import EvalTable

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_hist_worker, args=(r, world, port, q, deal)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    data = _frame_data(world)
    frames = sorted(data)
    single = _grouped_hist(data, frames, [d for _, d in frames])
    assert int(single[0].sum()) == 0 and all(int(single[d].sum()) == world * HW for d in range(1, GOP))
    for _, hist, n_frames in results:
        assert n_frames == GOP - 1
        assert torch.equal(torch.from_numpy(hist), single)
    assert EvalTable(torch.from_numpy(results[0][1])).miou[1:] == EvalTable(single).miou[1:]
