#!/usr/bin/env python3
"""What the 16-bit storage paths cost per keyframe distance, and what the grouped evaluator tail costs.  One process.

1. On synthetic GOP-12 clips (synth.make_clip): the GOP step (keyframe HR forward + 11 non-keyframes through alter_res_batch_pred) of
   PSPNet-18 (CamVid, 12 classes) and BiSeNet-18 (Cityscapes, 19 classes) in bf16 and fp16 storage, with the fp32 GPU step's labels as
   pseudo-label: one [12, n_cls, n_cls] histogram per configuration from ONE grouped launch per step (d = 0 is the keyframe's own
   segmentation), label agreement per distance = trace / sum of that distance's matrix.
2. The evaluator tail at the headline shapes, three forms alternated (repeats x forms, windows of >= 0.5 s as tools/bench_psp16.py):
   the grouped launch, the ungrouped launch (the floor: one histogram) and eleven one-frame launches with a histogram each (what the
   per-distance table costs without the grouped entry point).
One JSON line on stdout, the same written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from arseg_amd import ops, synth
from arseg_amd import evaluation as ev
from arseg_amd.model import BiSeNetV1, BiSeNetV1WithFuse, PSPNet, PSPNetWithFuse

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
GOP = 12


def window_ms(fn, min_s=0.5):
    """ms per call, averaged over a window of at least min_s seconds (HIP events on the launch stream)."""
    fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < 1e3 * min_s:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(4):
            fn()
        e.record()
        e.synchronize()
        total += s.elapsed_time(e)
        n += 4
    return total / n


def nets(kind, dev):
    if kind == "psp18":
        kw = dict(sizes=(1, 2, 3, 6), n_classes=12, psp_size=512, deep_features_size=256, backend="resnet18")
        hr, lr, norm = PSPNet(**kw), PSPNetWithFuse(atten_k=7, **kw), (synth.CAMVID_MEAN, synth.CAMVID_STD)
    else:
        hr, lr, norm = BiSeNetV1(n_classes=19, backend="resnet18"), BiSeNetV1WithFuse(n_classes=19, backend="resnet18"), (synth.CITY_BISE_MEAN, synth.CITY_BISE_STD)
    synth.load_synth_weights(hr, 0)
    synth.load_synth_weights(lr, 1)
    return hr.to(dev).eval(), lr.to(dev).eval(), norm


def agreement(kind, H, W, clips, dev):
    """{dtype: per-distance label agreement with the fp32 step} over `clips` synthetic GOPs."""
    hr, lr, (mean, std) = nets(kind, dev)
    n_cls = 12 if kind == "psp18" else 19
    hist = {v: torch.zeros((GOP, n_cls, n_cls), dtype=torch.int64, device=dev) for v in ("bf16", "fp16")}
    for seed in range(clips):
        clip = synth.make_clip(40 + seed, H, W, gop=GOP, mean=mean, std=std)
        frames, mvs = torch.from_numpy(clip["frames"]).to(dev), torch.from_numpy(clip["mv"]).to(dev)
        pseudo = None
        for v in ("fp32", "bf16", "fp16"):
            hr.set_storage(DT[v])
            lr.set_storage(DT[v])
            out_k, ref = hr.forward_keyframe(frames[0:1])
            if v == "fp32":
                key_pred, _ = ops.argmax_confusion(out_k, None, H, W)
                pred, _ = ev.alter_res_batch_pred(lr, [ref[0]] * (GOP - 1), frames[1:], mvs[1:], 0.5)
                pseudo = torch.cat([key_pred, pred]).long()          # the fp32 step's labels, d = 0 .. 11
            else:
                ops.argmax_confusion_grouped(out_k, pseudo[0:1], [0], GOP, H, W, hist=hist[v], want_pred=False)
                ev.alter_res_batch_pred(lr, [ref[0]] * (GOP - 1), frames[1:], mvs[1:], 0.5, labels=pseudo[1:], hist=hist[v],
                                        groups=list(range(1, GOP)), n_groups=GOP)
    res = {"frame": [H, W], "clips": clips, "pixels_per_distance": int(hist["bf16"][1].sum())}
    for v, h in hist.items():
        h = h.cpu().double()
        per_d = [float(h[d].diag().sum() / h[d].sum()) for d in range(GOP)]
        res[v] = {"agreement_by_distance": per_d, "agreement_d1_to_11": float(h[1:].sum(0).diag().sum() / h[1:].sum())}
    return res


def tail_cost(name, n_cls, h, w, H, W, align, repeats, window, dev):
    N = GOP - 1
    g = torch.Generator(device="cpu").manual_seed(3)
    logits = torch.randn(N, n_cls, h, w, generator=g).to(dev)
    label = torch.randint(0, n_cls, (N, H, W), generator=g).to(dev)
    groups = torch.arange(1, GOP, dtype=torch.int32, device=dev)
    hist_g = torch.zeros((GOP, n_cls, n_cls), dtype=torch.int64, device=dev)
    hist_u = torch.zeros((n_cls, n_cls), dtype=torch.int64, device=dev)
    hist_f = [torch.zeros((n_cls, n_cls), dtype=torch.int64, device=dev) for _ in range(N)]

    def per_frame():
        for i in range(N):
            ops.argmax_confusion(logits[i:i + 1], label[i:i + 1], H, W, hist=hist_f[i], align_corners=align)

    forms = {"grouped_one_launch": lambda: ops.argmax_confusion_grouped(logits, label, groups, GOP, H, W, hist=hist_g, align_corners=align),
             "ungrouped_one_launch": lambda: ops.argmax_confusion(logits, label, H, W, hist=hist_u, align_corners=align),
             "eleven_one_frame_launches": per_frame}
    for fn in forms.values():          # one call each: the three forms count the same pixels
        fn()
    assert torch.equal(hist_g.sum(0), hist_u) and all(torch.equal(hist_g[i + 1], hist_f[i]) for i in range(N))
    ms = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            ms[k].append(window_ms(fn, window))
    return {"shape": name, "logits": [N, n_cls, h, w], "labels": [N, H, W], "repeats": repeats, "window_s": window,
            **{k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--clips", type=int, default=1)
    ap.add_argument("--psp-size", type=int, nargs=2, default=(512, 1024))
    ap.add_argument("--bise-size", type=int, nargs=2, default=(1024, 2048))
    ap.add_argument("--only", choices=["agreement", "cost"], default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval_by_distance.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"gop": GOP}
    with torch.no_grad():
        if a.only != "cost":
            res["label_agreement_with_fp32_step"] = {"psp18": agreement("psp18", *a.psp_size, a.clips, dev),
                                                     "bise18": agreement("bise18", *a.bise_size, a.clips, dev)}
        if a.only != "agreement":
            res["tail_cost"] = [tail_cost("equal size (PSPNet-18 headline tail)", 12, 512, 1024, 512, 1024, True, a.repeats, a.window, dev),
                                tail_cost("fused x8, align_corners=False (BiSeNet-18)", 19, 128, 256, 1024, 2048, False, a.repeats, a.window, dev)]
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
