"""Every conv plan and route on the edge geometries of tests/conv_geometry.py (tests/test_conv_geometry.py shows on the CPU that the table
catches the indexing defects it is there for and that this sweep cannot pass vacuously).  Per hazard class and engine -- the fp32 engine
under both maths, the 16-bit engine on fp16 and bf16 -- every case of the class runs on every pinned plan (each id of the library's plan
table, the split-K pairs), on every route above the engines it is eligible for, and once on the automatic plan.  For every (case, plan):

  verdict        the launch raises ArsegError exactly when arseg_conv_plan_query refuses the descriptor ops.conv2d launches (a route: never
                 within its host condition); a refused launch leaves the output untouched;
  values         an accepted launch meets the float64 reference within the bound of its path's older tests: 2e-4 absolute (fp32-engine tiles,
                 patch plans, Winograd), 5e-5 (the tap route), close16 with extra = 2e-5 max|want| (16-bit engine);
  guards         input and residual are the images [1 : N + 1] of a buffer of N + 2 images whose first and last are NaN, and a channel slice of
                 it with NaN neighbours: a read outside the batch or the slice poisons the result.  The output is such a view too: its own
                 elements start as NaN (an unwritten one fails the value check), everything around them holds the sentinel, which must
                 survive; the input and residual buffers must come back bit-identical;
  repeatability  two runs of a pinned plan are torch.equal.

The closing test holds the module's record of what ran to the floor: every plan in every class it applies to, every route in every class it is
eligible in.  ``pytest -s`` prints per test how many (case, plan) pairs were accepted and refused, and the largest error over its bound."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import conv_geometry as cg
from helpers import SENTINEL, bits, boxed, neighbours_intact, pinned

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAIRS = [(cls, name) for cls in cg.CLASSES for name in cg.ENGINES]
_BROKEN = []          # why no further sweep may launch: an exception other than a refusal (a HIP error) ended an earlier one


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def guarded(t_, lead, trail, outer, own=None):
    """(wide, view): ``wide`` [N + 2, H, W, lead + C + trail] filled with ``outer``; ``view`` = wide[1 : N + 1, :, :, lead : lead + C], a legal NHWC
    view, set to ``t_`` (own None) or filled with ``own``."""
    n = t_.shape[0]
    image = torch.full_like(t_[:1], outer)
    wide, _ = boxed(torch.cat([image, t_ if own is None else torch.full_like(t_, own), image]), lead, trail, outer)
    return wide, wide[1:n + 1, :, :, lead:lead + t_.shape[3]]


def surroundings_intact(wide, view_shape, lead):
    """everything of ``wide`` outside the view still holds the sentinel: the images before and after the batch, the channels beside the slice"""
    n, c = view_shape[0], view_shape[3]
    return bool((wide[0] == SENTINEL).all()) and bool((wide[n + 1] == SENTINEL).all()) and neighbours_intact(wide[1:n + 1], lead, c)


class Bench:
    """One case on one engine, on the device: the packed layer, the guarded operands, the reference and its bound."""

    def __init__(self, c, name, dev):
        from arseg_amd import _lib, ops
        from arseg_amd.packing import PackedConv

        self.c, self.name, self.dev = c, name, dev
        self.dtype = cg.DTYPE16.get(name)
        ins = cg.inputs(c.id)
        act = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "prelu": _lib.ACT_PRELU}[c.act]
        self.pc = PackedConv(ins["w"], ins["b"], ins["bn"], c.stride, c.pad, c.dil, act, cg.SLOPE if c.act == "prelu" else 0.0, dev)
        st = torch.float32 if self.dtype is None else self.dtype
        g = 4 if self.dtype is None else 8                      # channels per 16 bytes: the granule of a view either engine takes
        x = F.pad(ins["x"], (0, cg.cin_pad(c, name) - c.Cin)).to(st).to(dev)
        self.wx, self.x = guarded(x, g, g, NAN)
        self.wx_dense, self.x_dense = guarded(x, 0, 0, NAN)     # for the one route that wants dense rows (gemm_rows16)
        self.wr = self.res = None
        if c.res:
            # (16-bit rows are padded to 8 channels, as the library's own output rows are)
            self.wr, self.res = guarded(ins["res"].to(st).to(dev), g, g + (-c.Cout % 8 if self.dtype else 0), NAN)
        self.wx0, self.wxd0, self.wr0 = self.wx.clone(), self.wx_dense.clone(), None if self.wr is None else self.wr.clone()
        self.lead, self.trail = g, g + (-c.Cout % 8 if self.dtype else 0)
        self.oshape = (c.N,) + cg.out_hw(c) + (c.Cout,)
        if self.dtype is not None and c.up2:
            # the 16-bit path rounds the upsampled tensor to 16 bits (resize16, or the staging of a fused plan): the reference runs on the
            # device's own materialised upsample, as tests/test_gpu_conv_views.py and test_gpu_16bit.py do
            want = cg.reference(c.id, self.dtype, conv_input=ops.resize_nhwc(self.x.contiguous(), 2 * c.H, 2 * c.W, _lib.BILINEAR, False))
        else:
            want = cg.want(c.id, self.dtype)
        self.want = want.to(dev)
        self.tol16 = None if self.dtype is None else cg.tol16(want, self.dtype).to(dev)
        self.ld = {"in_ld": self.x.shape[3] + 2 * g, "out_ld": c.Cout + self.lead + self.trail,
                   "res_ld": c.Cout + self.lead + self.trail}

    def fresh(self):
        return guarded(torch.empty(self.oshape, dtype=self.x.dtype, device=self.dev), self.lead, self.trail, SENTINEL, NAN)

    def excess(self, got, tol):
        """max over the elements of |got - want| / bound (fp32: ``tol`` absolute; 16-bit: the elementwise bound of close16); inf where an element
        is NaN or misses it by any amount that is no number"""
        d = (got.double() - self.want).abs()
        r = d / (tol if self.tol16 is None else self.tol16)
        return float("inf") if not bool((r == r).all()) else float(r.max())

    def operands_intact(self):
        return (torch.equal(bits(self.wx), bits(self.wx0)) and torch.equal(bits(self.wx_dense), bits(self.wxd0))
                and (self.wr is None or torch.equal(bits(self.wr), bits(self.wr0))))


def launchers(b):
    """[(label, expected verdict, tolerance, fn(out), repeatable)] of one bench: the pinned plans, the eligible routes, the automatic plan."""
    from arseg_amd import _lib, ops

    c, pc, name = b.c, b.pc, b.name
    out = []

    def engine(cfg, sk, tuner=True):
        def fn(o):
            prev = None if tuner else ops.configure(conv_autotune=False)
            try:
                ops.conv2d(b.x, pc, residual=b.res, out=o, tile_cfg=cfg, split_k=sk, up2=c.up2)
            finally:
                if prev is not None:
                    ops.configure(**prev)
        return fn

    for cfg, sk in cg.plans(name):
        label = f"{cfg}" if sk in (0, 1) else f"{cfg}/{sk}"
        out.append((label, cg.verdict(c, name, cfg, sk, **b.ld)[0], cg.TOL, engine(cfg, sk, tuner=(cfg, sk) != (0, 0)), True))
    for label in cg.routes(c, name):
        kind, arg = label.split(":")[0], int(label.split(":")[1]) if ":" in label else None
        if kind == "wino":
            H, W = cg.conv_hw(c)

            def fn(o, g=arg, H=H, W=W):
                T = _lib.load().arseg_wino43_tiles(c.N, H, W, pc.dil)
                with pinned(("wino_gemm", b.dev.index, T, pc.cin_pad, pc.cout, ops._config.sw.math), g):
                    ops._conv_wino(b.x, pc, b.res, o, c.N, H, W, up2=c.up2)
        elif kind == "x3":
            fn = lambda o, cfg=arg: ops._conv1x1_x3(b.x, pc, b.res, o, False, cfg)      # noqa: E731
        elif kind == "taps":
            fn = lambda o: ops._conv_up2_taps(b.x, pc, o)      # noqa: E731
        elif kind == "up2_c64":
            fn = lambda o, w=arg: ops.conv_up2_c64(b.x, pc, out=o, max_wgs=w)      # noqa: E731
        else:
            assert kind == "rows16"
            fn = lambda o, cfg=arg: ops.gemm_rows16(b.x_dense, pc, residual=b.res, out=o, cfg=cfg)      # noqa: E731
        out.append((label, True, cg.route_tol(label), fn, True))
    # the automatic plan: whatever the tuner lands on (it may time routes and plans of every kind; timing runs are not repeatable bit for bit
    # across plans, so the second run -- the cached plan -- is only held to the bound)
    out.append(("auto", True, cg.TOL, lambda o: ops.conv2d(b.x, pc, residual=b.res, out=o, up2=c.up2), False))
    return out


@functools.lru_cache(maxsize=None)
def sweep(cls, name):
    """-> (failures, {label: accepted launches}, refused launches, worst error / bound): computed once per (class, engine)"""
    from arseg_amd import _lib, ops

    assert not _BROKEN, f"nothing more is launched after {_BROKEN[0]}"
    dev = torch.device("cuda:0")
    prev = ops.set_conv_math("f16x3" if name == "f16x3" else "f32")
    fails, ran, n_ref, worst = [], {}, 0, (0.0, "")
    _BROKEN.append(f"the sweep of {cls} / {name} raised")          # (taken back where the sweep comes to its end: a HIP error is no ArsegError)
    try:
        if name == "f16x3":
            assert ops.gemm_x3_enabled()
        for c in cg.of_class(cls):
            b = Bench(c, name, dev)
            for label, expected, tol, fn, repeatable in launchers(b):
                at = f"{c.id} {name} {label}"
                wo, o = b.fresh()
                try:
                    fn(o)
                    accepted = True
                except _lib.ArsegError as err:
                    status = re.search(r"status (-?\d+)", str(err))
                    if status and int(status.group(1)) > 0:          # a HIP error code, not a verdict: nothing more is launched
                        raise
                    accepted = False
                    if expected:
                        fails.append(f"{at}: refused although {'eligible' if ':' in label or label in ('taps', 'auto') else 'the plan query accepts it'}: {err}")
                if accepted and not expected:
                    fails.append(f"{at}: ran although the plan query refuses it")
                if not surroundings_intact(wo, b.oshape, b.lead):
                    fails.append(f"{at}: wrote outside the output view")
                if not b.operands_intact():
                    fails.append(f"{at}: the input or residual buffer changed")
                    b = Bench(c, name, dev)
                if not accepted:
                    n_ref += 1
                    if not bool(torch.isnan(o).all()):
                        fails.append(f"{at}: refused the call but wrote the output")
                    continue
                e = b.excess(o, tol)
                worst = max(worst, (e, at))
                if not e <= 1.0:
                    bad = ~((o.double() - b.want).abs() <= (tol if b.tol16 is None else b.tol16))
                    where = [tuple(int(v) for v in i) for i in bad.nonzero()[:4]]
                    fails.append(f"{at}: error {e:.3g} x the bound; {int(bad.sum())} of {bad.numel()} elements miss it, first at (n, y, x, c) = {where}")
                    continue
                wo2, o2 = b.fresh()
                fn(o2)
                if repeatable and not torch.equal(o, o2):
                    fails.append(f"{at}: two runs differ by {float((o.double() - o2.double()).abs().max()):.3g}")
                elif not repeatable and not b.excess(o2, tol) <= 1.0:
                    fails.append(f"{at}: second run: error {b.excess(o2, tol):.3g} x the bound")
                if not surroundings_intact(wo2, b.oshape, b.lead):
                    fails.append(f"{at}: second run wrote outside the output view")
                ran[label] = ran.get(label, 0) + 1
        torch.cuda.synchronize()
        _BROKEN.pop()
    finally:
        ops.set_conv_math(prev)
    print(f"{cls} {name}: {sum(ran.values())} launches accepted and checked, {n_ref} refused; worst error {worst[0]:.3g} x its bound ({worst[1]})")
    for f in fails[:40]:
        print("  " + f)
    return fails, ran, n_ref, worst


@pytest.mark.parametrize("cls,name", PAIRS)
def test_every_plan_on_every_case_of_the_class(dev, cls, name):
    fails = sweep(cls, name)[0]
    assert not fails, f"{len(fails)} failures, the first: {fails[:10]}"


def test_every_plan_and_route_ran_in_every_class_it_applies_to(dev):
    """Coverage does not erode: on the device, every plan id and split-K pair was accepted (and checked) at least once in every class it
    applies to, every route in every class a case of which is eligible, the automatic plan on every case.  (The sweeps are computed once; run
    alone, this test computes them.)"""
    missing = []
    for cls, name in PAIRS:
        ran = sweep(cls, name)[1]
        need = {(f"{cfg}" if sk in (0, 1) else f"{cfg}/{sk}") for cfg, sk in cg.plans(name) if cg.applies(name, cfg, sk, cls)}
        need |= {label for c in cg.of_class(cls) for label in cg.routes(c, name)}
        missing += [(cls, name, label) for label in sorted(need) if not ran.get(label)]
        if ran.get("auto", 0) != len(cg.of_class(cls)):
            missing.append((cls, name, "auto", ran.get("auto", 0)))
    assert not missing, missing
