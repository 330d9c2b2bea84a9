"""Every kernel form of csrc/layers.hip on the edge geometries of tests/layer_geometry.py (tests/test_layer_geometry.py shows on the CPU that
the table catches the indexing defects it is there for and that this sweep cannot pass vacuously).  Per hazard class and op, every case of
the class runs in every storage it has.  For every (case, storage):

  values         the result meets the float64 reference within the bound of the op's older test (the heads: the derived bound), exactly where
                 the op selects or moves bits;
  guards         an operand that may be a view is one: the images [1 : N + 1] of a buffer of N + 2 images whose first and last are NaN, and a
                 channel slice of it with NaN neighbours, so that a read outside the batch or the slice poisons the result.  An output view's own
                 elements start as NaN (an unwritten one fails the value check), everything around them holds the sentinel, which must
                 survive; the input buffers must come back bit-identical.  (grid_wrap cases run dense: a guarded 34 MB tensor is 300 MB.)
  poison         where the op allocates its output, a NaN block of the result's size is allocated and freed first, so that an unwritten
                 element is likely to read NaN;
  repeatability  two runs are torch.equal (the reduces are deterministic).

The closing test holds the module's record of what ran to the floor tests/test_layer_geometry.py pins: every route label, as often as the
table reaches it.  ``pytest -s`` prints per test the largest error over its bound."""
import functools
import re

import pytest
import torch

import layer_geometry as lg
from helpers import SENTINEL, bits, boxed, neighbours_intact

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAIRS = [(cls, op) for cls in lg.CLASSES for op in lg.APPLIES[cls]]
VIEW_OPS = lg.APPLIES["views"]
_BROKEN = []          # why no further sweep may launch: an exception other than a refusal (a HIP error) ended an earlier one
RAN = {}              # route label -> (case, storage) pairs launched and checked
WORST = {}            # (op, storage) -> (largest error / bound, where)


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


def surroundings_intact(wide, n, c, lead):
    return bool((wide[0] == SENTINEL).all()) and bool((wide[n + 1] == SENTINEL).all()) and neighbours_intact(wide[1:n + 1], lead, c)


def poison(shape, dtype, dev):
    """the caching allocator hands this block back to the op's own torch.empty of the same size"""
    block = torch.full(tuple(shape), NAN, dtype=dtype, device=dev)
    del block


class Bench:
    """One case in one storage, on the device: its operands (guarded views where the op takes views), and ``run()`` -> (result in the layout
    of lg.want, failures of the guards)."""

    def __init__(self, c, dname, dev, ins):
        self.c, self.dname, self.dev = c, dname, dev
        self.dtype = lg.DTYPES[dname]
        self.st = torch.float32 if self.dtype is None else self.dtype
        self.g = lg.vec(dname)
        self.viewed = c.op in VIEW_OPS and c.cls != "grid_wrap"
        self.d = {}
        for k, v in ins.items():
            if v is None:
                self.d[k] = None
            elif c.op == "cast":
                self.d[k] = lg.cast_input(c.id, self.dtype, ins).to(dev)
            elif k in lg.ROUNDED:
                self.d[k] = v.to(self.st).to(dev)
            else:
                self.d[k] = v.to(dev)
        self.wx = None
        if self.viewed:
            self.wx, self.d["x"] = guarded(self.d["x"], self.g, self.g, NAN)
        self.before = {k: (self.wx if k == "x" and self.viewed else v).clone() for k, v in self.d.items() if v is not None} if c.cls != "grid_wrap" else {}

    def operands_intact(self):
        for k, v0 in self.before.items():
            now = self.wx if k == "x" and self.viewed else self.d[k]
            same = torch.equal(now, v0) if v0.dtype == torch.uint8 else torch.equal(bits(now.reshape(-1)), bits(v0.reshape(-1)))
            if not same:
                return False
        return True

    def run(self):
        from arseg_amd import _lib, ops

        c, p, d, dev, st = self.c, self.c.p, self.d, self.dev, self.st
        fails = []
        if c.op == "maxpool3x3s2":
            poison((p["N"], (p["H"] - 1) // 2 + 1, (p["W"] - 1) // 2 + 1, p["C"]), st, dev)
            return ops.maxpool3x3s2(d["x"]), fails
        if c.op == "adaptive_avgpool":
            N, C, bins = p["N"], p["C"], p["oh"] * p["ow"]
            if not p.get("wide"):
                poison((N, p["oh"], p["ow"], C), st, dev)
                return ops.adaptive_avgpool(d["x"], p["oh"], p["ow"]), fails
            # rows [1 : 1 + bins] and columns [4 : 4 + C] of a matrix [N, bins + 2, C + 8]: a row pitch and an image stride of its own
            mat = torch.full((N, bins + 2, C + 8), SENTINEL, dtype=st, device=dev)
            mat[:, 1:1 + bins, 4:4 + C] = NAN
            ops.adaptive_avgpool(d["x"], p["oh"], p["ow"], out=mat[0, 1, 4:], out_ld=C + 8, out_n_stride=(bins + 2) * (C + 8))
            got = mat[:, 1:1 + bins, 4:4 + C].reshape(N, p["oh"], p["ow"], C).clone()
            mat[:, 1:1 + bins, 4:4 + C] = SENTINEL
            if not bool((mat == SENTINEL).all()):
                fails.append("wrote outside its rows of the wider matrix")
            return got, fails
        if c.op == "psp_pool_matrix":
            poison((p["N"], sum(s * s for s in p["sizes"]), 1, len(p["sizes"]) * p["C"]), st, dev)
            return ops.psp_pool_matrix(d["x"], p["sizes"])[:, :, 0], fails
        if c.op == "psp_prior_sum":
            poison((p["N"], p["H"], p["W"], p["C"]), st, dev)
            return ops.psp_prior_sum(d["t"], p["sizes"], p["H"], p["W"]), fails
        if c.op == "global_reduce":
            poison((p["N"], 1, 1, p["C"]), st, dev)
            return ops.global_reduce(d["x"], _lib.REDUCE_MEAN if p["rop"] == "mean" else _lib.REDUCE_MAX).reshape(p["N"], p["C"]), fails
        if c.op == "resize_nhwc":
            mode = _lib.NEAREST if p["mode"] == "nearest" else _lib.BILINEAR
            if not self.viewed:
                poison((p["N"], p["Hout"], p["Wout"], p["C"]), st, dev)
                return ops.resize_nhwc(d["x"], p["Hout"], p["Wout"], mode, p["align"]), fails
            wo, o = guarded(torch.empty((p["N"], p["Hout"], p["Wout"], p["C"]), dtype=st, device=dev), self.g, self.g, SENTINEL, NAN)
            ops.resize_nhwc(d["x"], p["Hout"], p["Wout"], mode, p["align"], out=o)
            if not surroundings_intact(wo, p["N"], p["C"], self.g):
                fails.append("wrote outside the output view")
            return o, fails
        if c.op == "resize_nchw":
            poison((p["N"], p["C"], p["Hout"], p["Wout"]), st, dev)
            return ops.resize_nchw(d["x"], p["Hout"], p["Wout"], _lib.NEAREST if p["mode"] == "nearest" else _lib.BILINEAR, p["align"]), fails
        if c.op == "scale_add":
            poison((p["N"], p["H"], p["W"], p["C"]), st, dev)
            return ops.scale_add(d["x"], d["scale"], add_full=d["full"], add_vec=d["vec"]), fails
        if c.op == "head":
            poison((p["N"], p["n_cls"], p["H"], p["W"]), torch.float32, dev)
            got = ops.head(d["x"], d["wf"], d["bf"], p["lsm"])
            if got.dtype != torch.float32:
                fails.append(f"logits are {got.dtype}")
            return got, fails
        if c.op in ("frame_ingest", "frame_u8_to_nhwc4"):
            if c.op == "frame_ingest":
                poison((p["N"], p["h"], p["w"], 4 if self.dtype is None else 8), st, dev)
                got = ops.frame_ingest(d["img"], p["h"], p["w"], st)
            else:
                poison((p["N"], p["h"], p["w"], 4), st, dev)
                got = ops.frame_u8_to_nhwc4(d["img"], p["h"], p["w"], lg.U8_MEAN, lg.U8_STD)
            if got.shape[3] != (4 if self.dtype is None else 8) or not bool((got[..., 3:] == 0).all()):
                fails.append("the padding channels are not zero")
            return got[..., :3], fails
        if c.op == "to_nhwc":
            poison((p["N"], p["H"], p["W"], p["C"]), st, dev)
            return ops.to_nhwc(d["x"]), fails
        if c.op == "to_nchw_contiguous":
            poison((p["N"], p["C"], p["H"], p["W"]), st, dev)
            return ops.to_nchw_contiguous(d["x"]), fails
        assert c.op == "cast"
        to = self.dtype if p["to"] == "16" else torch.float32
        poison((p["count"],), to, dev)
        return ops.cast(d["x"], to), fails


def excess(got, w64, b):
    """max over the elements of |got - want| / bound (an exact op: 0 or inf); inf where an element is NaN"""
    g64 = got.double()
    if isinstance(b, float) and b == 0.0:
        return 0.0 if torch.equal(g64, w64) else float("inf")
    r = (g64 - w64).abs() / b
    return float("inf") if not bool((r == r).all()) else float(r.max())


@functools.lru_cache(maxsize=None)
def sweep(cls, op):
    """-> (failures, [(route labels, case, storage)] launched and checked, worst error / bound): computed once per (class, op)"""
    from arseg_amd import _lib

    assert not _BROKEN, f"nothing more is launched after {_BROKEN[0]}"
    dev = torch.device("cuda:0")
    fails, ran, worst = [], [], (0.0, "")
    _BROKEN.append(f"the sweep of {cls} / {op} raised")          # (taken back where the sweep comes to its end: a HIP error is no ArsegError)
    for c in lg.of_class(cls, op):
        ins = lg.inputs(c.id)          # (a grid_wrap case: built here, once, for all its storages)
        for dname in c.dtypes:
            at = f"{c.id} {dname}"
            dtype = lg.DTYPES[dname]
            b = Bench(c, dname, dev, ins)
            w64 = lg.want(c.id, dtype, ins)
            bd = lg.bound(c, dtype, w64, ins)
            w64 = w64.to(dev)
            bd = bd if isinstance(bd, float) else bd.to(dev)
            try:
                got, guard_fails = b.run()
            except _lib.ArsegError as err:
                status = re.search(r"status (-?\d+)", str(err))
                if status and int(status.group(1)) > 0:          # a HIP error code, not a verdict: nothing more is launched
                    raise
                fails.append(f"{at}: refused: {err}")
                continue
            fails += [f"{at}: {f}" for f in guard_fails]
            if not b.operands_intact():
                fails.append(f"{at}: an input buffer changed")
            if tuple(got.shape) != tuple(w64.shape):
                fails.append(f"{at}: shape {tuple(got.shape)}, want {tuple(w64.shape)}")
                continue
            e = excess(got, w64, bd)
            worst = max(worst, (e, at))
            WORST[(op, dname)] = max(WORST.get((op, dname), (0.0, "")), (e, at))
            if not e <= 1.0:
                bad = ~lg.within(got.double(), w64, bd)
                where = [tuple(int(v) for v in i) for i in bad.nonzero()[:4]]
                fails.append(f"{at}: error {e:.3g} x the bound; {int(bad.sum())} of {bad.numel()} elements miss it, first at {where}")
                continue
            got = got.clone()
            got2, guard_fails = b.run()
            fails += [f"{at}: second run: {f}" for f in guard_fails]
            if not torch.equal(got, got2):
                fails.append(f"{at}: two runs differ by {float((got.double() - got2.double()).abs().max()):.3g}")
            ran.append((lg.route(c, dname), c.id, dname))
            del b, got, got2, w64, bd
        del ins
    torch.cuda.synchronize()
    _BROKEN.pop()
    for labels, _, _ in ran:
        for label in labels:
            RAN[label] = RAN.get(label, 0) + 1
    print(f"{cls} {op}: {len(ran)} launches checked; worst error {worst[0]:.3g} x its bound ({worst[1]})")
    for f in fails[:40]:
        print("  " + f)
    return fails, ran, worst


@pytest.mark.parametrize("cls,op", PAIRS)
def test_every_case_of_the_class(dev, cls, op):
    fails = sweep(cls, op)[0]
    assert not fails, f"{len(fails)} failures, the first: {fails[:10]}"


def test_every_route_ran_as_often_as_the_table_reaches_it(dev):
    """Coverage does not erode: on the device, every route label of lg.ALL_ROUTES was launched and checked on every (case, storage) pair the
    CPU test pins for it (lg.ROUTE_COUNTS) -- the four block-row forms, the 64-lane max, the fp32 row-walk prior sum, the rows ingest at two and
    three segments, the wide heads, each capped grid past its cap.  (The sweeps are computed once; run alone, this test computes them.)"""
    for cls, op in PAIRS:
        sweep(cls, op)
    for op in lg.OPS:
        print(f"{op}: worst error / bound " + ", ".join(f"{d} {WORST[(op, d)][0]:.3g} ({WORST[(op, d)][1].split()[0]})" for d in lg.ALL if (op, d) in WORST))
    assert set(lg.ROUTE_COUNTS) == set(lg.ALL_ROUTES)
    missing = {label: (RAN.get(label, 0), n) for label, n in lg.ROUTE_COUNTS.items() if RAN.get(label, 0) != n}
    assert not missing, missing
