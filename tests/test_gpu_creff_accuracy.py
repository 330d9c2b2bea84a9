"""Every CReFF kernel held to fp32-grade error against fp64 and to its operand range (tests/creff_accuracy.py; tests/test_creff_accuracy.py
proves on the CPU that these bounds pass the correct split-fp16 arithmetic and fail a lost low half of K, V, P, Q or Wf and a dropped
cross term).  In range ("normal", "wide", "high"): e = max|got - want| / max|want| <= margin x e32 for p and for the logits, e32 the error of
the plain float32 loop on the same inputs.  "low": the same plus the 2^-24 floor of the format.  "over": against V clamped to +-131008,
e <= 2^-10 + margin x e32, nothing NaN or Inf, and the same call on the feature clamped to +-65504 meets the in-range bound.

The table: ops.creff pinned to the fp32 VALU kernel (the fp32 arithmetic itself, held to the same bound) and to creff_mfma with 16- and
8-row tiles, at C = 64 and 128; ops.creff_warp (fp32) pinned to the rolling kernel under three schedules and to the tile kernel, both output
layouts; heads of 0, 12 (log_softmax) and 19 classes on every kernel that serves them.  The 16-bit direct route is not in the table:
test_gpu_creff16.py::test_direct_equals_cast_once_bit_for_bit ties it bit for bit to the fp32 instantiation that this table covers.  The
wrappers allocate p and the logits themselves, so no output can start as NaN here; a NaN or an Inf in a result fails its row.  A fallback
of creff_mfma to the VALU kernel (the library falls back silently for shapes creff_mfma refuses) is seen by p being bit-equal to the VALU
result; nothing here tells mfma8 from mfma16 -- their figures are equal in every column, so a creff_tile_rows that was ignored would go
unnoticed by this file (test_gpu_ops.py::test_creff_vs_oracle pins both tile heights on ragged shapes).

Every test prints the figures it asserts (route, e, e / e32, margin); ``pytest -s`` shows them."""
import collections
import functools

import pytest
import torch

import creff_accuracy as ca

pytestmark = pytest.mark.gpu

CREFF = [(c.id, d, g) for c in ca.CASES if c.entry == "creff" for d in ca.DISTS for g in ca.GAINS]
WARP = [(c.id, d, g) for c in ca.CASES if c.entry == "warp" for d in ca.DISTS for g in ca.GAINS]
# route -> the knobs that pin it
CREFF_ROUTES = {"creff:valu": dict(creff_impl="valu", creff_tile_rows=0), "creff:mfma16": dict(creff_impl="mfma", creff_tile_rows=16),
                "creff:mfma8": dict(creff_impl="mfma", creff_tile_rows=8)}
WARP_ROUTES = {"warp:roll": dict(creff_warp_impl="roll", creff_seg_rows=0, creff_max_wgs=0),
               "warp:roll/seg6x3": dict(creff_warp_impl="roll", creff_seg_rows=6, creff_max_wgs=3),
               "warp:roll/wgs5": dict(creff_warp_impl="roll", creff_seg_rows=0, creff_max_wgs=5),
               "warp:tiles": dict(creff_warp_impl="tiles", creff_seg_rows=0, creff_max_wgs=0)}
# the head widths a kernel serves (tests/test_host_config.py::test_creff_dispatch_table: the rolling kernel has no 17-32-class head)
SERVES = {r: ((0, 12) if "roll" in r else ca.HEADS) for r in list(CREFF_ROUTES) + list(WARP_ROUTES)}

Row = collections.namedtuple("Row", "route what head e e32 margin bound problem")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def on_device(case_id, dist, gain, clamp=False):
    """(PackedAttention, keyframe feature(s), lr NHWC, {n_cls: head or None}, mvq or None) of a case on the device.  ops.creff: the feature in
    C8; ops.creff_warp: the un-warped features NHWC [Hp, Wp, C], one per frame (frames 0 and 2 share one tensor)."""
    from arseg_amd import _lib, ops
    from arseg_amd.model import MyAttention
    from arseg_amd.packing import PackedAttention

    c, ins, dev = ca.BY_ID[case_id], ca.inputs(case_id, dist, gain, clamp), torch.device("cuda:0")
    m = MyAttention(c.C, kW=7, kH=7)
    m.load_state_dict(ins["sd"])
    heads = {0: None}
    heads.update({n: (wf.to(dev), bf.to(dev)) for n, (wf, bf) in ins["heads"].items()})
    lr = ops.to_nhwc(ins["lr"].to(dev))
    if c.entry == "creff":
        return PackedAttention(m, dev), ops.to_c8(ins["hr"].to(dev), _lib.NCHW), lr, heads, None
    refs = [r.permute(1, 2, 0).contiguous().to(dev) for r in ins["refs"][:2]]
    return PackedAttention(m, dev), [refs[0], refs[1], refs[0]], lr, heads, ins["mvq"].to(dev)


class Table:
    """The rows of one (case, distribution, gain): what ran, its error and bound, and what went wrong."""

    def __init__(self, case_id, dist, gain):
        self.case_id, self.dist, self.gain, self.rows = case_id, dist, gain, []

    def add(self, route, what, n_cls, got, clamp=False):
        """got: {0: p NCHW, n_cls: logits} or a string saying what went wrong.  The fp32 VALU kernel does not split and so does not clamp:
        "over" is in range for it."""
        if isinstance(got, str):
            self.rows.append(Row(route, what, n_cls, float("nan"), float("nan"), 0.0, float("nan"), got))
            return
        split = route != "creff:valu" or self.dist != "over"
        y = ca.yardstick(self.case_id, self.dist, self.gain, clamp, split)
        for n in sorted(got):
            m = ca.margin(self.case_id, self.dist, self.gain, route, n)
            floor = ca.low_floor(self.case_id, self.gain, n) if self.dist == "low" else 0.0
            e, prob = ca.problem(self.dist, got[n], y.want[n], y.e32[n], m, floor, clamp or not split)
            bound = ca.bound_of(self.dist, y.want[n], y.e32[n], m, floor, clamp or not split)
            self.rows.append(Row(route, what + (" clamped" if clamp else "") + (" logits" if n else " p"), n_cls, e, y.e32[n], m, bound, prob))


def settle(tab):
    """Print the rows, return them; the caller asserts."""
    for r in tab.rows:
        print(f"{tab.case_id:5s} {tab.dist:6s} {tab.gain:4g} {r.route:16s} {r.what:24s} e = {r.e:.3g} = {r.e / r.e32:5.2f} x e32 ({r.e32:.3g}), margin {r.margin:g}, {r.e / r.bound:4.2f} of the bound {r.problem}")
    return tab.rows


def failures(rows):
    return [f"{r.route} {r.what}: {r.problem}" for r in rows if r.problem]


# ---------------------------------------------------------------------------------------------- the groups, each computed once
@functools.lru_cache(maxsize=None)
def creff_routes(case_id, dist, gain):
    """ops.creff pinned to each of its kernels, every head; "over" also on the clamped feature"""
    from arseg_amd import _lib, ops

    tab = Table(case_id, dist, gain)
    for clamp in ((False, True) if dist == "over" else (False,)):
        pa, hr_c8, lr, heads, _ = on_device(case_id, dist, gain, clamp)
        valu = {}
        for route, knobs in CREFF_ROUTES.items():
            for n in SERVES[route]:
                prev = ops.configure(**knobs)
                try:
                    p_c8, logits = ops.creff(hr_c8, lr, pa, heads[n], ca.LOGSM[n], 7, 7)
                finally:
                    ops.configure(**prev)
                if (logits is None) != (n == 0):
                    tab.add(route, f"head {n}", n, "logits returned without a head, or none with one")
                    continue
                if route == "creff:valu":
                    valu[n] = p_c8
                elif torch.equal(p_c8, valu[n]):          # the library falls back to the VALU kernel for shapes creff_mfma refuses
                    tab.add(route, f"head {n}", n, "bit-equal to the VALU kernel: the matrix-core kernel did not run")
                    continue
                got = {0: ops.from_c8(p_c8, _lib.NCHW)}
                if n:
                    got[n] = logits
                tab.add(route, f"head {n}", n, got, clamp)
    return settle(tab)


@functools.lru_cache(maxsize=None)
def warp_routes(case_id, dist, gain):
    """ops.creff_warp (fp32) pinned to the rolling kernel under three schedules and to the tile kernel, every head the kernel serves, both
    output layouts; "over" also on the clamped feature"""
    from arseg_amd import _lib, ops

    c, tab = ca.BY_ID[case_id], Table(case_id, dist, gain)
    for clamp in ((False, True) if dist == "over" else (False,)):
        pa, refs, lr, heads, mvq = on_device(case_id, dist, gain, clamp)
        for route, knobs in WARP_ROUTES.items():
            for n in SERVES[route]:
                for layout in ("c8", "nhwc"):
                    prev = ops.configure(**knobs)
                    try:
                        kernel = ops.creff_warp_kernel(c.B, c.C, c.Hp, c.Wp, c.hp, c.wp, n)
                        p, logits = ops.creff_warp(refs, mvq, lr, pa, heads[n], ca.LOGSM[n], 7, 7, p_layout=_lib.C8 if layout == "c8" else _lib.NHWC)
                    finally:
                        ops.configure(**prev)
                    what = f"head {n} {layout}"
                    if kernel != knobs["creff_warp_impl"]:
                        tab.add(route, what, n, f"ran on {kernel}")
                        continue
                    got = {0: ops.from_c8(p, _lib.NCHW) if layout == "c8" else p.permute(0, 3, 1, 2)}
                    if n:
                        got[n] = logits
                    tab.add(route, what, n, got, clamp)
    return settle(tab)


GROUPS = [(creff_routes, CREFF), (warp_routes, WARP)]


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("case_id,dist,gain", CREFF)
def test_creff_kernels(dev, case_id, dist, gain):
    assert not failures(creff_routes(case_id, dist, gain))


@pytest.mark.parametrize("case_id,dist,gain", WARP)
def test_fused_warp_kernels(dev, case_id, dist, gain):
    assert not failures(warp_routes(case_id, dist, gain))


def test_every_route_ran_under_each_distribution_with_every_head_it_serves(dev):
    """Coverage does not erode: every route produced checked rows under each distribution, for p and for the logits of every head width its
    kernel serves, the fused routes in both layouts, "over" also on the clamped feature (the groups are computed once; run alone, this test
    computes them)."""
    ran = {d: set() for d in ca.DISTS}
    for group, params in GROUPS:
        for case_id, dist, gain in params:
            ran[dist] |= {(r.route, r.what) for r in group(case_id, dist, gain) if r.margin > 0}
    for d in ca.DISTS:
        missing = []
        for route in list(CREFF_ROUTES) + list(WARP_ROUTES):
            for n in SERVES[route]:
                for layout in (("",) if route in CREFF_ROUTES else (" c8", " nhwc")):
                    for cl in (("", " clamped") if d == "over" else ("",)):
                        for out in ((" p", " logits") if n else (" p",)):
                            if (route, f"head {n}{layout}{cl}{out}") not in ran[d]:
                                missing.append((route, n, layout, cl, out))
        assert not missing, (d, missing)
