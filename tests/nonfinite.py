"""Dependency probe for NaN / Inf propagation (a plain helper module; DESIGN.md section 2, "Non-finite values").

An op ``f`` has a torch CPU reference ``ref(inputs) -> fp64 tensor`` over a dict of finite input tensors.  One float tensor of the dict is
chosen for planting, and one site ``s`` (an index tuple) in it.  ``probe`` runs the reference five times and derives, per output element:

  T[v]   the reference of the input with x[s] = v is non-finite there, v in {NaN, +Inf, -Inf};  T = T[NaN]
  D      the reference differs between x[s] = +3 and x[s] = -5 by more than 1e-9 * max|out| (the reference is fp64 and the sums have at most
         ~1e4 terms: rounding noise is <= 1e-12) -- the outputs that depend on the site with non-zero weight.  D is a subset of T (asserted:
         a reference that breaks it is no reference for this probe).  T \\ D holds weight-0 bilinear taps (0 * NaN) and outputs a ReLU clips
         under both probes.
  A      the allowed set: T, unless the op computes in tiles wider than its receptive field and states a larger one with its reason
         (``grow``).  Never everything.

``check`` holds a result ``y`` of the op under test, computed from the same planted input, to:

  (a)  y is non-finite on D (for an infinite plant: on D & T[v] -- max(-Inf, ..) and relu(-Inf) are finite in the reference itself, and an
       output the reference keeps finite cannot be asked to be non-finite);
  (b)  outside A, y is finite and ``close`` to the reference of the planted input (the tolerance of the op's own test, passed in);
  (c)  a NaN stays a NaN: under a NaN plant y is infinite nowhere (every op, every number format -- an Inf may become a NaN, as in the hi/lo
       split of the split-fp16 convs, never the other way round);  ``exact``: the non-finite set of y equals T for a NaN plant;  ``select``:
       for all three plants the class of y (finite / NaN / +Inf / -Inf) equals the reference's everywhere.

A failure names the op, the planted tensor, the site and the value, lists every property that missed and counts the outputs."""
import torch

NAN, INF = float("nan"), float("inf")
PLANTS = {"nan": NAN, "+inf": INF, "-inf": -INF}
PROBE_HI, PROBE_LO = 3.0, -5.0
DEP_EPS = 1e-9


def klass(t):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf, elementwise."""
    t = t.detach().cpu().double()
    k = torch.zeros(t.shape, dtype=torch.int8)
    k[torch.isnan(t)] = 1
    k[t == INF] = 2
    k[t == -INF] = 3
    return k


def planted(inputs, key, site, value):
    """A copy of ``inputs`` whose tensor ``key`` has ``value`` at ``site``; the other tensors are shared, never written."""
    out = dict(inputs)
    x = inputs[key].clone()
    x[tuple(site)] = value
    out[key] = x
    return out


class Probe:
    """The reference side of one (op, planted tensor, site): see the module docstring."""

    def __init__(self, name, ref, inputs, key, site, grow=None):
        self.name, self.key, self.site = name, key, tuple(int(i) for i in site)
        assert inputs[key].is_floating_point(), f"{name}: {key} is no float tensor"
        for k, v in inputs.items():
            assert not torch.is_tensor(v) or not v.is_floating_point() or bool(torch.isfinite(v.float()).all()), f"{name}: input {k} is not finite"
        self.inputs = {v: planted(inputs, key, self.site, val) for v, val in PLANTS.items()}
        self.want = {v: ref(self.inputs[v]).detach().double() for v in PLANTS}
        self.T = {v: ~torch.isfinite(self.want[v]) for v in PLANTS}
        hi = ref(planted(inputs, key, self.site, PROBE_HI)).detach().double()
        lo = ref(planted(inputs, key, self.site, PROBE_LO)).detach().double()
        assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all()), f"{name}: the reference of a finite input is not finite"
        scale = max(float(hi.abs().max()), float(lo.abs().max()))
        self.D = (hi - lo).abs() > DEP_EPS * scale
        assert bool(self.D.any()), f"{self.where()}: no output depends on the site"
        assert not bool((self.D & ~self.T["nan"]).any()), f"{self.where()}: the reference keeps {int((self.D & ~self.T['nan']).sum())} dependent outputs finite under a NaN"
        self._allowed = {}
        self.A = self.allowed(grow)

    def allowed(self, grow=None):
        """The allowed set under ``grow`` (None: T itself), held to: it contains T, and it is not every output."""
        if grow not in self._allowed:
            A = self.T["nan"] if grow is None else grow(self.T["nan"])
            assert A.shape == self.D.shape and not bool((self.T["nan"] & ~A).any()), f"{self.where()}: the allowed set does not hold T"
            assert not bool(A.all()), f"{self.where()}: the allowed set is every output -- the entry checks nothing"
            self._allowed[grow] = A
        return self._allowed[grow]

    def where(self, value=None):
        s = f"{self.name}: {self.key}{list(self.site)}"
        return s if value is None else f"{s} = {value}"

    def check(self, value, y, close, exact=False, select=False, grow=None):
        """(a)-(c) for the result ``y`` computed from ``self.inputs[value]``.  ``close(got, want) -> bool tensor``: True where |got - want|
        is within the op's tolerance (both fp64, the elements outside A only).  ``grow``: the allowed set of this result, where one probe
        serves several kernels (default: the probe's own)."""
        A = self.A if grow is None else self.allowed(grow)
        w = self.where(value)
        y = y.detach().cpu().double()
        want, T = self.want[value], self.T[value]
        assert y.shape == want.shape, f"{w}: result {tuple(y.shape)}, reference {tuple(want.shape)}"
        bad = ~torch.isfinite(y)
        fails = []
        need = self.D & T
        miss = need & ~bad
        if bool(miss.any()):
            fails.append(f"(a) {int(miss.sum())} of {int(need.sum())} outputs that depend on the site are finite")
        out = ~A
        leak = out & bad
        if bool(leak.any()):
            fails.append(f"(b) {int(leak.sum())} outputs outside the allowed set ({int(A.sum())} of {A.numel()}) are non-finite")
        ok = close(y[out], want[out]) | leak[out]
        if not bool(ok.all()):
            err = (y[out] - want[out]).abs()
            fails.append(f"(b) {int((~ok).sum())} outputs outside the allowed set miss the tolerance, max |err| {float(err[~leak[out]].max()):.3g}")
        if value == "nan":
            turned = torch.isinf(y) & ~torch.isinf(want)
            if bool(turned.any()):
                fails.append(f"(c) {int(turned.sum())} outputs are infinite: the NaN did not stay a NaN")
        if exact and value == "nan":
            dropped, extra = T & ~bad, bad & ~T
            if bool(dropped.any()) or bool(extra.any()):
                fails.append(f"(c) non-finite set differs from the reference's: {int(dropped.sum())} of {int(T.sum())} missed, {int(extra.sum())} extra")
        if select:
            ky, kw = klass(y), klass(want)
            diff = ky != kw
            if bool(diff.any()):
                fails.append(f"(c) {int(diff.sum())} outputs are of another class (finite / NaN / +Inf / -Inf) than the reference's "
                             f"({int((kw != 0).sum())} non-finite there)")
        assert not fails, f"{w}: " + "; ".join(fails)


def run(name, ref, call, inputs, key, site, close, exact=False, select=False, grow=None, values=tuple(PLANTS)):
    """Probe one site and check ``call(inputs) -> tensor`` for every plant.  Returns the probe (its sets, for a test that wants to look)."""
    p = Probe(name, ref, inputs, key, site, grow)
    for v in values:
        p.check(v, call(p.inputs[v]), close, exact=exact, select=select)
    return p


def within(atol, rtol=0.0):
    return lambda got, want: (got - want).abs() <= atol + rtol * want.abs()


def sites_nhwc(shape, vec):
    """The three sites of an NHWC (or any channels-last) tensor: interior, corner, and channel C-1 -- the last element of the last ``vec``-wide
    channel vector, a tail one where C is no multiple of ``vec`` -- at an interior pixel of the last image."""
    n, h, w, c = shape
    return {"interior": (0, h // 2, w // 2, min(c // 2 + 1, c - 1)), "corner": (n - 1, h - 1, w - 1, 0), "lastvec": (n - 1, max(h // 2 - 1, 0), max(w // 2 - 1, 0), c - 1)}


def grow_tiles(th, tw, d=1, hdim=1, wdim=2):
    """T grown to whole th x tw output tiles on the dilation-``d`` lattice (tile origin at 0; y = d * (th * ty + i) + ry): the allowed set of a
    kernel whose arithmetic mixes a whole tile, e.g. Winograd F(4,3)."""
    def groups(n, t):          # one-hot [n, groups]: positions of one tile row (column) of one lattice residue share a group
        pos = torch.arange(n)
        key = (pos % d) * (n // (d * t) + 1) + (pos // d) // t
        return (key[:, None] == key.unique()[None, :]).double()

    def grow(T):
        t = T.movedim((hdim, wdim), (-2, -1)).double()
        gy, gx = groups(t.shape[-2], th), groups(t.shape[-1], tw)
        hit = gy.T @ t @ gx                                   # [..., tile rows, tile columns]: elements of T in the tile
        return ((gy @ hit @ gx.T) > 0).movedim((-2, -1), (hdim, wdim)) | T
    return grow
