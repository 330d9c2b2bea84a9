"""The dependency probe of tests/nonfinite.py, proven on torch's own functions: the real ones pass against themselves, and the two ways a
kernel goes wrong -- a max that drops the NaN, a result that hides it -- fail with a message that names the site and counts the outputs."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite as nf


def rnd(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


X = rnd(1, 2, 5, 9, 11)                  # NCHW
WGT = rnd(2, 4, 5, 3, 3) * 0.2
SITES = [(0, 2, 4, 5), (1, 4, 8, 10), (1, 0, 0, 0)]
EXACT = nf.within(1e-12)


def conv(x):
    return F.conv2d(x.double(), WGT.double(), padding=1)


OPS = {
    "relu": (lambda x: F.relu(x.double()), True, True),
    "max_pool2d": (lambda x: F.max_pool2d(x.double(), 3, 2, 1), True, True),
    "nearest": (lambda x: F.interpolate(x.double(), size=(14, 17), mode="nearest"), True, True),
    "bilinear": (lambda x: F.interpolate(x.double(), size=(13, 20), mode="bilinear", align_corners=True), True, False),
    "conv2d": (conv, True, True),
    "conv2d+relu": (lambda x: F.relu(conv(x)), True, True),
}


@pytest.mark.parametrize("site", SITES)
@pytest.mark.parametrize("name", sorted(OPS))
def test_real_functions_pass_against_themselves(name, site):
    f, exact, select = OPS[name]
    p = nf.run(name, lambda i: f(i["x"]), lambda i: f(i["x"]), {"x": X}, "x", site, EXACT, exact=exact, select=select)
    assert bool(p.D.any()) and not bool((p.D & ~p.T["nan"]).any())
    assert not bool(p.A.all())


def test_sets_of_a_relu_after_a_conv():
    """T \\ D: the outputs a ReLU clips under both probes depend on the site for a NaN only; D, T and the receptive field agree."""
    p = nf.Probe("conv2d+relu", lambda i: F.relu(conv(i["x"])), {"x": X}, "x", (0, 2, 4, 5))
    field = torch.zeros(2, 4, 9, 11, dtype=torch.bool)
    field[0, :, 3:6, 4:7] = True
    assert torch.equal(p.T["nan"], field)
    assert bool((p.T["nan"] & ~p.D).any()), "no output is clipped under both probes: the case shows nothing"
    # relu(-Inf * w) is 0 for w > 0: the reference itself is finite there, and (a) does not ask for more
    assert bool((p.D & ~p.T["-inf"]).any())


def test_fmax_relu_fails_c():
    """torch.fmax returns the operand that is not NaN, as fmaxf / v_max_f32 do: the "ReLU" turns the planted NaN into 0."""
    fake = lambda i: torch.fmax(i["x"].double(), torch.zeros((), dtype=torch.float64))
    with pytest.raises(AssertionError) as e:
        nf.run("fmax-relu", lambda i: F.relu(i["x"].double()), fake, {"x": X}, "x", (0, 2, 4, 5), EXACT, exact=True, values=("nan",))
    msg = str(e.value)
    assert msg.startswith("fmax-relu: x[0, 2, 4, 5] = nan: "), msg
    assert "(c) non-finite set differs from the reference's: 1 of 1 missed, 0 extra" in msg, msg
    # with (a) out of the way -- a site the probes clip, so D is empty there -- the same function still fails (c), and says how many
    p = nf.Probe("fmax-relu", lambda i: F.relu(conv(i["x"])), {"x": X}, "x", (0, 2, 4, 5))
    y = torch.fmax(conv(p.inputs["nan"]["x"]), torch.zeros((), dtype=torch.float64))
    y[p.D] = nf.NAN                                   # (a) holds by construction; the clipped outputs of T \ D stay 0
    with pytest.raises(AssertionError) as e:
        p.check("nan", y, EXACT, exact=True)
    n_clip = int((p.T["nan"] & ~p.D).sum())
    assert f"(c) non-finite set differs from the reference's: {n_clip} of {int(p.T['nan'].sum())} missed, 0 extra" in str(e.value), str(e.value)
    assert "fmax-relu: x[0, 2, 4, 5] = nan" in str(e.value)


def test_nan_to_num_after_conv_fails_a():
    fake = lambda i: torch.nan_to_num(conv(i["x"]), nan=0.0, posinf=0.0, neginf=0.0)
    for v in nf.PLANTS:
        with pytest.raises(AssertionError) as e:
            nf.run("conv-then-nan_to_num", lambda i: conv(i["x"]), fake, {"x": X}, "x", (1, 4, 8, 10), EXACT, values=(v,))
        assert f"conv-then-nan_to_num: x[1, 4, 8, 10] = {v}: (a) 16 of 16 outputs that depend on the site are finite" in str(e.value), str(e.value)


def test_leak_outside_the_allowed_set_fails_b():
    """A non-finite value outside A, and a finite one off the tolerance there, both fail (b)."""
    p = nf.Probe("conv2d", lambda i: conv(i["x"]), {"x": X}, "x", (0, 2, 4, 5))
    y = p.want["nan"].clone()
    y[1, 0, 0, 0] = nf.NAN
    with pytest.raises(AssertionError, match=r"\(b\) 1 outputs outside the allowed set \(36 of 792\) are non-finite"):
        p.check("nan", y, EXACT)
    y = p.want["nan"].clone()
    y[1, 0, 0, 0] += 1e-3
    with pytest.raises(AssertionError, match=r"\(b\) 1 outputs outside the allowed set miss the tolerance"):
        p.check("nan", y, EXACT)
    p.check("nan", y, nf.within(2e-3))


def test_select_checks_class_and_sign():
    p = nf.Probe("max_pool2d", lambda i: F.max_pool2d(i["x"].double(), 3, 2, 1), {"x": X}, "x", (0, 2, 4, 5))
    y = p.want["+inf"].clone()
    y[y == nf.INF] = nf.NAN                           # non-finite where it should be, of the wrong class
    p.check("+inf", y, EXACT, exact=True)
    with pytest.raises(AssertionError, match=r"\(c\) \d+ outputs are of another class"):
        p.check("+inf", y, EXACT, select=True)


def test_a_nan_that_comes_out_as_an_infinity_fails_c():
    """max(v, -inf) as the identity "activation": the NaN leaves as -Inf -- non-finite where it should be, and still wrong."""
    fake = lambda i: torch.fmax(conv(i["x"]), torch.full((), -nf.INF, dtype=torch.float64))
    with pytest.raises(AssertionError, match=r"conv-max-neginf: x\[0, 2, 4, 5\] = nan: \(c\) 36 outputs are infinite: the NaN did not stay a NaN"):
        nf.run("conv-max-neginf", lambda i: conv(i["x"]), fake, {"x": X}, "x", (0, 2, 4, 5), EXACT, exact=True, values=("nan",))
    nf.run("conv-max-neginf", lambda i: conv(i["x"]), fake, {"x": X}, "x", (0, 2, 4, 5), EXACT, exact=True, values=("+inf", "-inf"))


def test_allowed_set_may_grow_but_never_to_everything():
    f = lambda i: conv(i["x"])
    p = nf.Probe("tiles", f, {"x": X}, "x", (0, 2, 4, 5), grow=nf.grow_tiles(4, 4, hdim=2, wdim=3))
    want = torch.zeros(2, 4, 9, 11, dtype=torch.bool)
    want[0, :, 0:8, 4:8] = True                       # T = rows 3..5, cols 4..6 -> tile rows 0 and 1, tile column 1
    assert torch.equal(p.A, want)
    with pytest.raises(AssertionError, match="every output"):
        nf.Probe("all", f, {"x": X}, "x", (0, 2, 4, 5), grow=lambda T: torch.ones_like(T))
    with pytest.raises(AssertionError, match="does not hold T"):
        nf.Probe("less", f, {"x": X}, "x", (0, 2, 4, 5), grow=lambda T: torch.zeros_like(T))


def test_grow_tiles_on_a_dilation_lattice():
    T = torch.zeros(1, 10, 13, 1, dtype=torch.bool)
    T[0, 5, 9, 0] = True                              # d = 4: residues (1, 1), lattice index (1, 2) -> tile (0, 0): y in {1, 5, 9}, x in {1, 5, 9}
    A = nf.grow_tiles(4, 4, d=4)(T)
    want = torch.zeros_like(T)
    for y in (1, 5, 9):
        for x in (1, 5, 9):
            want[0, y, x, 0] = True
    assert torch.equal(A, want)


def test_sites_nhwc():
    s = nf.sites_nhwc((2, 9, 50, 36), 32)
    assert s["corner"] == (1, 8, 49, 0) and s["lastvec"][3] == 35 and 0 < s["interior"][1] < 8 and 0 < s["interior"][2] < 49
