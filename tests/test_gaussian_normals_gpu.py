"""GPU checks of bags_raster.gaussian_normals / gaussian_normals_views (csrc/gaussian_normals.hip) against the PyTorch statement in
float32 and float64 on the named cases of tests/gaussian_normals_cases.py: forward and backward for one view and for many, the
host's chunking above 16 views, cloud sizes either side of a wave and a workgroup, and the independence and repeatability of every
output."""
import functools

import pytest
import torch

import gaussian_normals_cases as K
from bags_raster import gaussian_normals, gaussian_normals_views, gaussian_normals_views_torch
from scenes import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SLACK = 3.0                                       # parity.assert_ill_conditioned: the project's slack for ill-conditioned cases
WELL = ("generic", "scaled_view", "disks", "log_scales", "ties", "dead")


def _mask(name, P, masked):
    """The rows that keep their cotangent where a case takes rows out of all three sides: `grazing` the rows whose sigma differs
    between the statements, `dead` the rows that are dead in float32 (|q| = 1e-25 is alive in float64, with a gradient of 1e25)."""
    if not masked:
        return None
    return (~K.dead_rows() if name == "dead" else ~K.sigma_flips(name))[:P]


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, P=K.P_FULL, V=1, masked=False, zero_block=False):
    """The statement on the CPU, computed once per (case, dtype, size): shared by the tests, never written to."""
    mask = _mask(name, P, masked)
    return K.forward_backward(gaussian_normals_views_torch, name, dtype, "cpu", P, V, mask, zero_block)


def _hip(name, P=K.P_FULL, V=1, masked=False, zero_block=False):
    mask = _mask(name, P, masked)
    outs, grads = K.forward_backward(gaussian_normals_views, name, F32, DEV, P, V, mask, zero_block)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], {n: g.cpu() for n, g in grads.items()}


def _check(name, P, V, masked=False, keep=None):
    """Forward <= 1e-5 (1 + |x|) against float64 (and float32), every gradient tensor <= 1e-4 (scenes.rel_err) against float64
    autograd; an ill-conditioned case: SLACK x the float32 statement's own error plus the bar.  Returns the worst error over bar."""
    o64, g64 = _reference(name, F64, P, V, masked)
    o32, g32 = _reference(name, F32, P, V, masked)
    outs, grads = _hip(name, P, V, masked)
    keep = torch.ones(P, dtype=torch.bool) if keep is None else keep
    worst = 0.0
    for v in range(V):
        assert outs[v].shape == (P, 3) and outs[v].dtype == F32 and torch.isfinite(outs[v]).all()
        d64 = ((outs[v].double() - o64[v]).abs() / (1 + o64[v].abs()))[keep]
        d32 = ((outs[v].double() - o32[v].double()).abs() / (1 + o32[v].double().abs()))[keep]
        ref = ((o32[v].double() - o64[v]).abs() / (1 + o64[v].abs()))[keep].max().item()
        print("\n%s P=%d view %d/%d forward: |hip - f64| %.2e  |hip - f32| %.2e  |f32 - f64| %.2e  bitwise equal to f32 on %d of %d rows"
              % (name, P, v, V, d64.max().item(), d32.max().item(), ref, int((outs[v] == o32[v]).all(1)[keep].sum()), int(keep.sum())))
        bar = 1e-5 if name in WELL else SLACK * ref + 1e-5
        assert d64.max().item() <= bar and (name not in WELL or d32.max().item() <= 1e-5)
        worst = max(worst, d64.max().item() / bar)
    assert set(grads) == set(g64)
    for n in g64:
        err, ref32 = rel_err(grads[n], g64[n]), rel_err(g32[n], g64[n])
        print("%s P=%d V=%d backward %s: %.2e (f32 statement %.2e)" % (name, P, V, n, err, ref32))
        assert torch.isfinite(grads[n]).all(), n
        bar = 1e-4 if name in WELL else SLACK * ref32 + 1e-4
        assert err <= bar, (n, err, ref32)
        worst = max(worst, err / bar)
        if n != "rotations":                       # what nothing depends on is written as zeros, not left as it was
            assert (grads[n][3] == 0).all() and (grads[n][:, 3] == 0).all() and grads[n][:3, :3].abs().max() > 0
    print("%s P=%d V=%d: worst error over bar %.3f" % (name, P, V, worst))
    return outs, grads


@pytest.mark.parametrize("name", ("generic", "scaled_view", "disks", "ties"))
def test_one_view_forward_and_backward(name):
    """Measured on an MI355X (the test prints every figure; table in profiles/gaussian_normals/NOTES.md): the forward equals the
    float32 statement bit for bit on every row of every case and is 1.0e-7 to 1.2e-7 from float64; dL/drotations is 1.2e-7 from
    float64 autograd (the float32 statement: 1.3e-7), the view-matrix gradients at most 2.8e-7; worst error over bar 0.012."""
    _check(name, K.P_FULL, 1)


def test_log_scales_give_the_bits_of_the_scales():
    a, ga = _check("log_scales", K.P_FULL, 1)
    b, gb = _hip("generic")
    assert torch.equal(a[0], b[0]) and all(torch.equal(ga[n], gb[n]) for n in ga)


def test_ties_follow_the_first_minimum_row_by_row():
    """The three columns of Q are orthogonal: a row that took another axis is off by sqrt(2), not by 1e-5."""
    c = K.case("ties")
    s = c["scales"]
    tied = (s[:, 0] == s[:, 1]) | (s[:, 1] == s[:, 2]) | (s[:, 0] == s[:, 2])
    assert int(tied.sum()) >= K.P_FULL // 3
    out = _hip("ties")[0][0].double()
    R = torch.nn.functional.normalize(c["rotations"].double(), dim=1)
    w, x, y, z = R.unbind(1)
    cols = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], 1),
                        torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], 1),
                        torch.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], 1)], 1)      # (P, k, 3)
    axis = cols[torch.arange(K.P_FULL), K.first_minimum(s)] @ c["views"][0].double()[:3, :3]
    assert ((out * axis).sum(1).abs() >= 1 - 1e-5).all()


@pytest.mark.parametrize("zero_block", (False, True), ids=("rigid", "zero_block"))
def test_dead_rows_are_zeros_with_zero_gradients_and_nothing_is_nan(zero_block):
    dead = torch.ones(K.P_FULL, dtype=torch.bool) if zero_block else K.dead_rows()
    if not zero_block:
        _check("dead", K.P_FULL, 1, masked=True, keep=~dead)           # the other rows stay within the bars
    outs, grads = _hip("dead", V=2, zero_block=zero_block)             # every row has a cotangent
    for o in outs:
        assert (o[dead] == 0).all() and torch.isfinite(o).all()
    assert (grads["rotations"][dead] == 0).all() and torch.isfinite(grads["rotations"]).all()
    assert zero_block or grads["rotations"][~dead].abs().max(1).values.min() > 0
    for n, g in grads.items():
        assert torch.isfinite(g).all(), n
        if zero_block:
            assert (g == 0).all(), n


def test_grazing_without_the_rows_whose_sigma_flips():
    flips = K.sigma_flips("grazing")
    assert int(flips.sum()) <= K.P_FULL // 100
    _check("grazing", K.P_FULL, 1, masked=True, keep=~flips)


@pytest.mark.parametrize("V", (2, 5, 16))
@pytest.mark.parametrize("name", ("generic", "scaled_view"))
def test_many_views(name, V):
    views, cots = K.case(name)["views"][:V], K.cotangents(K.P_FULL, V)
    assert all(not torch.equal(views[a], views[b]) and not torch.equal(cots[a], cots[b]) for a in range(V) for b in range(a))
    _check(name, K.P_FULL, V)


def test_seventeen_views_are_a_sixteen_view_call_and_a_one_view_call():
    lv = K.leaves("generic", F32, DEV, V=17)
    cots = [c.to(DEV, F32) for c in K.cotangents(K.P_FULL, 17)]
    q, s, x, views = lv["rotations"], lv["scales"], lv["means3D"], lv["views"]
    outs = gaussian_normals_views(q, s, x, views)
    g17 = torch.autograd.grad(list(outs), [q] + views, cots)
    a = gaussian_normals_views(q, s, x, views[:16])
    ga = torch.autograd.grad(list(a), [q] + views[:16], cots[:16])
    b = gaussian_normals(q, s, x, views[16])
    gb = torch.autograd.grad(b, [q, views[16]], cots[16])
    assert len(outs) == 17 and all(torch.equal(o, r) for o, r in zip(outs, list(a) + [b]))
    assert torch.equal(g17[0], ga[0] + gb[0])
    assert all(torch.equal(g, r) for g, r in zip(g17[1:], list(ga[1:]) + [gb[1]]))
    ref = _reference("generic", F64, K.P_FULL, 17)[1]
    assert rel_err(g17[0], ref["rotations"]) <= 1e-4 and rel_err(g17[17], ref["view16"]) <= 1e-4


@pytest.mark.parametrize("P", K.SIZES)
def test_cloud_sizes_either_side_of_a_wave_and_a_workgroup(P):
    o64, g64 = _reference("scaled_view", F64, P, 2)
    outs, grads = _hip("scaled_view", P, 2)
    for v in range(2):
        assert outs[v].shape == (P, 3) and ((outs[v].double() - o64[v]).abs() <= 1e-5 * (1 + o64[v].abs())).all()
    for n in g64:
        assert tuple(grads[n].shape) == tuple(g64[n].shape) and rel_err(grads[n], g64[n]) <= 1e-4, (n, rel_err(grads[n], g64[n]))


def test_no_rows():
    outs, grads = _hip("generic", 0, 2)
    assert all(o.shape == (0, 3) for o in outs) and grads["rotations"].shape == (0, 4)
    assert all(grads["view%d" % v].shape == (4, 4) and (grads["view%d" % v] == 0).all() for v in range(2))


def test_a_view_does_not_depend_on_its_neighbours():
    """View 3 of `scaled_view` alone, first, last and in the middle of a call: the same output and the same matrix gradient, bit for
    bit.  (dL/drotations is a sum over the views of the call.)"""
    c = K.case("scaled_view")
    q, s, x = (c[n].to(DEV) for n in ("rotations", "scales", "means3D"))
    cot = K.cotangents(K.P_FULL, 4)[3].to(DEV, F32)
    results = []
    for order in ([3], [3, 0, 1], [0, 1, 3], [5, 3, 6, 7, 8], list(range(4, 16)) + [3, 0, 1, 2]):
        views = [c["views"][v].to(DEV).requires_grad_() for v in order]
        outs = gaussian_normals_views(q, s, x, views)
        at = order.index(3)
        (g,) = torch.autograd.grad(list(outs), [views[at]], [cot if k == at else torch.zeros_like(cot) for k in range(len(order))])
        results.append((outs[at].detach(), g))
    for o, g in results[1:]:
        assert torch.equal(o, results[0][0]) and torch.equal(g, results[0][1])
    assert results[0][1].abs().max() > 0


def test_a_view_no_loss_uses_is_a_zero_cotangent():
    """Its cotangent arrives as None and goes down as NULL: the same bits as an explicit zero cotangent, and a zero matrix gradient."""
    cots = [c.to(DEV, F32) for c in K.cotangents(K.P_FULL, 3)]

    def grads(unused):
        lv = K.leaves("scaled_view", F32, DEV, V=3)
        outs = gaussian_normals_views(lv["rotations"], lv["scales"].detach(), lv["means3D"].detach(), lv["views"])
        if unused:
            return torch.autograd.grad([outs[0], outs[2]], [lv["rotations"]] + lv["views"], [cots[0], cots[2]], allow_unused=True)
        return torch.autograd.grad(list(outs), [lv["rotations"]] + lv["views"], [cots[0], torch.zeros_like(cots[1]), cots[2]])

    a, b = grads(True), grads(False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert (a[2] == 0).all() and a[1].abs().max() > 0 and a[3].abs().max() > 0
    # no view used at all: nothing is launched, every gradient is None
    lv = K.leaves("scaled_view", F32, DEV, V=2)
    outs = gaussian_normals_views(lv["rotations"], lv["scales"].detach(), lv["means3D"].detach(), lv["views"])
    extra = (lv["rotations"] * 2.0).sum()
    g = torch.autograd.grad(extra + 0.0 * sum(o.detach().sum() for o in outs), [lv["rotations"]] + lv["views"], allow_unused=True)
    assert g[1] is None and g[2] is None


def test_two_runs_give_the_same_bits():
    a_out, a = _hip("scaled_view", V=5)
    b_out, b = _hip("scaled_view", V=5)
    assert all(torch.equal(x, y) for x, y in zip(a_out, b_out))
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_a_wanted_gradient_does_not_depend_on_which_others_are_wanted():
    cots = [c.to(DEV, F32) for c in K.cotangents(K.P_FULL, 3)]

    def grads(wanted):
        lv = K.leaves("generic", F32, DEV, V=3)
        named = {"rotations": lv["rotations"], "view0": lv["views"][0], "view1": lv["views"][1], "view2": lv["views"][2]}
        for n, t in named.items():
            t.requires_grad_(n in wanted)
        outs = gaussian_normals_views(lv["rotations"], lv["scales"].detach(), lv["means3D"].detach(), lv["views"])
        return dict(zip(wanted, torch.autograd.grad(list(outs), [named[n] for n in wanted], cots)))

    full = grads(("rotations", "view0", "view1", "view2"))
    for wanted in (("rotations",), ("view1",), ("view0", "view2"), ("rotations", "view2")):
        part = grads(wanted)
        for n in wanted:
            assert torch.equal(part[n], full[n]), (wanted, n)
