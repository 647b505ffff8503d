"""GPU checks of the regularisers on the Gaussians: bags_raster.gaussian_reg_loss / GaussianBag.regularizers (csrc/gaussian_reg.hip)
against gaussian_reg_loss_torch in float64 on the cases of tests/gaussian_reg_cases.py, held to that module's bars on every row; the
bitwise properties of its sums, its subsets, its placements and its optional outputs; the degenerate inputs; the bag's method; and
the chain render() + regularisers -> backward -> GaussianAdam."""
import ctypes as C

import pytest
import torch

import gaussian_reg_cases as G
from bags_raster import GaussianAdam, PipelineParams, REG_TERMS, _lib as L, gaussian_reg_loss, render
from bags_raster.gaussians import GaussianBag
from bags_raster.synth import look_at_origin_camera
from scenes import make_case as make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
COMBO_IDS = ["%s-%s" % ("filtered" if f else "plain", "mask" if s else "all") for f, s in G.COMBOS]
NAMES = ("terms", "dL/d_opacity", "dL/d_scaling")
MID, LARGE = G.ROWS_PER_GROUP + 1, 3 * G.ROWS_PER_GROUP + 17


def _place(t, offset):
    """``t`` as a GPU tensor of its dtype: at the start of an allocation (16-byte aligned), or -- ``offset`` -- as a view one element
    (float32: 4 bytes) into a larger one, which no access wider than an element may touch."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=t.dtype, device=DEV)
    v = (buf[1:1 + n] if offset else buf[:n]).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (t.element_size() if offset else 0) and v.is_contiguous()
    return v


def _inputs(c, offset=False):
    return (_place(c["opacity"], offset), _place(c["scaling"], offset), _place(c["filter"], offset) if c["filtered"] else None,
            _place(c["sel"], offset) if c["selected"] else None)


def _run(c, offset=False, terms=REG_TERMS, cot=None):
    """Forward and backward through autograd for L = sum_k cot_k terms_k: (terms (6,), dL/d_opacity (P,1), dL/d_scaling (P,3), count)
    on the host."""
    x, r, f, sel = _inputs(c, offset)
    x.requires_grad_(True), r.requires_grad_(True)
    out, count = gaussian_reg_loss(x, r, f, sel, terms, G.MAX_RATIO, G.MAX_SCALE)
    assert tuple(out.shape) == (6,) and tuple(count.shape) == () and out.dtype == F32 and out.grad_fn is not None and not count.requires_grad
    g_x, g_r = torch.autograd.grad(out, [x, r], (c["cot"] if cot is None else cot).to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), g_x.cpu(), g_r.cpu(), count.cpu()


def _same(a, b, what=""):
    for x, y, name in zip(a, b, NAMES + ("count",)):
        assert torch.equal(x, y), (what, name)


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("filtered,selected", G.COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("P", G.SIZES)
def test_values_against_float64(P, filtered, selected):
    """All six terms and both gradients, on every row, within the bars of gaussian_reg_cases.bars; the test prints the margins
    (largest error over bar; profiles/gaussian_reg/NOTES.md has their maximum).  Rows that are not selected are exact zeros."""
    c = G.make_case(P, filtered, selected)
    res = _run(c)
    assert all(torch.isfinite(t).all() for t in res)
    ref = G.reference(P, filtered, selected)
    assert res[3].item() == ref[3].item() == float(c["sel"].sum())
    off = ~c["sel"]
    assert res[1][off].abs().sum().item() == 0.0 and res[2][off].abs().sum().item() == 0.0
    m = G.margins(P, filtered, selected, res)
    print("\nP=%d %s %s: margins %s" % (P, "filtered" if filtered else "plain", "mask" if selected else "all",
                                       "  ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, m))))
    assert all(v <= 1.0 for v in m), m                        # (a NaN fails)


# ---------------------------------------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("filtered,selected", G.COMBOS, ids=COMBO_IDS)
def test_two_runs_and_two_placements_give_the_same_bits(filtered, selected):
    """No atomics: a second run is torch.equal; tensors 4 bytes off a 16-byte boundary (the mask: 1 byte) give the aligned run's bits."""
    c = G.make_case(LARGE, filtered, selected)
    first = _run(c)
    _same(first, _run(c), "second run")
    _same(first, _run(c, offset=True), "offset placement")


@pytest.mark.parametrize("filtered,selected", G.COMBOS, ids=COMBO_IDS)
def test_a_subset_of_terms_is_the_full_call_in_those_entries(filtered, selected):
    c = G.make_case(MID, filtered, selected)
    full = _run(c)
    for names in (("opacity", "scale"), ("flat",), ("aniso", "big"), ("entropy",), ("scale", "entropy", "flat")):
        ks = [REG_TERMS.index(n) for n in names]
        one_hot = torch.zeros(6)
        one_hot[ks] = c["cot"][ks]
        sub = _run(c, terms=names)                            # the case's six cotangents: those of unnamed terms must not be seen
        want = _run(c, cot=one_hot)                           # the full call with the cotangents of the other terms zero
        for k in range(6):
            assert sub[0][k].item() == (full[0][k].item() if k in ks else 0.0), (names, k)
        assert torch.equal(sub[1], want[1]) and torch.equal(sub[2], want[2]) and torch.equal(sub[3], full[3]), names
    none = _run(c, terms=())
    assert none[0].abs().sum().item() == 0.0 and none[1].abs().sum().item() == 0.0 and none[2].abs().sum().item() == 0.0
    assert torch.equal(none[3], full[3])


def _c_calls(c, want_o, want_s, offset=False):
    """bags_gaussian_reg_forward and _backward themselves, with a real NULL for what is not wanted, into buffers pre-filled with NaN
    and with a workspace of 0xFF bytes."""
    x, r, f, sel = _inputs(c, offset)
    P = c["P"]
    args = L.BagsGaussianReg(P, 63, G.MAX_RATIO, G.MAX_SCALE, L.ptr(x), L.ptr(r), L.ptr(f), L.ptr(sel))
    terms, count = torch.full((6,), float("nan"), device=DEV), torch.full((), float("nan"), device=DEV)
    stats = torch.full((L.GAUSSIAN_REG_STATS,), float("nan"), dtype=F64, device=DEV)
    ws = L.workspace(L.load().bags_gaussian_reg_workspace_size(P), DEV)
    ws.fill_(255)                                            # NaN bit patterns: every record that is read was written
    L.call("bags_gaussian_reg_forward", DEV, C.byref(args), L.ptr(ws), ws.numel(), L.ptr(terms), L.ptr(count), L.ptr(stats))
    g_x = _place(torch.full((P, 1), float("nan")), offset) if want_o else None
    g_r = _place(torch.full((P, 3), float("nan")), offset) if want_s else None
    g = c["cot"].to(DEV)
    L.call("bags_gaussian_reg_backward", DEV, C.byref(args), L.ptr(stats), L.ptr(g), L.ptr(g_x), L.ptr(g_r))
    torch.cuda.synchronize()
    return terms.cpu(), None if g_x is None else g_x.cpu(), None if g_r is None else g_r.cpu(), count.cpu(), stats.cpu()


@pytest.mark.parametrize("filtered,selected", G.COMBOS, ids=COMBO_IDS)
def test_one_gradient_alone_through_the_c_entry(filtered, selected):
    c = G.make_case(LARGE, filtered, selected)
    both = _c_calls(c, True, True)
    _same(both[:4], _run(c), "the C entries against autograd")          # 0xFF workspace, NaN outputs: nothing of them is seen
    stats = both[4]
    assert torch.isfinite(stats).all() and stats[6].item() == float(c["sel"].sum()) and stats[7].item() == 0.0
    n = stats[6].item()
    want = torch.stack([stats[0] / n, stats[1] / (3 * n), stats[2] / n, stats[3] / n, stats[4] / (3 * n), stats[5] / n])
    assert ((both[0].double() - want).abs() <= G.EPS32 * want.abs()).all()                # the terms are the raw sums, rounded once
    only_o, only_s = _c_calls(c, True, False), _c_calls(c, False, True, offset=True)
    assert only_o[2] is None and torch.equal(only_o[1], both[1]) and torch.equal(only_o[0], both[0])
    assert only_s[1] is None and torch.equal(only_s[2], both[2]) and torch.equal(only_s[4], both[4])


# ---------------------------------------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("filtered", (False, True))
def test_no_rows_and_nothing_selected(filtered):
    c = G.make_case(257, filtered, True)
    x, r, f, _ = _inputs(c)
    cases = ((x[:0], r[:0], None if f is None else f[:0], None), (x[:0], r[:0], None if f is None else f[:0], torch.zeros(0, dtype=torch.bool, device=DEV)),
             (x, r, f, torch.zeros(257, dtype=torch.bool, device=DEV)))
    for xe, re_, fe, se in cases:
        xe, re_ = xe.clone().requires_grad_(True), re_.clone().requires_grad_(True)
        terms, count = gaussian_reg_loss(xe, re_, fe, se, REG_TERMS, G.MAX_RATIO, G.MAX_SCALE)
        g_x, g_r = torch.autograd.grad(terms, [xe, re_], c["cot"].to(DEV))
        assert count.item() == 0.0 and terms.abs().sum().item() == 0.0                    # (a NaN is not 0)
        assert g_x.shape == xe.shape and g_r.shape == re_.shape
        assert g_x.abs().sum().item() == 0.0 and g_r.abs().sum().item() == 0.0


@pytest.mark.parametrize("filtered", (False, True))
def test_saturated_rows_are_finite_and_have_no_entropy(filtered):
    """The planted logits +40 and -110: finite gradients everywhere; unfiltered, o is 1 / 0 in float32, so the rows have no entropy
    and get no gradient from it (with a filter, o = c < 1 at +40 and the row is an ordinary one)."""
    c = G.make_case(65, filtered, False)
    hi, lo = G.PLANTED["logit_high"], G.PLANTED["logit_low"]
    one_hot = torch.zeros(6)
    one_hot[5] = 1.0
    res = _run(c, terms=("entropy",), cot=one_hot)
    assert all(torch.isfinite(t).all() for t in res)
    assert res[1][lo].item() == 0.0 and res[2][lo].abs().sum().item() == 0.0
    if not filtered:
        assert res[1][hi].item() == 0.0 and res[2].abs().sum().item() == 0.0
        rest = [i for i in range(65) if i not in (hi, lo)]
        x, r, _, _ = _inputs(c)
        only = gaussian_reg_loss(x[rest], r[rest], None, None, ("entropy",))[0]
        assert abs(only[5].item() * 63 - res[0][5].item() * 65) <= 4 * G.EPS32 * 65       # the two rows add nothing to the sum
    full = _run(c)
    assert all(torch.isfinite(t).all() for t in full)


# ---------------------------------------------------------------------------------------------------------------- the bag
def _bag(P=300):
    scene, _ = make_scene(P, 64, 48, 1.0, 1, seed=5)
    return GaussianBag.from_activated(scene, 1, device=DEV)


def test_the_bag_method_is_the_function():
    bag = _bag()
    sel = (torch.arange(300, device=DEV) % 3) != 0
    for filtered in (False, True):
        if filtered:
            view, _, intr, _ = look_at_origin_camera(64, 48, device=DEV).get_matrices(None, None)
            bag.compute_3D_filter(view.detach()[None], intr.detach()[None], torch.tensor([[64, 48]]))
        f = bag.filter_3D
        assert (f is not None) == filtered
        for s in (None, sel):
            got = bag.regularizers(s, max_ratio=3.0, max_scale=0.02)
            want = gaussian_reg_loss(bag._opacity, bag._scaling, f, s, REG_TERMS, 3.0, 0.02)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].grad_fn is not None
            lam = torch.tensor([0.01, 0.01, 1.0, 0.5, 0.25, 0.1], device=DEV)
            ga = torch.autograd.grad(got[0] @ lam, [bag._opacity, bag._scaling])
            gb = torch.autograd.grad(want[0] @ lam, [bag._opacity, bag._scaling])
            assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1]) and ga[1].abs().sum().item() > 0
    assert (got[0][:3] > 0).all()
    bag.filter_3D = bag.filter_3D[:-1]
    with pytest.raises(RuntimeError, match="GaussianBag.regularizers.*stale"):
        bag.regularizers()


def test_chain_render_plus_regularizers_then_adam():
    """terms @ lambdas added to a tiny render() loss, one backward, one GaussianAdam step: the .grad of _opacity / _scaling is the sum of
    the two parts computed separately, within one float32 rounding of the sum."""
    lam = torch.tensor([0.01, 0.01, 100.0, 0.1, 10.0, 0.05], device=DEV)
    g_img = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    bg = torch.zeros(3, device=DEV)
    cam = look_at_origin_camera(64, 48, device=DEV)

    def route(kind):
        bag = _bag()
        view, _, intr, _ = cam.get_matrices(None, None)
        bag.compute_3D_filter(view.detach()[None], intr.detach()[None], torch.tensor([[64, 48]]))
        loss = 0.0
        if kind in ("both", "render"):
            res = render(cam, bag, PipelineParams(), bg, 0.0, None)
            loss = loss + (res["render"] * g_img).sum() / g_img.numel()
        if kind in ("both", "reg"):
            terms, count = bag.regularizers(max_ratio=3.0, max_scale=0.02)
            assert count.item() == 300
            loss = loss + terms @ lam
        loss.backward()
        torch.cuda.synchronize()
        return bag

    both, img, reg = route("both"), route("render"), route("reg")
    for name in ("_opacity", "_scaling"):
        a, b, got = getattr(img, name).grad.double(), getattr(reg, name).grad.double(), getattr(both, name).grad.double()
        assert b.abs().sum().item() > 0 and a.abs().sum().item() > 0
        assert ((got - (a + b)).abs() <= G.EPS32 * (a + b).abs()).all(), name
    leaves = {"opacity": both._opacity, "scaling": both._scaling}
    before = {k: v.detach().clone() for k, v in leaves.items()}
    opt = GaussianAdam([{"params": [v], "lr": 1e-3, "name": k} for k, v in leaves.items()], lr=0.0, eps=1e-15)
    opt.step()
    torch.cuda.synchronize()
    for k, v in leaves.items():
        moved = (v.detach() != before[k])
        assert torch.isfinite(v).all() and moved.any() and torch.equal(moved, v.grad != 0), k
