"""No-GPU checks of the regularisers on the Gaussians (bags_raster.gaussian_reg_loss, csrc/gaussian_reg.hip): the PyTorch statement
in float64 against the closed forms written out by hand and against the published 3DGS-MCMC lines, what the bars of
tests/gaussian_reg_cases.py reject, the generator's guarantees on every case the GPU tests use, the C ABI (header, bound symbols,
struct layout, every rejection that needs no device) and the Python argument errors."""
import ctypes as C
import os
import re

import pytest
import torch

import bags_raster
import gaussian_reg_cases as G
from bags_raster import REG_TERMS, _lib, gaussian_reg_loss, gaussian_reg_loss_torch
from bags_raster.gaussians import GaussianBag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_gaussian_reg_workspace_size", "bags_gaussian_reg_forward", "bags_gaussian_reg_backward")
F64 = torch.float64
ALL = [(P, f, s) for P in G.SIZES for f, s in G.COMBOS]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("P", (1, 65, G.ROWS_PER_GROUP + 1))
@pytest.mark.parametrize("filtered,selected", G.COMBOS)
def test_statement_equals_the_closed_forms(P, filtered, selected):
    """gaussian_reg_loss_torch in float64 with autograd against the six sums and their gradients written out by hand, the
    through_c term of the filtered opacity included."""
    c = G.make_case(P, filtered, selected)
    ref, cf = G.reference(P, filtered, selected), G.closed_form(c)
    for name, a, b in zip(("terms", "dL/d_opacity", "dL/d_scaling"), cf, ref[:3]):
        assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-12 * (1 + b.abs().max().item()), name
    assert ref[3].item() == float(c["sel"].sum()) == c["figures"]["n"]
    unselected = ~c["sel"]
    assert ref[1][unselected].abs().sum().item() == 0.0 and ref[2][unselected].abs().sum().item() == 0.0
    if filtered and P > 1:                                   # the opacity terms reach _scaling: dropping through_c is seen
        assert (G.closed_form(c, drop_through_c=True)[2] - ref[2]).abs().max().item() > 1e-6 / P


def test_indices_0_and_1_are_the_mcmc_lines():
    """3DGS-MCMC's train.py: ``args.opacity_reg * torch.abs(gaussians.get_opacity).mean()`` and ``args.scale_reg *
    torch.abs(gaussians.get_scaling).mean()``, on the bag's properties, with and without a 3D filter."""
    c = G.make_case(257, True, False)
    bag = GaussianBag(0)
    bag._xyz = torch.zeros(257, 3, dtype=F64)
    bag._opacity, bag._scaling = c["opacity"].double().requires_grad_(True), c["scaling"].double().requires_grad_(True)
    terms, count = bag.regularizers(terms=("opacity", "scale"))
    assert count.item() == 257 and terms[2:].abs().sum().item() == 0.0
    assert abs(terms[0].item() - torch.abs(bag.get_opacity).mean().item()) <= 1e-14
    assert abs(terms[1].item() - torch.abs(bag.get_scaling).mean().item()) <= 1e-14
    bag.filter_3D = c["filter"].double()
    terms, _ = bag.regularizers()
    assert abs(terms[0].item() - torch.abs(bag.get_opacity_with_3D_filter).mean().item()) <= 1e-14
    assert abs(terms[1].item() - torch.abs(bag.get_scaling_with_3D_filter).mean().item()) <= 1e-14
    assert torch.equal(terms, gaussian_reg_loss_torch(bag._opacity, bag._scaling, bag.filter_3D)[0])
    bag.filter_3D = bag.filter_3D[:-1]
    with pytest.raises(RuntimeError, match="GaussianBag.regularizers.*stale"):
        bag.regularizers()


def test_subset_hinges_and_degenerate_inputs():
    c = G.make_case(65, True, True)
    x, r, f, sel = c["opacity"].double(), c["scaling"].double(), c["filter"].double(), c["sel"]
    full = gaussian_reg_loss_torch(x, r, f, sel, REG_TERMS, G.MAX_RATIO, G.MAX_SCALE)[0]
    for k, name in enumerate(REG_TERMS):
        one = gaussian_reg_loss_torch(x, r, f, sel, (name,), G.MAX_RATIO, G.MAX_SCALE)[0]
        assert one[k].item() == full[k].item() and one.abs().sum().item() == abs(full[k].item()), name
    # a strict hinge: exactly at the threshold the value and the gradient are zero
    r1 = torch.log(torch.tensor([[0.25, 0.5, 1.0]], dtype=F64)).requires_grad_(True)
    x1 = torch.zeros(1, 1, dtype=F64, requires_grad=True)
    terms, _ = gaussian_reg_loss_torch(x1, r1, None, None, ("aniso", "big"), 4.0, 1.0)
    assert terms[3].item() == 0.0 and terms[4].item() == 0.0
    terms.sum().backward()
    assert r1.grad.abs().sum().item() == 0.0
    # the planted saturated logits: no entropy, finite gradients
    x2 = torch.tensor([[40.0], [-110.0]], requires_grad=True)
    r2 = torch.zeros(2, 3, requires_grad=True)
    terms, _ = gaussian_reg_loss_torch(x2, r2, None, None, ("entropy",))
    terms[5].backward()
    assert terms[5].item() == 0.0 and torch.isfinite(x2.grad).all() and x2.grad.abs().sum().item() == 0.0
    # n == 0: no rows, nothing selected
    for xe, re_, se in ((x[:0], r[:0], None), (x, r, torch.zeros(65, dtype=torch.bool))):
        xe, re_ = xe.clone().requires_grad_(True), re_.clone().requires_grad_(True)
        terms, count = gaussian_reg_loss_torch(xe, re_, None if se is None else f, se)
        assert count.item() == 0 and terms.abs().sum().item() == 0.0
        terms.sum().backward()
        assert xe.grad.abs().sum().item() == 0.0 and re_.grad.abs().sum().item() == 0.0 and torch.isfinite(re_.grad).all()


# ---------------------------------------------------------------------------------------------------------------- cases and bars
@pytest.mark.parametrize("P,filtered,selected", ALL)
def test_check_case_holds_on_every_gpu_case(P, filtered, selected):
    c = G.make_case(P, filtered, selected)
    fig = G.check_case(c)
    assert fig == c["figures"] and fig["gap_ratio"] > G.NEAR and fig["gap_scale"] > G.NEAR
    assert c["opacity"].dtype == c["scaling"].dtype == torch.float32 and c["sel"].dtype == torch.bool
    logits = c["opacity"][~c["planted"]]
    assert logits.numel() == 0 or (logits.abs().max().item() <= 8.0)
    assert (c["cot"] > 0).any() and (c["cot"] < 0).any()
    if P >= 8:
        r = c["scaling"]
        k = G.PLANTED
        assert r[k["tie_min"], 0] == r[k["tie_min"], 1] < r[k["tie_min"], 2] and r[k["tie_max"], 0] < r[k["tie_max"], 1] == r[k["tie_max"], 2]
        assert r[k["tie_all"], 0] == r[k["tie_all"], 1] == r[k["tie_all"], 2]
        assert c["opacity"][k["logit_high"]].item() == 40.0 and c["opacity"][k["logit_low"]].item() == -110.0
        assert torch.sigmoid(c["opacity"])[k["logit_high"]].item() == 1.0 and torch.sigmoid(c["opacity"])[k["logit_low"]].item() == 0.0
        assert c["sel"][c["planted"]].all() and (not selected or not c["sel"].all())
        if filtered:
            assert c["filter"][k["big_filter"]].item() > 100 * torch.exp(r[k["big_filter"]]).max().item()
    others = c["filter"][~c["planted"]]
    assert others.numel() == 0 or (0.0009 <= others.min().item() and others.max().item() <= 0.0501)


def test_sizes_come_from_the_kernel_constants():
    R = G.ROWS_PER_GROUP
    assert R == _lib.GAUSSIAN_REG_ROWS and R % _lib.GAUSSIAN_REG_BLOCK == 0
    assert {1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 17} == set(G.SIZES)


def test_bars_reject_three_wrong_answers():
    """The through_c term dropped, n in place of 3n, argmax taken for flat: each is far outside the bars, the closed form inside."""
    for P in (257, G.ROWS_PER_GROUP + 1):
        c = G.make_case(P, True, True)
        assert max(G.margins(P, True, True, G.closed_form(c))) <= 0.26
        m = G.margins(P, True, True, G.closed_form(c, drop_through_c=True))
        assert m[2] > 100 and m[0] <= 0.26 and m[1] <= 0.26, m
        m = G.margins(P, True, True, G.closed_form(c, n_not_3n=True))
        assert m[0] > 100 and m[2] > 100, m
        m = G.margins(P, True, True, G.closed_form(c, flat_argmax=True))
        assert m[0] > 100 and m[2] > 100, m
    bar = G.bars(257, True, True)
    c = G.make_case(257, True, True)
    assert bar[1][~c["sel"]].abs().sum().item() == 0.0 and bar[2][~c["sel"]].abs().sum().item() == 0.0       # exact zeros there
    live = c["sel"].clone()
    live[G.PLANTED["logit_high"]] = False                    # sigmoid(40) is 1 in float64 too: no slope, the bar of dL/d_opacity is 0 there
    assert bar[1][G.PLANTED["logit_high"]].item() == 0.0
    assert (bar[1][live] > 0).all() and float(bar[1].max()) < 1e-6                                            # of order eps / n


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _header_struct_fields(name):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*?\]", "", part).strip().split()[-1].lstrip("*") for part in decl.split(",")]
    return fields


def test_symbols_struct_and_constants(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in FUNCS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, header, re.S).group(1)
        if name != "bags_gaussian_reg_workspace_size":                                   # the stream comes last
            assert decl.rstrip().endswith("void* stream") and _lib.SYMBOLS[name][1][-1] is C.c_void_p, name
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert [f[0] for f in _lib.BagsGaussianReg._fields_] == _header_struct_fields("BagsGaussianReg") == \
        ["P", "terms", "max_ratio", "max_scale", "opacity_raw", "scaling_raw", "filter", "select"]
    B = _lib.BagsGaussianReg
    assert (B.terms.offset, B.max_ratio.offset, B.max_scale.offset, B.opacity_raw.offset, B.select.offset) == (4, 8, 12, 16, 40)
    assert C.sizeof(B) == 48
    for name, value in (("BLOCK", _lib.GAUSSIAN_REG_BLOCK), ("ROWS", _lib.GAUSSIAN_REG_ROWS), ("STATS", _lib.GAUSSIAN_REG_STATS),
                        ("TERMS", _lib.GAUSSIAN_REG_TERMS)):
        assert re.search(r"#define BAGS_GAUSSIAN_REG_%s %d\b" % (name, value), header), name
    assert len(REG_TERMS) == _lib.GAUSSIAN_REG_TERMS and REG_TERMS == ("opacity", "scale", "flat", "aniso", "big", "entropy")
    names = ("REG_TERMS", "gaussian_reg_loss", "gaussian_reg_loss_torch")
    assert set(names) <= set(bags_raster.__all__) and all(hasattr(bags_raster, n) for n in names)
    assert callable(GaussianBag.regularizers)
    makefile = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "build/gaussian_reg.o" in makefile and "EXTRA_gaussian_reg = -ffp-contract=off" in makefile


def test_workspace_size(lib):
    """One record of 8 doubles per ROWS rows, in multiples of 256 bytes; nothing for P <= 0."""
    size = lib.bags_gaussian_reg_workspace_size
    R = _lib.GAUSSIAN_REG_ROWS
    assert size(0) == 0 and size(-5) == 0
    assert size(1) == size(R) == size(4 * R) == 256 and size(4 * R + 1) == 512
    for P in (500_000, 2_000_000, 5_000_000, 2 ** 31 - 1):
        assert size(P) % 256 == 0 and -(-P // R) * 64 <= size(P) < -(-P // R) * 64 + 256


def test_every_rejection_is_reached_without_a_device(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 8192)()
    addr = (C.addressof(buf) + 255) & ~255
    P = 3000
    need = lib.bags_gaussian_reg_workspace_size(P)
    assert need == 256

    def args(**edit):
        a = _lib.BagsGaussianReg(P, 63, 10.0, 0.05, addr, addr, addr, addr)
        for n, v in edit.items():
            setattr(a, n, v)
        return a

    def fwd(a, ws=addr + 256, ws_bytes=need, terms=addr + 2048, count=addr + 2112, stats=addr + 2176):
        return lib.bags_gaussian_reg_forward(C.byref(a) if a is not None else None, ws, ws_bytes, terms, count, stats, None)

    def bwd(a, stats=addr + 2176, g_terms=addr + 2048, g_opacity=addr + 4096, g_scaling=addr + 4352):
        return lib.bags_gaussian_reg_backward(C.byref(a) if a is not None else None, stats, g_terms, g_opacity, g_scaling, None)

    def refused(rc, text, code=-1):
        msg = lib.bags_last_error().decode()
        assert rc == code and "gaussian_reg" in msg and text in msg, (rc, msg)

    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    assert "BAGS_ERR_ARG = -1" in header and "BAGS_ERR_SIZE = -3" in header
    for call in (fwd, bwd):
        refused(call(None), "null struct")
        refused(call(args(P=-1)), "P < 0 (got -1)")
        refused(call(args(terms=64)), "unknown bits in terms 0x40")
        refused(call(args(terms=0x80000001)), "unknown bits")
        refused(call(args(max_ratio=0.5)), "max_ratio must be >= 1")
        refused(call(args(max_ratio=float("nan"))), "max_ratio must be >= 1")
        refused(call(args(max_scale=-1e-3)), "max_scale must be >= 0")
        refused(call(args(max_scale=float("nan"))), "max_scale must be >= 0")
        refused(call(args(opacity_raw=None)), "null opacity_raw / scaling_raw")
        refused(call(args(scaling_raw=None)), "null opacity_raw / scaling_raw")
    refused(fwd(args(), terms=None), "null terms / count / stats")
    refused(fwd(args(), count=None), "null terms / count / stats")
    refused(fwd(args(), stats=None), "null terms / count / stats")
    refused(fwd(args(), stats=addr + 2180), "stats is not 8-byte aligned")
    refused(fwd(args(), ws=None), "needs a workspace of %d bytes (got 0)" % need, code=-3)
    refused(fwd(args(), ws_bytes=need - 1), "needs a workspace of %d bytes (got %d)" % (need, need - 1), code=-3)
    refused(fwd(args(), ws=addr + 256 + 8), "not 16-byte aligned")
    refused(bwd(args(), stats=None), "null stats")
    refused(bwd(args(), stats=addr + 2180), "stats is not 8-byte aligned")
    refused(bwd(args(), g_terms=None), "null g_terms")
    refused(bwd(args(), g_opacity=addr), "must not be its leaf")
    refused(bwd(args(), g_scaling=addr), "must not be its leaf")
    # nothing wanted, or no rows: a successful no-op that launches nothing; the filter and the mask are optional
    assert bwd(args(), g_opacity=None, g_scaling=None) == 0
    assert bwd(args(filter=None, select=None), g_opacity=None, g_scaling=None) == 0
    assert bwd(args(P=0, opacity_raw=None, scaling_raw=None)) == 0


# ---------------------------------------------------------------------------------------------------------------- the wrappers
def test_wrappers_refuse_what_they_cannot_run():
    c = G.make_case(65, True, True)
    x, r, f, sel = c["opacity"], c["scaling"], c["filter"], c["sel"]
    with pytest.raises(NotImplementedError, match="gaussian_reg_loss_torch"):
        gaussian_reg_loss(x, r, f, sel)                       # host tensors into the HIP path: refused, not copied
    for fn, op in ((gaussian_reg_loss, "gaussian_reg_loss"), (gaussian_reg_loss_torch, "gaussian_reg_loss_torch")):
        with pytest.raises(TypeError, match=op + ": opacity_raw must be a tensor"):
            fn(None, r)
        with pytest.raises(TypeError, match=op + ": scaling_raw must be a floating-point"):
            fn(x, r.long())
        with pytest.raises(ValueError, match=op + r": scaling_raw must be \(P,3\)"):
            fn(x, r[:, :2])
        with pytest.raises(ValueError, match=op + r": opacity_raw must be \(P,1\) with P = 65"):
            fn(x[:-1], r)
        with pytest.raises(TypeError, match=op + ": opacity_raw is torch.float64, scaling_raw is torch.float32"):
            fn(x.double(), r)
        with pytest.raises(ValueError, match=op + r": filter_3D must be \(P,1\)"):
            fn(x, r, f[:-1])
        with pytest.raises(TypeError, match=op + ": filter_3D must be a tensor or None"):
            fn(x, r, 0.02)
        with pytest.raises(TypeError, match=op + ": select must be a torch.bool tensor"):
            fn(x, r, f, sel.float())
        with pytest.raises(ValueError, match=op + r": select must be \(P,\)"):
            fn(x, r, f, sel[:, None])
        with pytest.raises(ValueError, match=op + ": unknown term 'flatness'"):
            fn(x, r, f, sel, ("opacity", "flatness"))
        with pytest.raises(ValueError, match=op + ": max_ratio must be >= 1"):
            fn(x, r, f, sel, REG_TERMS, 0.99)
        with pytest.raises(ValueError, match=op + ": max_ratio must be >= 1"):
            fn(x, r, f, sel, REG_TERMS, float("nan"))
        with pytest.raises(ValueError, match=op + ": max_scale must be >= 0"):
            fn(x, r, f, sel, REG_TERMS, 10.0, -0.1)
    # a single name is a subset of one; float32 on the host stays float32
    terms, count = gaussian_reg_loss_torch(x, r, f, sel, "flat")
    assert terms.dtype == torch.float32 and terms[2].item() > 0 and terms.abs().sum().item() == terms[2].item() and count.item() == int(sel.sum())
