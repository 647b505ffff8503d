"""No-GPU checks of antialiased rendering (csrc/antialias.hip, bags_raster/antialias.py): the PyTorch statement against the closed
form and against finite differences, the named cases of tests/antialias_cases.py against what they claim to contain, the C ABI
surface with its argument validation (reported before anything is enqueued), and the settings fields."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import antialias_cases as A
import bags_raster
from bags_raster import GaussianRasterizationSettings, GaussianRasterizer, PipelineParams, _lib
from scenes import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_antialias_forward", "bags_antialias_workspace_size", "bags_antialias_backward")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. closed form
def _on_axis(s, z, dtype=torch.float64):
    """Isotropic Gaussians of scale s[i] on the optical axis at depth z[i] under the identity view and fx = fy = 64."""
    n = len(s)
    eye = torch.eye(4, dtype=dtype)
    k = torch.zeros(4, 4, dtype=dtype)
    k[0, 0] = k[1, 1] = 2.0                                                    # fx = k[0] * W / 2 = 64 = fy
    means = torch.zeros(n, 3, dtype=dtype)
    means[:, 2] = torch.as_tensor(z, dtype=dtype)
    scales = torch.as_tensor(s, dtype=dtype).reshape(n, 1).expand(n, 3).contiguous()
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=dtype).expand(n, 4).contiguous()
    return bags_raster.antialias_opacity_torch(means, torch.ones(n, 1, dtype=dtype), eye, k, (64, 64), (0.5, 0.5), scales=scales, rotations=rot)


def test_closed_form_on_the_optical_axis():
    """u = (fx s / z)^2 on both axes and no cross term: h = sqrt(u^2 / (u + 0.3)^2) = u / (u + 0.3)."""
    s = [0.001 * 1.35 ** i for i in range(24)]                                 # 0.001 .. 1.0: h from 0.0135 to 0.9999
    z = [1.0 + 0.37 * (i % 5) for i in range(24)]
    out = _on_axis(s, z)
    u = torch.tensor([(64.0 * a / b) ** 2 for a, b in zip(s, z)], dtype=torch.float64)
    want = u / (u + 0.3)
    assert want.min().item() > 0.005 and want.max().item() > 0.999
    assert (out[:, 0] - want).abs().max().item() <= 1e-12
    # below the floor (u / (u + 0.3) < 0.005 from u < 0.0015, s < 6.1e-4 at z = 1): exactly upstream's 0.005
    low = _on_axis([1e-6, 1e-4, 5e-4], [1.0, 1.0, 1.0])
    assert math.sqrt(A.FLOOR) == 0.005 and torch.equal(low, torch.full((3, 1), 0.005, dtype=torch.float64))
    # at and behind the near plane (view depth <= 0.2) the opacity is left alone
    near = _on_axis([0.01, 0.01, 0.01, 0.01], [0.2, 0.1, 0.0, -3.0])
    assert torch.equal(near, torch.ones(4, 1, dtype=torch.float64))
    assert _on_axis([0.01], [0.2000001]).item() < 1.0
    # float32 on the CPU: the same values to fp32 rounding of the chain
    out32 = _on_axis(s, z, torch.float32)
    assert out32.dtype == torch.float32 and (out32[:, 0].double() - want).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2. gradcheck
def _rows(name, want_clamped):
    """Seven rows of a case in front of the near plane: with clamped ones among them, or none."""
    c = A.case(name)
    d = A._decisions(name, torch.float64, A.P_FULL, False, 1.0)
    live = ~d["culled"] & ~d["floor"]
    pick = (live & d["clamped"]).nonzero()[:3, 0].tolist() + (live & ~d["clamped"]).nonzero()[:4, 0].tolist() if want_clamped \
        else (live & ~d["clamped"]).nonzero()[:7, 0].tolist()
    assert len(pick) == 7
    return c, torch.tensor(pick)


@pytest.mark.parametrize("cov", (False, True), ids=("scales_rotations", "cov3D_precomp"))
@pytest.mark.parametrize("clamp_grad", ("stock", "exact"))
def test_gradcheck_of_the_float64_statement(clamp_grad, cov):
    """Finite differences against autograd for every input, on seven rows of `inside_shift` (non-zero shift_factors, camera inside
    the cloud).  "exact" is the derivative of the function, so three of its rows sit on the field-of-view clamp.  "stock" holds a
    clamped t.x constant, which on a clamped row is by design NOT the derivative of the forward; its rows are unclamped ones, where
    the two modes are the same function and the same graph but for the `where` that selects the detached value."""
    c, rows = _rows("inside_shift", want_clamped=clamp_grad == "exact")
    dd = lambda t: t.double().clone().requires_grad_(True)                     # noqa: E731
    means, opac, view, intr, sf = (dd(c[n][rows]) if n in ("means3D", "opacities") else dd(c[n]) for n in ("means3D", "opacities", "viewmatrix",
                                                                                                              "intrinsic", "shift_factors"))
    scales, rot = c["scales"][rows].double(), c["rotations"][rows].double()
    if cov:
        src = (dd(A.covariance_from_scaling_rotation(scales, 1.7, rot)),)
        fn = lambda m, o, v, k, s_, cv: bags_raster.antialias_opacity_torch(m, o, v, k, c["image_hw"], c["tanfov"], cov3D_precomp=cv,      # noqa: E731
                                                                           shift_factors=s_, clamp_grad=clamp_grad)
    else:
        src = (dd(scales), dd(rot))
        fn = lambda m, o, v, k, s_, sc, q: bags_raster.antialias_opacity_torch(m, o, v, k, c["image_hw"], c["tanfov"], scales=sc,        # noqa: E731
                                                                              rotations=q, shift_factors=s_, scale_modifier=1.7,
                                                                              clamp_grad=clamp_grad)
    assert torch.autograd.gradcheck(fn, (means, opac, view, intr, sf) + src, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_dead_rows_give_the_opacity_gradient_and_nothing_else():
    """A culled row and a row on the floor: dL/dopacity = g h, zeros everywhere else, no NaN in the pose sums."""
    z = [1.0, 0.1, 1.0]                                                        # floor, culled, live (anisotropic and turned)
    eye = torch.eye(4, dtype=torch.float64).requires_grad_(True)
    k = torch.zeros(4, 4, dtype=torch.float64)
    k[0, 0] = k[1, 1] = 2.0
    k.requires_grad_(True)
    means = torch.tensor([[0.1, 0.0, z[0]], [0.0, 0.1, z[1]], [0.1, 0.1, z[2]]], dtype=torch.float64, requires_grad=True)
    scales = torch.tensor([[1e-5, 1e-5, 1e-5], [0.01, 0.01, 0.01], [0.01, 0.02, 0.03]], dtype=torch.float64, requires_grad=True)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.8, 0.2, -0.4, 0.4]], dtype=torch.float64, requires_grad=True)
    opac = torch.full((3, 1), 0.5, dtype=torch.float64, requires_grad=True)
    out = bags_raster.antialias_opacity_torch(means, opac, eye, k, (64, 64), (0.5, 0.5), scales=scales, rotations=rot)
    only_live = bags_raster.antialias_opacity_torch(means[2:], opac[2:], eye, k, (64, 64), (0.5, 0.5), scales=scales[2:], rotations=rot[2:])
    g_all = torch.autograd.grad(out.sum(), (means, scales, rot, opac, eye, k))
    g_live = torch.autograd.grad(only_live.sum(), (eye, k))
    assert torch.equal(out[:2, 0].detach(), torch.tensor([0.5 * 0.005, 0.5], dtype=torch.float64))
    for g in g_all[:3]:
        assert torch.isfinite(g).all() and g[:2].abs().max().item() == 0.0 and g[2].abs().max().item() > 0.0
    assert torch.equal(g_all[3][:, 0], torch.tensor([0.005, 1.0, out[2, 0].item() / 0.5], dtype=torch.float64))
    assert torch.equal(g_all[4], g_live[0]) and torch.equal(g_all[5], g_live[1])


# ---------------------------------------------------------------------------------------------------------------- 3. the cases
#                 floor culled clamped   (about half of what the float64 statement counts: antialias_cases.counts)
HALF = {"generic":      (0,   0,   1),
        "subpixel":     (271, 0,   0),
        "inside":       (0,   98,  271),
        "inside_shift": (0,   98,  270),
        "needles":      (15,  0,   0)}


@pytest.mark.parametrize("name", tuple(A.CASES))
def test_cases_contain_what_they_claim(name):
    n = A.counts(name)
    print(name, n)
    floor, culled, clamped = HALF.get(name, (0, 0, 0))
    assert n["floor"] >= floor and n["culled"] >= culled and n["clamped"] >= clamped, n
    if name != "needles":
        assert n["flips"] == 0, n
    else:
        assert 1 <= n["flips"] <= A.P_FULL // 100, n                          # the rows the GPU test leaves out: at most 1 %
    if name in ("generic", "small", "inside", "inside_shift"):
        assert n["floor"] == 0, n
    if name == "small":                                                        # minified, but nowhere near the floor
        assert 0.05 <= n["h_min"] and n["h_max"] <= 0.9, n
    if name == "flat":                                                         # d0 cancels: fp32 loses h at the 1e-4 level
        assert n["h_err"] >= 4.8e-5, n
    if name == "needles":
        assert n["h_err"] >= 7.5e-4, n


@pytest.mark.parametrize("name", A.WELL)
def test_float32_statement_is_within_the_gradient_bar_where_the_kernel_is_held_to_it(name):
    """The GPU tests hold the kernel to 1e-4 against float64 on the well-conditioned cases: float32 arithmetic must be able to.
    Asserted on the per-Gaussian tensors; the pose sums are printed only -- this statement adds them in float32 in whatever order
    torch sums in and differentiates the atan polynomial, neither of which the kernel does (inside: shift_factors 1.1e-4)."""
    o64, g64 = A.reference(name, torch.float64)
    o32, g32 = A.reference(name, torch.float32)
    assert ((o32.double() - o64).abs() <= 1e-5 * (1 + o64.abs())).all()
    errs = {n: rel_err(g32[n], g64[n]) for n in g64}
    print(name, errs)
    assert all(torch.isfinite(g).all() for g in g64.values()), errs
    assert max(errs[n] for n in ("means3D", "opacities", "scales", "rotations")) <= 1e-4, errs
    assert all(g64[n].abs().max().item() > 0 for n in g64), "every argument's gradient is exercised"
    assert ("shift_factors" in g64) == (name == "inside_shift")


def test_sizes_are_either_side_of_a_workgroup():
    src = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "antialias.hip")).read()
    assert "#define AA_BLOCK %d" % A.BLOCK in src and A.SIZES == (1, 255, 257, 1025)


# ---------------------------------------------------------------------------------------------------------------- 4. the C ABI
def _header_struct_fields(name):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [part.strip().split()[-1].lstrip("*") for part in decl.split(",")]
    return fields


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in FUNCS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert [f[0] for f in _lib.BagsAntialias._fields_] == _header_struct_fields("BagsAntialias")
    assert C.sizeof(_lib.BagsAntialias) == 8 * 4 + 8 * 8 and _lib.BagsAntialias.means3D.offset == 32
    assert _lib.SYMBOLS["bags_antialias_forward"][1][-1] is C.c_void_p and _lib.SYMBOLS["bags_antialias_backward"][1][-1] is C.c_void_p
    sizes = [lib.bags_antialias_workspace_size(P) for P in (0, 1, 256, 257, 1025, 100_000, 500_000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[1] < sizes[-2] < sizes[-1]
    assert sizes[-1] >= (500_000 + 255) // 256 * 17 * 4
    assert callable(bags_raster.antialias_opacity) and callable(bags_raster.antialias_opacity_torch)
    assert "antialias_opacity" in bags_raster.__all__ and "antialias_opacity_torch" in bags_raster.__all__


def test_argument_validation(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 15) & ~15
    big = 1 << 40

    def refused(rc, text, code=-1):
        msg = lib.bags_last_error()
        assert rc == code and text in msg, (rc, msg)

    def args(P=10, W=64, H=48, clamp=0, cov=False, **edit):
        a = _lib.BagsAntialias(P, W, H, clamp, 0.5, 0.4, 1.0, 0, addr, None if cov else addr, None if cov else addr, addr if cov else None,
                               addr, None, addr, addr)
        for n, v in edit.items():
            setattr(a, n, v)
        return a
    ref = lambda a: None if a is None else C.byref(a)                                                                 # noqa: E731
    fwd = lambda a, out=addr: lib.bags_antialias_forward(ref(a), out, None)                                          # noqa: E731

    def bwd(a, grad_out=addr, ws=addr, ws_bytes=big, outs=None):
        o = dict(g_opacities=addr, g_means3D=addr, g_scales=addr, g_rotations=addr, g_cov3D=None, g_viewmatrix=addr, g_intrinsic=addr, g_shift=addr)
        o.update(outs or {})
        return lib.bags_antialias_backward(ref(a), grad_out, ws, ws_bytes, *o.values(), None)
    for fn, op in ((fwd, b"antialias_forward"), (bwd, b"antialias_backward")):
        assert fn(None) == -1 and op + b": null struct" in lib.bags_last_error()
        refused(fn(args(P=-1)), op + b": P < 0")
        refused(fn(args(W=0)), op + b": empty image")
        refused(fn(args(clamp=2)), op + b": clamp_grad 2")
        refused(fn(args(cov3D_precomp=addr)), op + b": provide exactly one of either scale/rotation pair or precomputed 3D covariance")      # both
        refused(fn(args(scales=None, rotations=None)), op + b": provide exactly one")                                                        # neither
        refused(fn(args(rotations=None)), op + b": provide exactly one")                                                                     # half a pair
        refused(fn(args(cov=True, rotations=addr)), op + b": provide exactly one")
        refused(fn(args(means3D=None)), op + b": NULL means3D / opacities")
        refused(fn(args(opacities=None)), op + b": NULL means3D / opacities")
        refused(fn(args(viewmatrix=None)), op + b": NULL viewmatrix / intrinsic")
        refused(fn(args(intrinsic=None)), op + b": NULL viewmatrix / intrinsic")
    refused(fwd(args(), out=None), b"antialias_forward: NULL out")
    refused(bwd(args(), grad_out=None), b"antialias_backward: NULL grad_out")
    refused(bwd(args(), ws_bytes=16), b"pose gradients need a workspace", code=-3)
    refused(bwd(args(), ws=None), b"pose gradients need a workspace", code=-3)
    refused(bwd(args(), ws_bytes=lib.bags_antialias_workspace_size(10) - 1), b"pose gradients need a workspace", code=-3)
    refused(bwd(args(), outs=dict(g_cov3D=addr)), b"covariance source that was not given")
    refused(bwd(args(cov=True)), b"covariance source that was not given")                      # g_scales / g_rotations with cov3D_precomp
    # nothing to do: no device is touched
    empty = _lib.BagsAntialias(0, 64, 48, 0, 0.5, 0.4, 1.0, 0, *([None] * 8))
    assert fwd(empty, out=None) == 0
    assert lib.bags_antialias_backward(C.byref(empty), None, None, 0, *([None] * 8), None) == 0
    none = dict(g_opacities=None, g_means3D=None, g_scales=None, g_rotations=None, g_viewmatrix=None, g_intrinsic=None, g_shift=None)
    assert bwd(args(), ws=None, ws_bytes=0, outs=none) == 0                                     # no output wanted


# ---------------------------------------------------------------------------------------------------------------- 5. settings
def _settings(**kw):
    eye = torch.eye(4)
    return GaussianRasterizationSettings(32, 32, 0.5, 0.5, torch.zeros(3), 1.0, eye, eye, eye, 0, torch.zeros(3), False, False, 0, **kw)


def test_settings_and_pipeline_fields():
    assert _settings(antialiasing=True).antialiasing is True and _settings().antialiasing is False
    assert GaussianRasterizationSettings._field_defaults["antialiasing"] is False
    assert GaussianRasterizationSettings._fields[:14] == _settings()._fields[:14] and "antialiasing" in GaussianRasterizationSettings._fields[14:]
    assert PipelineParams().antialiasing is False and PipelineParams(antialiasing=True).antialiasing is True
    assert "antialiasing" not in [f[0] for f in _lib.BagsSettings._fields_]                     # it never reaches the C struct
    x = torch.rand(5, 3)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="antialiasing must be True or False"):              # before anything looks at a device
            GaussianRasterizer(_settings(antialiasing=bad))(means3D=x, means2D=None, opacities=torch.rand(5, 1), colors_precomp=x,
                                                            scales=x, rotations=torch.rand(5, 4))
        with pytest.raises(ValueError, match="antialiasing must be True or False"):
            bags_raster.debug_views(_settings(antialiasing=bad), x, None, None, None, x, torch.rand(5, 1), x, torch.rand(5, 4), None)


def test_host_tensors_are_sent_to_the_twin():
    lv = {n: t.detach() for n, t in A.leaves("generic", torch.float32, P=5).items()}
    with pytest.raises(NotImplementedError, match="antialias_opacity runs only on an AMD GPU.*antialias_opacity_torch"):
        A.run(bags_raster.antialias_opacity, "generic", lv)
    for kw in (dict(scales=None, rotations=None), dict(cov3D_precomp=torch.rand(5, 6))):
        c = A.case("generic")
        a = dict(scales=lv["scales"], rotations=lv["rotations"], cov3D_precomp=None)
        a.update(kw)
        with pytest.raises(ValueError, match="antialias_opacity_torch: provide exactly one"):
            bags_raster.antialias_opacity_torch(lv["means3D"], lv["opacities"], lv["viewmatrix"], lv["intrinsic"], c["image_hw"], c["tanfov"], **a)
    if not torch.cuda.is_available():                         # (with a GPU the settings route runs: tests/test_antialias_gpu.py)
        with pytest.raises(NotImplementedError, match="antialias_opacity runs only on an AMD GPU"):
            x = torch.rand(5, 3)
            GaussianRasterizer(_settings(antialiasing=True))(means3D=x, means2D=None, opacities=torch.rand(5, 1), colors_precomp=x,
                                                             scales=x, rotations=torch.rand(5, 4))
