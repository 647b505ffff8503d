"""No-GPU checks of the bilateral-grid step (bags_raster/bilagrid.py, csrc/bilagrid.hip): the PyTorch statements against the
published grid_sample / index_select formulations, the (1,1,1) grid against appearance_torch, the neutral grid, the C ABI and the
rejections of its entry points, BilateralGridBank on the host, and the generators and bars of tests/bilagrid_cases.py."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bilagrid_cases as B
import bags_raster
from bags_raster import BilateralGridBank, _lib, appearance_torch, apply_bilagrid, bilagrid_torch, bilagrid_tv_loss, bilagrid_tv_loss_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_bilagrid_forward", "bags_bilagrid_workspace_size", "bags_bilagrid_backward", "bags_bilagrid_tv_workspace_size",
         "bags_bilagrid_tv_forward", "bags_bilagrid_tv_backward")
F32, F64 = torch.float32, torch.float64
IDS = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the function
def published(img, G):
    """gsplat's slice-and-apply, literally: grid_sample over ((x+0.5)/W - 0.5)*2, ((y+0.5)/H - 0.5)*2 and luma*2 - 1, then the
    affine matmul.  ``img`` (V,3,H,W), ``G`` (V,12,L,Gy,Gx)."""
    V, _, H, W = img.shape
    xs = ((torch.arange(W, dtype=img.dtype) + 0.5) / W - 0.5) * 2
    ys = ((torch.arange(H, dtype=img.dtype) + 0.5) / H - 0.5) * 2
    rgb = img.permute(0, 2, 3, 1)                                                       # (V,H,W,3)
    luma = (rgb * torch.tensor([0.299, 0.587, 0.114], dtype=img.dtype)).sum(-1)
    coords = torch.stack([xs[None, None, :].expand(V, H, W), ys[None, :, None].expand(V, H, W), luma * 2 - 1], -1)[:, None]
    A = F.grid_sample(G, coords, mode="bilinear", align_corners=True, padding_mode="border")[:, :, 0]     # (V,12,H,W)
    A = A.permute(0, 2, 3, 1).reshape(V, H, W, 3, 4)
    out = torch.matmul(A[..., :3], rgb[..., None])[..., 0] + A[..., 3]
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize("H,W", B.SHAPES, **IDS)
@pytest.mark.parametrize("grid", B.GRIDS, **IDS)
def test_statement_is_the_published_formulation(grid, H, W):
    """Output, dL/dimage and dL/dgrid of bilagrid_torch in float64 against the grid_sample formulation, to 1e-12, on every case:
    1e-12 of the tensor's largest magnitude where that exceeds 1 -- an element of dL/dgrid is a sum over up to 10^4 pixels that
    reaches 10^2, and two float64 summation orders differ by 1e-16 * sum |terms| there."""
    for V in B.VIEWS:
        c = B.make_case(grid, H, W, V)
        out, g_img, g_grid = B.reference(grid, H, W, V)
        img = c["images"].double().requires_grad_(True)
        G = c["grids"][c["rows"]].double().requires_grad_(True)
        want = published(img, G)
        w_img, w_grid = torch.autograd.grad(want, [img, G], c["cot"].double())
        for got, ref, what in ((out, want.detach(), "out"), (g_img, w_img, "dL/dimage"), (g_grid, w_grid, "dL/dgrid")):
            assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), (V, what)


def test_guidance_term_is_zero_at_and_outside_the_borders():
    """s <= 0 and s >= L-1: dL/dimage is the direct term alone (torch.clamp would pass a gradient AT s = 0)."""
    G = (torch.eye(3, 4, dtype=F64).reshape(1, 12, 1, 1, 1) + 0.3 * torch.randn(1, 12, 4, 3, 3, dtype=F64, generator=torch.Generator().manual_seed(1)))
    for value in (0.0, -0.2, 1.5):
        img = torch.full((1, 3, 2, 2), value, dtype=F64, requires_grad=True)
        out = bilagrid_torch(img, G)
        (g,) = torch.autograd.grad(out, img, torch.ones_like(out))
        A = bags_raster.bilagrid._affine(img.detach(), G).reshape(1, 3, 4, 2, 2)
        assert (g - A[:, :, :3].sum(1)).abs().max().item() <= 1e-14, value              # (a guidance term would be of the order of 0.1)


def test_three_forms_of_images_are_one_function():
    c = B.make_case((5, 4, 3), 3, 5, 2)
    G = c["grids"][c["rows"]]
    stack = bilagrid_torch(c["images"], G)
    seq = bilagrid_torch([c["images"][0], c["images"][1]], G)
    one = bilagrid_torch(c["images"][1], G[1])
    assert isinstance(seq, list) and torch.equal(seq[0], stack[0]) and torch.equal(seq[1], stack[1]) and torch.equal(one, stack[1])
    with pytest.raises(ValueError, match="2 images but 1 grids"):
        bilagrid_torch(c["images"], G[:1])
    with pytest.raises(ValueError, match="grids must be"):
        bilagrid_torch(c["images"], G[:, :11])


def gsplat_total_variation_loss(x):
    """lib_bilagrid.total_variation_loss, literally (x: N, C, L, H, W)."""
    tv = 0
    for i in range(2, x.dim()):
        n = x.shape[i]
        x1 = x.index_select(i, torch.arange(1, n))
        x2 = x.index_select(i, torch.arange(0, n - 1))
        count = 1
        for d in x1.shape[1:]:
            count *= d
        tv = tv + torch.pow(x1 - x2, 2).sum() / count
    return tv / x.shape[0]


@pytest.mark.parametrize("n", (1, B.N))
@pytest.mark.parametrize("grid", B.GRIDS, **IDS)
def test_tv_statement_is_gsplats(grid, n):
    grids, _ = B.tv_case(grid, n)
    x = grids.double().requires_grad_(True)
    got = bilagrid_tv_loss_torch(x)
    assert got.dtype == F64 and got.dim() == 0 and torch.isfinite(got)
    if min(grid) >= 2:
        y = grids.double().requires_grad_(True)
        want = gsplat_total_variation_loss(y)
        assert abs(got.item() - want.item()) <= 1e-14 * want.item() and got.item() > 0
        assert (torch.autograd.grad(got, x)[0] - torch.autograd.grad(want, y)[0]).abs().max().item() <= 1e-15
    else:                                                     # upstream divides 0 by 0 on an axis of one vertex; here it counts 0
        assert torch.isnan(gsplat_total_variation_loss(grids.double()))
        sizes = dict(zip("xyz", grid))
        live = [a for a in "xyz" if sizes[a] >= 2]
        assert (got.item() > 0) == bool(live)
    l64, g64 = B.tv_reference(grid, n)
    assert l64.item() == got.item() and torch.isfinite(g64).all()


def test_one_vertex_grid_is_the_exposure_matrix():
    """A (1,1,1) grid is one affine matrix for the whole image: appearance_torch with k = 0 and E[j][c] = A[c][j]."""
    c = B.make_case((1, 1, 1), 17, 67, 2)
    G = c["grids"][c["rows"]].double()
    A = G.reshape(2, 3, 4)
    table = torch.zeros(2, 16, dtype=F64)
    E = table[:, :12].view(2, 3, 4)
    E[:, :, :3] = A[:, :, :3].transpose(1, 2)
    E[:, :, 3] = A[:, :, 3]
    got, want = bilagrid_torch(c["images"].double(), G), appearance_torch(c["images"].double(), table)
    assert (got - want).abs().max().item() <= 1e-14


@pytest.mark.parametrize("grid", B.GRIDS, **IDS)
def test_neutral_grid_returns_a_float32_image_bit_for_bit(grid):
    bank = BilateralGridBank(B.N, grid)
    for H, W in ((17, 67), (3, 5)):
        img = B.make_case(grid, H, W, 2)["images"]
        assert img.dtype == F32
        out = bilagrid_torch(img, bank.grids.detach()[[5, 9]])
        assert torch.equal(out, img)
    # grid_sample's weight form does not: the reason the statement is the lerp form
    img = B.make_case((16, 16, 8), 37, 259, 2)["images"]
    assert not torch.equal(published(img, BilateralGridBank(2).grids.detach()), img)


# ---------------------------------------------------------------------------------------------------------------- the bank
def test_bank_on_the_host():
    bank = BilateralGridBank(B.N, (5, 4, 3))
    assert len(bank) == B.N and tuple(bank.grids.shape) == (B.N, 12, 3, 4, 5) and isinstance(bank.grids, torch.nn.Parameter)
    assert list(bank.state_dict()) == ["grids"] and tuple(BilateralGridBank(2).grids.shape) == (2, 12, 8, 16, 16)
    assert torch.equal(bank.grids[7, :, 2, 1, 3].detach(), torch.eye(3, 4).reshape(12))
    c = B.make_case((5, 4, 3), 17, 67, 2)
    with torch.no_grad():
        bank.grids.copy_(c["grids"])
    other = BilateralGridBank(B.N, (5, 4, 3))
    other.load_state_dict(bank.state_dict())                  # gsplat's name and layout: a trained tensor loads as it is
    assert torch.equal(other.grids, bank.grids)
    want = bilagrid_torch(c["images"], c["grids"][c["rows"]])
    assert torch.equal(bank.apply(c["images"], c["rows"]).detach(), want)
    assert torch.equal(bank.apply(c["images"][1], c["rows"][1]).detach(), want[1])
    seq = bank.apply([c["images"][0], c["images"][1]], c["rows"])
    assert isinstance(seq, list) and torch.equal(seq[1].detach(), want[1])
    assert bank.tv_loss().item() == bilagrid_tv_loss_torch(c["grids"]).item() > 0 and BilateralGridBank(3).tv_loss().item() == 0.0
    A = bank.affine(c["images"], c["rows"])
    assert tuple(A.shape) == (2, 3, 4, 17, 67) and tuple(bank.affine(c["images"][0], c["rows"][0]).shape) == (3, 4, 17, 67)
    assert torch.allclose(torch.einsum("vcjhw,vjhw->vchw", A[:, :, :3], c["images"]) + A[:, :, 3], want, atol=1e-6)
    # upstream's one Adam: a step moves the listed row; the rows that are not listed stay neutral through the TV term too
    bank = BilateralGridBank(4, (5, 4, 3))
    opt = torch.optim.Adam([bank.grids], lr=0.01)
    (bank.apply(c["images"][0], [2]).square().sum() + 10 * bank.tv_loss()).backward()
    assert bank.grids.grad[[0, 1, 3]].abs().max().item() == 0.0 and bank.grids.grad[2].abs().max().item() > 0.0
    opt.step()
    assert torch.equal(bank.grids[[0, 1, 3]], BilateralGridBank(3, (5, 4, 3)).grids) and not torch.equal(bank.grids[2], other.grids[0])
    with pytest.raises(ValueError, match="listed twice"):
        bank.apply(c["images"], [1, 1])
    with pytest.raises(ValueError, match=r"not in \[0, 4\)"):
        bank.apply(c["images"][0], [4])
    with pytest.raises(ValueError, match="no cameras"):
        BilateralGridBank(0)
    with pytest.raises(ValueError, match="must be >= 1"):
        BilateralGridBank(2, (4, 0, 2))


def test_wrappers_refuse_what_they_cannot_run():
    """Without a GPU: host tensors into the HIP paths, and a host image into a bank on another device, are refused, not copied."""
    grids = BilateralGridBank(3, (5, 4, 3)).grids.detach()
    with pytest.raises(RuntimeError, match="AMD GPU.*bilagrid_torch"):
        apply_bilagrid(torch.rand(3, 4, 4), grids, [0])
    with pytest.raises(RuntimeError, match="AMD GPU.*bilagrid_tv_loss_torch"):
        bilagrid_tv_loss(grids)
    elsewhere = BilateralGridBank(3, (5, 4, 3), device="meta")     # stands for a bank on a GPU: its grids are not on the host
    with pytest.raises(RuntimeError, match="the grids are on meta but images.0. is on cpu.*AMD GPU"):
        elsewhere.apply(torch.rand(3, 4, 4), [0])
    with pytest.raises(RuntimeError, match="nothing is copied"):
        elsewhere.affine(torch.rand(2, 3, 4, 4), [0, 1])
    with pytest.raises(ValueError, match="grids must be"):
        bilagrid_tv_loss_torch(torch.zeros(12, 3, 4, 5))


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
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert [f[0] for f in _lib.BagsBilagrid._fields_] == _header_struct_fields("BagsBilagrid") == \
        ["N", "grids", "n_rows", "rows", "C", "H", "W", "Gx", "Gy", "L", "path", "image", "out"]
    S = _lib.BagsBilagrid
    assert (S.grids.offset, S.n_rows.offset, S.rows.offset, S.C.offset, S.Gx.offset, S.path.offset, S.image.offset, S.out.offset) == \
        (8, 16, 20, 84, 96, 108, 112, 240)
    assert C.sizeof(S) == 368
    for name in FUNCS:
        if "workspace_size" not in name:
            assert _lib.SYMBOLS[name][1][-1] is C.c_void_p, name                       # the stream comes last
    for name in ("TILE_W", "TILE_H", "STAGE_VERTS", "MAX_G", "MAX_L", "TV_BLOCK", "TV_MAX_BLOCKS", "PATH_AUTO", "PATH_DIRECT"):
        assert re.search(r"#define BAGS_BILAGRID_%s %d\b" % (name, getattr(_lib, "BILAGRID_" + name)), header), name
    assert (_lib.BILAGRID_MAX_G, _lib.BILAGRID_MAX_L) == (64, 16) and _lib.BILAGRID_TILE_W * _lib.BILAGRID_TILE_H == 256
    assert {"BilateralGridBank", "apply_bilagrid", "bilagrid_torch", "bilagrid_tv_loss", "bilagrid_tv_loss_torch"} <= set(bags_raster.__all__)
    assert "one ``torch.optim.Adam([bank.grids]" in BilateralGridBank.__doc__
    makefile = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "build/bilagrid.o" in makefile and "EXTRA_bilagrid = -ffp-contract=off" in makefile


def test_workspace_sizes(lib):
    """The slice's adjoint keeps nothing between its launches; the TV forward one row of 4 doubles per workgroup."""
    assert lib.bags_bilagrid_workspace_size(16, 1080, 1920) == 0
    size = lib.bags_bilagrid_tv_workspace_size
    for Gx, Gy, Lz in B.GRIDS:
        for n in (1, B.N, 200):
            elems = n * 12 * Lz * Gy * Gx
            blocks = min(-(-elems // _lib.BILAGRID_TV_BLOCK), _lib.BILAGRID_TV_MAX_BLOCKS)
            assert blocks * 32 <= size(n, Gx, Gy, Lz) < blocks * 32 + 256 and size(n, Gx, Gy, Lz) % 16 == 0
    assert size(0, 4, 4, 4) == 0 and size(1, 0, 4, 4) == 0 and size(1, 65, 4, 4) == 0 and size(1, 4, 4, 17) == 0 and size(1, 4, -1, 4) == 0


def test_every_rejection_is_reached_without_a_device(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 255) & ~255

    def args(N=23, n_rows=2, rows=(4, 1), Cn=3, H=6, W=10, grid=(5, 4, 3), path=0, **edit):
        k = max(0, min(n_rows, 16))
        a = _lib.BagsBilagrid(N, addr, n_rows, (C.c_int32 * 16)(*rows), Cn, H, W, *grid, path, (_lib.c_fp * 16)(*[addr] * k), (_lib.c_fp * 16)(*[addr] * k))
        for n, v in edit.items():
            setattr(a, n, v)
        return a

    ptrs = (_lib.c_fp * 16)(*[addr] * 16)

    def fwd(a):
        return lib.bags_bilagrid_forward(C.byref(a) if a is not None else None, None)

    def bwd(a, g_out=ptrs, g_image=ptrs, g_grids=addr + 2048):
        return lib.bags_bilagrid_backward(C.byref(a) if a is not None else None, g_out, None, 0, g_image, g_grids, None)

    def refused(rc, *texts):
        msg = lib.bags_last_error().decode()
        assert rc == -1 and "bilagrid" in msg and all(t in msg for t in texts), (rc, msg)            # BAGS_ERR_ARG

    for call in (fwd, bwd):
        refused(call(None), "null struct")
        refused(call(args(grids=None)), "null grids")
        refused(call(args(N=0)), "N 0 < 1")
        refused(call(args(n_rows=0)), "n_rows 0 not in 1..16")
        refused(call(args(n_rows=17)), "n_rows 17 not in 1..16")
        refused(call(args(rows=(4, 23))), "rows[1] = 23 is not in [0, 23)")
        refused(call(args(rows=(4, 4))), "row 4 is listed twice")
        refused(call(args(H=0)), "empty image")
        refused(call(args(Cn=4)), "C must be 3")
        refused(call(args(H=1 << 16, W=1 << 15)), "2^31 pixels", "bilagrid_torch")
        refused(call(args(grid=(5, 4, 17))), "(5, 4, 17)", "bilagrid_torch")
        refused(call(args(grid=(0, 4, 3))), "(0, 4, 3)", "bilagrid_torch")
        refused(call(args(grid=(5, 65, 3))), "(5, 65, 3)", "bilagrid_torch")
        refused(call(args(grid=(5, 4, 0))), "(5, 4, 0)", "bilagrid_torch")
        refused(call(args(path=2)), "path 2")
        a = args()
        a.image[1] = None
        refused(call(a), "null image[1]")
    a = args()
    a.out[0] = None
    refused(fwd(a), "null out[0]")
    refused(bwd(args(), g_out=None), "null g_out")
    g = (_lib.c_fp * 16)(*[addr] * 16)
    g[1] = None
    refused(bwd(args(), g_out=g), "null g_out[1]")
    refused(bwd(args(), g_grids=addr), "must not be the grids")
    # nothing wanted: a successful no-op that launches nothing
    assert bwd(args(), g_image=None, g_grids=None) == 0
    assert bwd(args(), g_image=(_lib.c_fp * 16)(), g_grids=None) == 0
    # the total variation
    need = lib.bags_bilagrid_tv_workspace_size(23, 5, 4, 3)

    def tvf(grids=addr, N=23, grid=(5, 4, 3), ws=addr + 256, ws_bytes=need, loss=addr + 2048):
        return lib.bags_bilagrid_tv_forward(grids, N, *grid, ws, ws_bytes, loss, None)

    def tvb(grids=addr, N=23, grid=(5, 4, 3), g_loss=addr + 256, g_grids=addr + 2048):
        return lib.bags_bilagrid_tv_backward(grids, N, *grid, g_loss, g_grids, None)

    for call in (tvf, tvb):
        refused(call(grids=None), "null grids")
        refused(call(N=0), "N 0 < 1")
        refused(call(grid=(5, 4, 17)), "(5, 4, 17)", "bilagrid_torch")
        refused(call(grid=(0, 4, 3)), "(0, 4, 3)")
    refused(tvf(loss=None), "null loss")
    refused(tvf(ws=None), "needs a workspace of %d bytes" % need)
    refused(tvf(ws_bytes=need - 1), "needs a workspace of %d bytes (got %d)" % (need, need - 1))
    refused(tvf(ws=addr + 256 + 8), "not 16-byte aligned")
    refused(tvb(g_loss=None), "null g_loss")
    refused(tvb(g_grids=None), "null g_grids")
    refused(tvb(g_grids=addr), "must not be the grids")


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_cases_are_what_the_gpu_tests_say_they_are():
    assert B.GRIDS == ((16, 16, 8), (5, 4, 3), (2, 3, 2), (1, 1, 1)) and B.VIEWS == (1, 2, 16, 17) and B.N == 23
    assert B.SHAPES[:5] == ((1, 1), (3, 5), (16, 64), (17, 67), (37, 259)) and B.SHAPES[5] == B.DERIVED
    H, W = B.DERIVED
    assert H % B.TILE_H != 0 and W % B.TILE_W != 0 and H > B.TILE_H and W > B.TILE_W
    paths = {g: B.tile_paths(g, H, W) for g in B.GRIDS}
    assert paths[(16, 16, 8)][0] > 0 and paths[(16, 16, 8)][1] > 0          # one launch of the derived shape takes both paths
    assert B.tile_paths((16, 16, 8), 3, 5) == (0, 1)                         # an image smaller than its grid: direct
    assert any(n > B.BLOCK and n % B.BLOCK != 0 for n in B.rectangles((5, 4, 3), H, W))
    for grid, (H, W), V in (((16, 16, 8), (37, 259), 17), ((5, 4, 3), B.DERIVED, 2), ((2, 3, 2), (17, 67), 16), ((16, 16, 8), (3, 5), 16)):
        c = B.make_case(grid, H, W, V)
        img, kind, Lz = c["images"], c["kind"], grid[2]
        assert img.dtype == F32 and img.is_contiguous() and tuple(img.shape) == (V, 3, H, W)
        each = int((kind == 1).sum())
        assert each >= 1 and int((kind == 2).sum()) == each == int((kind == 3).sum()) and abs(2 * each / kind.numel() - 0.02) < 0.012
        px = img.permute(0, 2, 3, 1)
        assert (px[kind == 1] >= 1.01).all() and (px[kind == 2] <= -0.01).all() and (px[kind == 3] == 0).all()
        assert ((px[kind == 0] >= 0) & (px[kind == 0] <= 1)).all() and not (px == 1).all(-1).any()          # no white pixels
        s64, s32 = B.s_of(img, Lz, F64), B.s_of(img, Lz, F32)
        # every pixel but the black ones keeps its distance from the jumps of the guidance term ...
        assert (B.distance_to_integers(s64, Lz)[kind != 3] >= B.S_MARGIN).all()
        assert ((s32.double() - s64).abs() <= B.S_MARGIN / 250).all()                 # ... hundreds of times the float32 error of s (|s| reaches 10)
        # ... and the deliberate pixels classify identically in both precisions: black ones s == 0 (not live), the others outside
        assert (s64[kind == 3] == 0).all() and (s32[kind == 3] == 0).all()
        assert (s64[kind == 1] > Lz - 1).all() and (s32[kind == 1] > Lz - 1).all() and (s64[kind == 2] < 0).all() and (s32[kind == 2] < 0).all()
        assert torch.equal(s64.clamp(0, Lz - 1).floor(), s32.clamp(0, Lz - 1).floor().double())            # one z-bin in both
        G = c["grids"]
        assert tuple(G.shape) == (B.N, 12, Lz, grid[1], grid[0]) and (G - torch.eye(3, 4).reshape(1, 12, 1, 1, 1)).abs().max() <= 0.3
        assert G.reshape(B.N, 12, -1).std(-1).min() > 0.05 if G[0, 0].numel() > 1 else True      # differs from vertex to vertex
        assert len(set(c["rows"])) == V and (V == 1 or c["rows"] != sorted(c["rows"])) and all(0 <= r < B.N for r in c["rows"])
        assert (c["cot"] < 0).float().mean() > 0.2 and (c["cot"] > 0).float().mean() > 0.5
        assert B.make_case(grid, H, W, V) is c and torch.equal(B.make_case.__wrapped__(grid, H, W, V)["images"], img)       # seeded
        # the guidance term is not small: where it is live it carries a good part of dL/dimage
        _, g_img, g_grid = B.reference(grid, H, W, V)
        frozen = c["images"].double().requires_grad_(True)
        A = bags_raster.bilagrid._affine(c["images"].double(), c["grids"][c["rows"]].double()).reshape(V, 3, 4, H, W)
        direct = torch.einsum("vchw,vcjhw->vjhw", c["cot"].double(), A[:, :, :3])
        assert ((g_img - direct).abs().mean() > 0.1 * direct.abs().mean()) and frozen.grad is None
        if (H, W) == (3, 5):                                   # most vertices are unreached: exact zeros in the reference too
            assert (g_grid == 0).float().mean() > 0.5
    tiny = B.make_case((16, 16, 8), 1, 1, 1)
    assert tuple(tiny["images"].shape) == (1, 3, 1, 1) and int((tiny["kind"] != 0).sum()) == 0


def test_image_gradient_scale_is_the_sum_of_terms():
    """The choice recorded at bilagrid_cases.IMAGE_SCALE: the float32 PyTorch path does not stay inside 16 eps32 * (1 + |ref|)
    for dL/dimage, so that bar's scale is the pixel's sum |terms|; for the output it does stay inside, as the rule expects."""
    assert B.IMAGE_SCALE == "terms"
    worst_out = worst_img = worst_scale = 0.0
    for grid in B.GRIDS:
        for H, W in ((37, 259), B.DERIVED):
            r, f = B.reference(grid, H, W, 2), B.float32_path(grid, H, W, 2)
            image_abs, grid_abs = B.term_sums(grid, H, W, 2)
            floor = B.FLOOR_EPS * B.EPS32
            worst_out = max(worst_out, float(((f[0] - r[0]).abs() / (floor * (1 + r[0].abs()))).max()))
            worst_img = max(worst_img, float(((f[1] - r[1]).abs() / (floor * (1 + r[1].abs()))).max()))
            worst_scale = max(worst_scale, float((image_abs / (1 + r[1].abs())).max()))
            # sum |terms| bounds |sum|: the references are inside their own scales
            assert (r[1].abs() <= image_abs * (1 + 1e-12)).all() and (r[2].abs() <= grid_abs * (1 + 1e-12) + 1e-300).all()
            bar = B.bars(grid, H, W, 2)
            assert all(bool(((f[i] - r[i]).abs() <= bar[i]).all()) for i in range(3))
            assert (bar[0] > 0).all() and (bar[1] > 0).all() and ((bar[2] > 0) | (r[2] == 0)).all()
    print("float32 path over 16 eps (1 + |ref|): out %.2f  dL/dimage %.2f;  largest sum|terms| / (1 + |ref|) %.1f" % (worst_out, worst_img, worst_scale))
    assert worst_out <= 1.0 < worst_img and worst_scale > 10
