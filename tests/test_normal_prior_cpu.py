"""No-GPU checks of the normal prior (bags_raster/normal_prior.py, csrc/normal_prior.hip): the PyTorch statement against the closed
forms, that the bars of tests/normal_prior_cases.py reject wrong answers, a tilted plane, the generator's conditions, the degenerate
views in float64, pinhole_of against the oracle's projection, the C surface and every rejection of its entry points."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import normal_prior_cases as P
import bags_raster
from bags_raster import _lib, depth_to_normal, depth_to_normal_torch, normal_prior_loss, normal_prior_loss_torch, pinhole_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_normal_prior_workspace_size", "bags_normal_prior_forward", "bags_normal_prior_backward", "bags_depth_to_normal")
PUBLIC = ("normal_prior_loss", "normal_prior_loss_torch", "depth_to_normal", "depth_to_normal_torch", "pinhole_of")
F64 = torch.float64
JUMPS = (P.MAX_JUMP, math.inf)
IDS = ["%dx%d" % s for s in P.SHAPES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the function
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_statement_equals_the_closed_forms(H, W, mode):
    """normal_prior_loss_torch in float64 with autograd against the closed forms of the loss and of both gradients, element by
    element to round-off, with the guard on and off; exact zeros where the closed form has zeros."""
    for V in (2, 17):
        c = P.make_case(H, W, V, mode)
        for mj in JUMPS:
            ref, want = P.reference(H, W, V, mode, mj), P.closed_form(c, mj)
            for name, a, b in zip(("loss", "dL/dD", "dL/dA"), ref[:3], want):
                assert a.shape == b.shape and torch.isfinite(a).all(), name
                assert bool(((a - b).abs() <= 1e-12 * (1 + b.abs())).all()), (name, float((a - b).abs().max()))
                assert bool(((b == 0) <= (a == 0)).all()), name
            assert (ref[3] - P._pieces(c, mj)["cnt"]).abs().max() < 1e-12
            if (H, W) in P.FLAT:
                assert ref[0].abs().max() == 0 and ref[1].abs().max() == 0 and ref[2].abs().max() == 0 and ref[3].abs().max() == 0
            else:
                assert ((ref[0] > 0) == (ref[3] > 0)).all() and (ref[3] > 0).any() and ref[1].abs().max() > 0 and ref[2].abs().max() > 0


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("H,W", [s for s in P.SHAPES if s not in P.FLAT], ids=["%dx%d" % s for s in P.SHAPES if s not in P.FLAT])
def test_bars_reject_wrong_answers(H, W, mode):
    """The closed form with the n (n . g) projection dropped, with the sign of dL/dA flipped, and with 1/cnt replaced by 1 / (H W),
    is outside the bars on every case with an interior; the closed forms themselves are far inside."""
    for V in P.VIEWS:
        c = P.make_case(H, W, V, mode)
        for mj in JUMPS:
            good = P.margins(H, W, V, mode, P.closed_form(c, mj), mj)
            assert all(m <= 1e-3 for m in good), good
            m = P.margins(H, W, V, mode, P.closed_form(c, mj, drop_projection=True), mj)
            assert m[1] > 1.0 and m[2] > 1.0, ("drop_projection", V, m)
            m = P.margins(H, W, V, mode, P.closed_form(c, mj, flip_dA=True), mj)
            assert m[1] <= 1e-3 and m[2] > 1.0, ("flip_dA", V, m)
            m = P.margins(H, W, V, mode, P.closed_form(c, mj, n_is_pixels=True), mj)
            assert m[1] > 1.0 and m[2] > 1.0, ("n_is_pixels", V, m)


def _plane(H, W, pin, normal, d, dtype=F64):
    """Depth z(u,v) of the plane normal . X = d through the pinhole: z = d / (normal . ray)."""
    fx, fy, cx, cy = pin
    u = torch.arange(W, dtype=F64)[None, :].expand(H, W)
    v = torch.arange(H, dtype=F64)[:, None].expand(H, W)
    ray = torch.stack([(u - cx) / fx, (v - cy) / fy, torch.ones(H, W, dtype=F64)], 0)
    return (d / (normal.view(3, 1, 1) * ray).sum(0)).to(dtype)


def test_a_tilted_plane_gives_its_normal_at_every_interior_pixel():
    H, W, pin = 23, 31, (27.5, 29.25, 14.625, 11.375)
    nrm = torch.tensor((0.3, -0.2, -1.0), dtype=F64)
    nrm = nrm / nrm.norm()
    z = _plane(H, W, pin, nrm, -3.0)
    assert z.min() > 1.5
    A = torch.full((1, H, W), 0.8125, dtype=F64)
    D = A * z[None]
    n, valid = depth_to_normal_torch(D, A, pin)
    inner = torch.zeros(H, W, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    assert n.dtype == F64 and tuple(n.shape) == (3, H, W) and valid.dtype == torch.bool and torch.equal(valid, inner)
    err = (n - nrm.view(3, 1, 1))[:, inner].abs().max().item()
    print("\ntilted plane: largest |n - plane normal| %.3g" % err)
    assert err <= 1e-12 and n[:, ~inner].abs().max() == 0
    prior = nrm.view(3, 1, 1).expand(3, H, W).contiguous()
    for mode in P.MODES:
        loss, count = normal_prior_loss_torch(D, A, prior, pin, mode=mode)
        assert abs(loss.item()) <= 1e-12 and count.item() == (H - 2) * (W - 2)
    # a fronto-parallel wall faces the camera
    wall, ok = depth_to_normal_torch(torch.full((1, 5, 7), 2.0, dtype=F64), torch.ones(1, 5, 7, dtype=F64), (6.0, 6.5, 3.2, 1.9))
    assert ok[1:-1, 1:-1].all() and (wall[2][ok] == -1).all() and wall[:2].abs().max() == 0
    # the guard drops the centres next to a step, and only them
    step = torch.full((1, 9, 12), 3.0, dtype=F64)
    step[:, :, 6:] = 2.0
    _, ok = depth_to_normal_torch(step, torch.ones_like(step), pin, max_jump=0.25)
    want = torch.zeros(9, 12, dtype=torch.bool)
    want[1:-1, 1:-1] = True
    want[:, 5:7] = False
    assert torch.equal(ok, want)
    _, ok = depth_to_normal_torch(step, torch.ones_like(step), pin)
    assert int(ok.sum()) == 7 * 10


@pytest.mark.parametrize("mode", P.MODES)
def test_generator_conditions_hold_on_every_case(mode):
    worst = dict(gap=1.0, valid=1.0, jump=1.0, prior=1.0, kink=1.0)
    for H, W in P.SHAPES:
        for V in P.VIEWS:
            c = P.make_case(H, W, V, mode)
            f = P.check_case(c)
            assert f == c["figures"]
            worst = {k: min(worst[k], f[k]) for k in worst}
            assert c["D"].dtype == torch.float32 and tuple(c["D"].shape) == (V, 1, H, W) == tuple(c["A"].shape)
            assert tuple(c["prior"].shape) == (V, 3, H, W) and tuple(c["mask"].shape) == (V, H, W) and (c["mask"] >= 0).all()
            pin = c["pinhole"]
            assert tuple(pin.shape) == (V, 4) and pin.dtype == F64 and (pin[:, 0] >= 0.9 * W).all() and (pin[:, 0] <= 1.2 * W).all()
            assert ((pin[:, 1] / pin[:, 0] - 1).abs() <= 0.05 + 1e-6).all() and (pin[:, 2] - (W - 1) / 2).abs().max() <= 1.5
            assert V == 1 or (len(set(pin[:, 0].tolist())) == V and (c["cot"] > 0).any() and (c["cot"] < 0).any())
            if H * W >= 64:
                q_on, q_off = P._pieces(c), P._pieces(c, math.inf)
                assert c["prior"].isnan().any() and (c["prior"].abs().sum(1) == 0).any() and (c["A"] < 0.4).any()
                assert (c["mask"] == 0).any() and ((c["mask"] > 0) & (c["mask"] < 1)).any()
                assert int(q_on["geometric"].sum()) < int(q_off["geometric"].sum())          # max_jump = 0.25 has edges to drop
                z = (c["D"] / c["A"])[c["A"] >= 0.55]
                assert z.min() >= 1.2 and z.max() <= 4.2
            # float32 and float64 agree on every validity decision
            for mj in JUMPS:
                assert torch.equal(P.float32_path(H, W, V, mode, mj)[3], P.reference(H, W, V, mode, mj)[3].float().double())
            assert P.make_case(H, W, V, mode) is c                                       # cached
    print("\n%s: smallest |A - min_weight| %.3g, valid share %.3f, |jump - max_jump| %.3g, ||p|^2 - 0.25| %.3g, |n_k - ph_k| %.3g"
          % (mode, *worst.values()))
    assert P.SHAPES[:8] == ((1, 1), (2, 7), (7, 2), (3, 3), (3, 5), (16, 64), (17, 67), (37, 259)) and P.VIEWS == (1, 2, 16, 17)
    H, W = P.SEAM
    assert H * W < 100000 and -(-H // P.TILE_H) >= 2 and -(-W // P.TILE_W) >= 2 and H % P.TILE_H and W % P.TILE_W and P.SHAPES[8] == P.SEAM
    assert all(h * w < 100000 for h, w in P.SHAPES)


@pytest.mark.parametrize("mode", P.MODES)
def test_degenerate_views_in_float64(mode):
    """No solid pixel, an all-zero mask, an all-NaN prior: loss 0, count 0 and all-zero gradients, never NaN; a single valid centre:
    its own l, and gradients at its four neighbours only."""
    c = P.degenerate_case(mode)
    loss, gD, gA, count = P.run_torch(c, F64)
    assert all(torch.isfinite(t).all() for t in (loss, gD, gA, count))
    k = P.DEGENERATE_VIEWS
    for v in c["degenerate"]:
        assert loss[v] == 0 and count[v] == 0 and gD[v].abs().max() == 0 and gA[v].abs().max() == 0, v
    v = k["one_centre"]
    assert count[v] == 0.625 and loss[v] > 0 and int((gD[v] != 0).sum()) == 4 == int((gA[v] != 0).sum())
    at = c["mask"][v].nonzero()[0]
    assert gD[v][0, at[0], at[1]] == 0                                                   # the centre's own z enters only the guard
    q = P._pieces(c)
    lpix = (q["n"] - q["ph"]).abs().sum(-1) if mode == "l1" else 1.0 - (q["n"] * q["ph"]).sum(-1)
    assert abs(float(loss[v]) - float(lpix[v, at[0], at[1]])) < 1e-14
    live = [i for i in range(16) if i not in c["degenerate"]]
    for i in live:
        assert loss[i] != 0 and gD[i].abs().max() > 0 and gA[i].abs().max() > 0
    l32 = P.run_torch(c, torch.float32)[0]                                               # float32 takes the same branches
    assert all(l32[i] == 0 for i in c["degenerate"]) and all(l32[i] != 0 for i in live)
    want = P.closed_form(c)
    for a, b in zip((loss, gD, gA), want):
        assert bool(((a - b).abs() <= 1e-12 * (1 + b.abs())).all())
    base = P.make_case(17, 67, 16, mode)
    keep = [i for i in range(16) if i not in k.values()]
    assert all(torch.equal(c[n][keep], base[n][keep]) for n in ("D", "A", "mask", "prior") if not c[n][keep].isnan().any()) and len(keep) == 12


def test_statement_forms():
    c = P.make_case(16, 64, 2, "l1")
    D, A, p, m, pin = c["D"], c["A"], c["prior"], c["mask"], c["pinhole"]
    kw = dict(mode="l1", max_jump=P.MAX_JUMP)
    one = normal_prior_loss_torch(D[0], A[0], p[0], pin[0], m[0], **kw)
    seq = normal_prior_loss_torch([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], pin, [m[0], m[1]], **kw)
    assert one[0].shape == (1,) and seq[0].shape == (2,) and one[0].dtype == torch.float32 and torch.equal(one[0], seq[0][:1])
    assert torch.equal(one[1], seq[1][:1])
    # (H,W) maps, a None mask entry, no mask at all, pinholes as tuples, as a list of tuples and as a CPU tensor
    a = normal_prior_loss_torch(D[0, 0], A[0, 0], p[0], tuple(pin[0].tolist()), None)
    b = normal_prior_loss_torch([D[0]], [A[0]], [p[0]], [tuple(pin[0].tolist())], [None])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].item() > 0
    # one pinhole serves every view
    both = normal_prior_loss_torch([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], pin[0], None)
    assert torch.equal(both[0][:1], a[0]) and not torch.equal(both[0][1:], normal_prior_loss_torch(D[1], A[1], p[1], pin[1])[0])
    # the length of the prior does not matter; a short one is no prior
    long = normal_prior_loss_torch(D[0].double(), A[0].double(), 1.7 * p[0].double(), pin[0])
    same = normal_prior_loss_torch(D[0].double(), A[0].double(), p[0].double(), pin[0])
    assert abs(float(long[0] - same[0])) < 1e-12 and long[1] == same[1]
    assert normal_prior_loss_torch(D[0], A[0], 0.4 * p[0], pin[0])[1].item() == 0


def test_wrapper_refuses_what_it_cannot_run():
    c = P.make_case(3, 5, 2, "cos")
    D, A, p, m, pin = c["D"], c["A"], c["prior"], c["mask"], c["pinhole"]
    with pytest.raises(RuntimeError, match="AMD GPU"):
        normal_prior_loss(D[0], A[0], p[0], pin[0])          # host tensors into the HIP path: refused, not copied
    with pytest.raises(RuntimeError, match="AMD GPU"):
        depth_to_normal(D[0], A[0], pin[0])
    for fn in (normal_prior_loss, normal_prior_loss_torch):
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            fn(D[0], A[0], p[0], pin[0], m[0] > 0)
        with pytest.raises(ValueError, match="mode must be"):
            fn(D[0], A[0], p[0], pin[0], mode="pearson")
        with pytest.raises(ValueError, match="one size"):
            fn(D[0], torch.rand(1, 3, 6), p[0], pin[0])
        with pytest.raises(ValueError, match=r"prior\[0\] must be \(3,H,W\)"):
            fn(D[0], A[0], p[0][:2], pin[0])
        with pytest.raises(ValueError, match=r"prior\[0\] must be \(3,H,W\)"):
            fn(D[0], A[0], torch.rand(3, 3, 6), pin[0])
        with pytest.raises(ValueError, match="2 depth maps but 1 prior"):
            fn([D[0], D[1]], [A[0], A[1]], [p[0]], pin)
        with pytest.raises(ValueError, match="2 views but 3 pinholes"):
            fn([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], [tuple(pin[0].tolist())] * 3)
        with pytest.raises(ValueError, match="four finite numbers"):
            fn(D[0], A[0], p[0], (1.0, 2.0, 3.0))
        with pytest.raises(ValueError, match="four finite numbers"):
            fn(D[0], A[0], p[0], (0.0, 2.0, 3.0, 1.0))
        with pytest.raises(ValueError, match="four finite numbers"):
            fn(D[0], A[0], p[0], (1.0, 2.0, float("nan"), 1.0))
        with pytest.raises(ValueError, match="min_weight must be a positive number"):
            fn(D[0], A[0], p[0], pin[0], min_weight=0.0)
        with pytest.raises(ValueError, match="max_jump must be"):
            fn(D[0], A[0], p[0], pin[0], max_jump=-1.0)
        with pytest.raises(ValueError, match="max_jump must be"):
            fn(D[0], A[0], p[0], pin[0], max_jump=float("nan"))
        with pytest.raises(ValueError, match="must be a non-empty"):
            fn(torch.rand(2, 3, 5), A[0], p[0], pin[0])
    for fn in (depth_to_normal, depth_to_normal_torch):
        with pytest.raises(ValueError, match="one view per call"):
            fn([D[0], D[1]], [A[0], A[1]], pin[0])
        with pytest.raises(ValueError, match="min_weight must be a positive number"):
            fn(D[0], A[0], pin[0], min_weight=-0.5)
    with pytest.raises(ValueError, match=r"\(3,3\) matrix"):
        pinhole_of(torch.eye(2), 4, 4)
    doc = bags_raster.normal_prior.__doc__
    assert "NO gradient to the intrinsics" in doc and "intrinsics" in normal_prior_loss.__doc__


def test_the_three_texts_state_the_same_function():
    """The rules of the function, line by line, in the module docstring, the header comment and the kernel header."""
    def rules(text, strip):
        lines = [re.sub(r"\s+", " ", ln.strip().lstrip(strip).strip()) for ln in text.splitlines()]
        first = next(i for i, ln in enumerate(lines) if ln.startswith("solid(u,v)"))
        return lines[first:first + 12]
    doc = rules(bags_raster.normal_prior.__doc__, "")
    header = rules(open(os.path.join(ROOT, "include", "bags_raster.h")).read(), "*")
    kernel = rules(open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "normal_prior.hip")).read(), "/")
    assert doc == header == kernel and doc[-1].startswith("L_v = sum w l / cnt") and len(set(doc)) == 12


def test_pinhole_of_agrees_with_the_oracle_projection():
    """Random view-space points through oracle/raster_oracle.py's preprocess (identity view matrix, the projection matrix is the
    intrinsic) land where the pinhole of pinhole_of puts them, to 1e-12 in float64 (the oracle divides by w + 1e-7: so does the
    expectation)."""
    from oracle import raster_oracle as O
    from scenes import make_case, oracle_settings
    _, cam = make_case(8, 40, 28, 1.0, 0, seed=1)
    H, W = cam.image_height, cam.image_width
    K = cam.get_intrinsic().detach().double().clone()
    K[2, 0], K[2, 1] = 0.03, -0.02                                                       # a principal point off centre
    s = oracle_settings(cam, 0)
    s.viewmatrix, s.projmatrix, s.intrinsic, s.campos = torch.eye(4, dtype=F64), K, K, torch.zeros(3, dtype=F64)
    g = torch.Generator().manual_seed(11)
    n = 64
    zv = 1.0 + 4.0 * torch.rand(n, generator=g, dtype=F64)
    X = torch.stack([(torch.rand(n, generator=g, dtype=F64) - 0.5) * 0.5 * zv, (torch.rand(n, generator=g, dtype=F64) - 0.5) * 0.4 * zv, zv], 1)
    pre = O.preprocess(X, torch.zeros(n, 3, dtype=F64), None, None, torch.rand(n, 3, generator=g, dtype=F64), torch.full((n, 1), 0.5, dtype=F64),
                       torch.full((n, 3), 0.05, dtype=F64), torch.tensor((1.0, 0, 0, 0), dtype=F64).repeat(n, 1), None, s, dtype=F64)
    assert pre.visible.all()
    fx, fy, cx, cy = pinhole_of(K, H, W)
    assert pinhole_of(K.float(), H, W) == pytest.approx((fx, fy, cx, cy), rel=1e-6) and all(isinstance(t, float) for t in (fx, fy, cx, cy))
    c0x, c0y, zg = (W - 1) / 2, (H - 1) / 2, X[:, 2] + 1e-7
    want = torch.stack([(fx * X[:, 0] + (cx - c0x) * X[:, 2]) / zg + c0x, (fy * X[:, 1] + (cy - c0y) * X[:, 2]) / zg + c0y], 1)
    err = (pre.xy - want).abs().max().item()
    print("\npinhole_of against the oracle: %.3g px" % err)
    assert err <= 1e-12 * max(H, W) and abs(cx - c0x) > 0.5 and abs(cy - c0y) > 0.2


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
        if name != "bags_normal_prior_workspace_size":                                   # the stream comes last
            assert decl.rstrip().endswith("void* stream") and _lib.SYMBOLS[name][1][-1] is C.c_void_p, name
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert [f[0] for f in _lib.BagsNormalPrior._fields_] == _header_struct_fields("BagsNormalPrior") == \
        ["mode", "H", "W", "min_weight", "max_jump", "n_rows", "pinhole", "depth", "weights", "prior", "mask"]
    B = _lib.BagsNormalPrior
    assert (B.H.offset, B.min_weight.offset, B.max_jump.offset, B.n_rows.offset, B.pinhole.offset, B.depth.offset, B.mask.offset) == \
        (4, 12, 16, 20, 24, 536, 920)
    assert C.sizeof(B) == 1048
    for name, value in (("TILE_W", _lib.NORMAL_PRIOR_TILE_W), ("TILE_H", _lib.NORMAL_PRIOR_TILE_H), ("STATS", _lib.NORMAL_PRIOR_STATS),
                        ("COS", _lib.NORMAL_PRIOR_COS), ("L1", _lib.NORMAL_PRIOR_L1)):
        assert re.search(r"#define BAGS_NORMAL_PRIOR_%s %d\b" % (name, value), header), name
    assert _lib.NORMAL_PRIOR_TILE_W * _lib.NORMAL_PRIOR_TILE_H == 256
    assert set(PUBLIC) <= set(bags_raster.__all__) and all(hasattr(bags_raster, n) for n in PUBLIC)
    makefile = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "build/normal_prior.o" in makefile and "EXTRA_normal_prior = -ffp-contract=off" in makefile


def test_workspace_size(lib):
    """Grows with the views and with the tiles, a multiple of 16, one row of 2 doubles per tile (rounded up to 256 bytes); 0 for
    arguments the entries refuse."""
    size = lib.bags_normal_prior_workspace_size
    for H, W in P.SHAPES + ((1080, 1920),):
        sizes = [size(n, H, W) for n in range(1, 17)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert P.tiles(H, W) < 16 or all(a < b for a, b in zip(sizes, sizes[1:]))
        assert sizes == [-(-n * P.tiles(H, W) * 16 // 256) * 256 for n in range(1, 17)]
    assert P.tiles(1, 1) == 1 and P.tiles(17, 67) == 9 and P.tiles(*P.SEAM) == 12 and P.tiles(1080, 1920) == 60 * 135
    assert size(16, 8, 32) < size(16, 9, 32) == size(16, 16, 32) < size(16, 16, 33)
    assert size(0, 8, 8) == 0 and size(17, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 8, -1) == 0 and size(1, 1 << 16, 1 << 15) == 0
    assert size(1, 65535 * 8, 1) > 0 and size(1, 65535 * 8 + 1, 1) == 0


def test_every_rejection_is_reached_without_a_device(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 8192)()
    addr = (C.addressof(buf) + 255) & ~255
    inf, nan = float("inf"), float("nan")

    def args(mode=0, H=6, W=10, min_weight=0.5, max_jump=inf, n_rows=2, pin=(9.0, 9.5, 4.5, 2.5), **edit):
        k = max(0, min(n_rows, 16))
        field = ((C.c_double * 4) * 16)()
        for i in range(k):
            field[i][:] = pin
        a = _lib.BagsNormalPrior(mode, H, W, min_weight, max_jump, n_rows, field, (_lib.c_fp * 16)(*[addr] * k), (_lib.c_fp * 16)(*[addr] * k),
                                 (_lib.c_fp * 16)(*[addr] * k), (_lib.c_fp * 16)(*[addr] * k))
        for n, v in edit.items():
            setattr(a, n, v)
        return a

    ptrs = (_lib.c_fp * 16)(*[addr] * 16)
    need = lib.bags_normal_prior_workspace_size(2, 6, 10)

    def fwd(a, ws=addr + 256, ws_bytes=None, loss=addr + 2048, count=addr + 2112, stats=addr + 2176):
        return lib.bags_normal_prior_forward(C.byref(a) if a is not None else None, ws, need if ws_bytes is None else ws_bytes, loss, count, stats, None)

    def bwd(a, stats=addr + 2176, g_loss=addr + 2048, g_depth=ptrs, g_weights=ptrs):
        return lib.bags_normal_prior_backward(C.byref(a) if a is not None else None, stats, g_loss, g_depth, g_weights, None)

    def d2n(depth=addr, weights=addr, H=6, W=10, pin=(9.0, 9.5, 4.5, 2.5), min_weight=0.5, max_jump=inf, normal=addr + 1024, valid=addr + 4096):
        return lib.bags_depth_to_normal(depth, weights, H, W, None if pin is None else (C.c_double * 4)(*pin), min_weight, max_jump, normal, valid, None)

    def refused(rc, text, op="normal_prior"):
        msg = lib.bags_last_error().decode()
        assert rc == -1 and op in msg and text in msg, (rc, msg)                          # BAGS_ERR_ARG

    assert "BAGS_ERR_ARG = -1" in open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for call in (fwd, bwd):
        refused(call(None), "null struct")
        refused(call(args(mode=2)), "unknown mode 2")
        refused(call(args(n_rows=0)), "n_rows 0 not in 1..16")
        refused(call(args(n_rows=17)), "n_rows 17 not in 1..16")
        refused(call(args(H=0)), "empty image")
        refused(call(args(W=-2)), "empty image")
        refused(call(args(H=1 << 16, W=1 << 15)), "2^31 pixels")
        refused(call(args(H=65535 * 8 + 1, W=1)), "more than 524280 rows")
        refused(call(args(min_weight=nan)), "min_weight must be a positive number")
        refused(call(args(min_weight=0.0)), "min_weight must be a positive number")
        refused(call(args(min_weight=inf)), "min_weight must be a positive number")
        refused(call(args(max_jump=nan)), "max_jump must be a non-negative number or inf")
        refused(call(args(max_jump=-0.5)), "max_jump must be a non-negative number or inf")
        refused(call(args(pin=(9.0, nan, 4.5, 2.5))), "pinhole[0] is not finite")
        refused(call(args(pin=(9.0, 9.5, inf, 2.5))), "pinhole[0] is not finite")
        refused(call(args(pin=(0.0, 9.5, 4.5, 2.5))), "pinhole[0] has a zero focal length")
        a = args()
        a.pinhole[1][1] = 0.0
        refused(call(a), "pinhole[1] has a zero focal length")
        for field in ("depth", "weights", "prior"):
            a = args()
            getattr(a, field)[1] = None
            refused(call(a), "null %s[1]" % field)
    refused(fwd(args(), loss=None), "null loss / count / stats")
    refused(fwd(args(), count=None), "null loss / count / stats")
    refused(fwd(args(), stats=None), "null loss / count / stats")
    refused(fwd(args(), ws=None), "needs a workspace of %d bytes" % need)
    refused(fwd(args(), ws_bytes=need - 1), "needs a workspace of %d bytes (got %d)" % (need, need - 1))
    refused(fwd(args(), ws=addr + 256 + 8), "not 16-byte aligned")
    refused(fwd(args(), stats=addr + 2180), "stats is not 8-byte aligned")
    refused(bwd(args(), stats=None), "null stats")
    refused(bwd(args(), stats=addr + 2180), "stats is not 8-byte aligned")
    refused(bwd(args(), g_loss=None), "null g_loss")
    # nothing wanted: a successful no-op that launches nothing; a mask is optional
    assert bwd(args(), g_depth=None, g_weights=None) == 0
    assert bwd(args(), g_depth=(_lib.c_fp * 16)(), g_weights=None) == 0
    a = args()
    a.mask[0] = None
    assert bwd(a, g_depth=None, g_weights=None) == 0
    op = "depth_to_normal"
    refused(d2n(H=0), "empty image", op)
    refused(d2n(H=1 << 16, W=1 << 15), "2^31 pixels", op)
    refused(d2n(min_weight=-1.0), "min_weight must be a positive number", op)
    refused(d2n(max_jump=nan), "max_jump must be a non-negative number or inf", op)
    refused(d2n(pin=None), "null pinhole", op)
    refused(d2n(pin=(9.0, 0.0, 4.5, 2.5)), "zero focal length", op)
    refused(d2n(pin=(nan, 9.0, 4.5, 2.5)), "is not finite", op)
    refused(d2n(depth=None), "null depth / weights", op)
    refused(d2n(weights=None), "null depth / weights", op)
    refused(d2n(normal=None), "null normal / valid", op)
    refused(d2n(valid=None), "null normal / valid", op)
