"""No-GPU checks of the depth prior (bags_raster/depth_prior.py, csrc/depth_prior.hip): the PyTorch statement against the closed
forms, that the bars of tests/depth_prior_cases.py reject wrong answers, the generator's conditions, the degenerate views in
float64, the C surface and every rejection of its entry points, and the chain test's threshold on the oracle's weights map."""
import ctypes as C
import os
import re

import pytest
import torch

import depth_prior_cases as P
import bags_raster
from bags_raster import DepthPriorBank, _lib, depth_prior_loss, depth_prior_loss_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_depth_prior_forward", "bags_depth_prior_workspace_size", "bags_depth_prior_backward")
F64 = torch.float64
COMBOS = [(m, s) for m in P.MODES for s in P.SPACES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _live(c):
    return [v for v in range(c["V"]) if v not in c["degenerate"]]


# ---------------------------------------------------------------------------------------------------------------- the function
@pytest.mark.parametrize("mode,space", COMBOS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=["%dx%d" % s for s in P.SHAPES])
def test_statement_equals_the_closed_forms(H, W, mode, space):
    """depth_prior_loss_torch in float64 with autograd against the closed forms of the loss and of every gradient: 1e-12 relative
    (to the largest magnitude of the tensor; exact zeros where the closed form has zeros)."""
    for V in (2, 17):
        c = P.make_case(H, W, V, mode, space)
        ref, want = P.reference(H, W, V, mode, space), P.closed_form(c)
        for name, a, b in zip(("loss", "dL/dD", "dL/dA", "dL/dtable"), ref[:4], want):
            assert (a is None) == (b is None), name
            if a is None:
                continue
            assert a.shape == b.shape and torch.isfinite(a).all(), name
            assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-300), name
            assert bool(((b == 0) <= (a == 0)).all()), name
        assert torch.equal(ref[4], P._pieces(c)["n"].float().double()) or (ref[4] - P._pieces(c)["n"]).abs().max() < 1e-12


@pytest.mark.parametrize("mode,space", COMBOS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=["%dx%d" % s for s in P.SHAPES])
def test_bars_reject_wrong_answers(H, W, mode, space):
    """The reference's own gradient with the rho (x - xbar) / Vx term dropped, with the sign of dx/dA flipped, and with 1/n
    replaced by 1 / (H W), is outside the bars on every non-degenerate case; the reference itself and the closed forms are inside."""
    for V in P.VIEWS:
        c = P.make_case(H, W, V, mode, space)
        if not _live(c):
            continue
        good = P.margins(H, W, V, mode, space, P.closed_form(c))
        assert all(m <= 1e-3 for m in good), good
        wrong = [("flip_dA", dict(flip_dA=True), 2), ("n_is_pixels", dict(n_is_pixels=True), 1)]
        if mode == "pearson":
            wrong.append(("drop_rho", dict(drop_rho=True), 1))
        for name, kw, which in wrong:
            m = P.margins(H, W, V, mode, space, P.closed_form(c, **kw))
            assert m[which] > 1.0, (name, V, m)
            if name == "n_is_pixels":
                assert m[2] > 1.0 and (mode != "l1" or m[3] > 1.0), (name, V, m)


@pytest.mark.parametrize("mode,space", COMBOS)
def test_generator_conditions_hold_on_every_case(mode, space):
    worst = dict(gap=1.0, valid=1.0, rmin=1.0, cond=1.0)
    for H, W in P.SHAPES:
        for V in P.VIEWS:
            c = P.make_case(H, W, V, mode, space)
            f = P.check_case(c)
            assert f == c["figures"]
            worst = {k: min(worst[k], f[k]) for k in worst}
            assert c["D"].dtype == torch.float32 and tuple(c["D"].shape) == (V, 1, H, W) == tuple(c["A"].shape)
            assert tuple(c["prior"].shape) == (V, H, W) == tuple(c["mask"].shape) and (c["mask"] >= 0).all()
            assert len(set(c["rows"])) == V and (V == 1 or c["rows"] != sorted(c["rows"])) and all(0 <= r < P.N for r in c["rows"])
            t = c["table"]
            assert tuple(t.shape) == (P.N, 2) and (t[:, 0] - 1).abs().max() <= 0.2 and t[:, 1].abs().max() <= 0.2
            assert V == 1 or ((c["cot"] > 0).any() and (c["cot"] < 0).any())
            if H * W >= 64:
                assert c["prior"].isnan().any() and (c["prior"] == 0).any() and (c["A"] < 0.4).any()
                assert (c["mask"] == 0).any() and ((c["mask"] > 0) & (c["mask"] < 1)).any()
                z = (c["D"] / c["A"])[c["A"] >= 0.55]
                assert z.min() >= 2 - 1e-5 and z.max() <= 5 + 1e-5
            assert P.make_case(H, W, V, mode, space) is c                                # cached
    print("\n%s %s: smallest |A - min_weight| %.3g, valid share %.3f, |r| %.3g, V / mean square %.3g" % (mode, space, *worst.values()))
    assert P.SHAPES[:5] == ((1, 1), (3, 5), (16, 64), (17, 67), (37, 259)) and P.VIEWS == (1, 2, 16, 17) and P.N == 23
    H, W = P.STRIDED
    assert H <= 160 and W <= 520 and W % 4 == 0 and P.tiles(H, W) > P.slots(H, W) > 1 and (H * W // 4) % P.QUADS_PER_TILE != 0
    assert P.tiles(17, 67) == 2


@pytest.mark.parametrize("mode,space", COMBOS)
def test_degenerate_views_in_float64(mode, space):
    """No valid pixel, one valid pixel, an exactly constant prior, an all-zero mask: pearson has loss 0 and all-zero gradients for
    all four, never NaN; l1 for the two without a valid pixel, and the loss of the one-pixel view is that pixel's |r|."""
    c = P.degenerate_case(mode, space)
    loss, gD, gA, g_rows, count = P.run_torch(c, F64)
    assert all(torch.isfinite(t).all() for t in (loss, gD, gA, count))
    k = P.DEGENERATE_VIEWS
    assert count[k["none_valid"]] == 0 and count[k["mask_zero"]] == 0 and count[k["one_valid"]] == 0.625 and count[k["constant_prior"]] > 100
    for v in c["degenerate"]:
        assert loss[v] == 0 and gD[v].abs().max() == 0 and gA[v].abs().max() == 0, v
        assert g_rows is None or g_rows[v].abs().max() == 0
    q = P._pieces(c)
    if mode == "pearson":
        v = k["constant_prior"]
        assert 0 <= abs(float(q["Vp"][v] / q["ep2"][v])) < 1e-14                         # far below the 1e-12 of the rule
    else:
        v = k["one_valid"]
        assert abs(float(loss[v]) - float(q["r"][v].abs()[q["valid"][v]])) < 1e-14
        assert gD[k["constant_prior"]].abs().max() > 0 and gD[v].abs().max() > 0
    for v in _live(c):
        assert loss[v] != 0 and gD[v].abs().max() > 0 and gA[v].abs().max() > 0
    # float32 takes the same branches
    l32 = P.run_torch(c, torch.float32)[0]
    assert all(l32[v] == 0 for v in c["degenerate"]) and all(l32[v] != 0 for v in _live(c))
    # the other views are the base case's, untouched
    base = P.make_case(17, 67, 16, mode, space)
    keep = [v for v in range(16) if v not in k.values()]
    assert all(torch.equal(c[n][keep], base[n][keep]) for n in ("D", "A", "mask")) and len(keep) == 12


def test_statement_dtype_forms_and_host_bank():
    c = P.make_case(16, 64, 2, "l1", "inverse")
    D, A, p, m = c["D"], c["A"], c["prior"], c["mask"]
    one = depth_prior_loss_torch(D[0], A[0], p[0], m[0], mode="l1", table=c["table"], rows=[c["rows"][0]])
    seq = depth_prior_loss_torch([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], [m[0], m[1]], mode="l1", table=c["table"], rows=c["rows"])
    assert one[0].shape == (1,) and seq[0].shape == (2,) and one[0].dtype == torch.float32 and torch.equal(one[0], seq[0][:1])
    assert torch.equal(one[1], seq[1][:1])
    # (H,W) maps, a None mask entry and no mask at all
    a = depth_prior_loss_torch(D[0, 0], A[0, 0], p[0][None], None)
    b = depth_prior_loss_torch([D[0]], [A[0]], [p[0]], [None])
    assert torch.equal(a[0], b[0]) and a[1].item() == float(((A[0, 0] >= 0.5) & (p[0] > 0)).sum())
    # no table: (a, b) = (1, 0)
    t = torch.tensor((1.0, 0.0)).repeat(3, 1)
    assert torch.equal(depth_prior_loss_torch(D[0], A[0], p[0], m[0], mode="l1")[0],
                       depth_prior_loss_torch(D[0], A[0], p[0], m[0], mode="l1", table=t, rows=[2])[0])
    # pearson does not see scale or shift of the prior
    l0 = depth_prior_loss_torch(D[0].double(), A[0].double(), p[0].double(), m[0].double())[0]
    moved = torch.where(p[0] > 0, 3.0 * p[0].double() + 0.25, p[0].double())            # (a prior of 0 or NaN stays "no prior here")
    l1 = depth_prior_loss_torch(D[0].double(), A[0].double(), moved, m[0].double())[0]
    assert abs(float(l0 - l1)) < 1e-12 and 0 < float(l0) < 1
    bank = DepthPriorBank(P.N)
    assert len(bank) == P.N and isinstance(bank.table, torch.nn.Parameter) and torch.equal(bank.table.detach(), torch.tensor((1.0, 0.0)).repeat(P.N, 1))
    with torch.no_grad():
        bank.table.copy_(c["table"])
    loss, count = bank.loss([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], c["rows"], [m[0], m[1]])
    assert torch.equal(loss.detach(), seq[0]) and torch.equal(count, seq[1])
    opt = torch.optim.Adam([bank.table], lr=0.01)
    loss.sum().backward()
    before = bank.table.detach().clone()
    opt.step()
    moved = (bank.table.detach() != before).any(1)
    assert moved[c["rows"]].all() and int(moved.sum()) == 2
    assert bank.loss(D[0], A[0], p[0], 3, mode="pearson")[0].item() == depth_prior_loss_torch(D[0], A[0], p[0])[0].item()


def test_wrapper_refuses_what_it_cannot_run():
    c = P.make_case(3, 5, 2, "l1", "depth")
    D, A, p, m = c["D"], c["A"], c["prior"], c["mask"]
    with pytest.raises(RuntimeError, match="AMD GPU"):
        depth_prior_loss(D[0], A[0], p[0])                   # host tensors into the HIP path: refused, not copied
    for fn in (depth_prior_loss, depth_prior_loss_torch):
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            fn(D[0], A[0], p[0], m[0] > 0)
        with pytest.raises(ValueError, match="pearson"):
            fn(D[0], A[0], p[0], table=c["table"], rows=[0])
        with pytest.raises(ValueError, match="mode must be"):
            fn(D[0], A[0], p[0], mode="l2")
        with pytest.raises(ValueError, match="space must be"):
            fn(D[0], A[0], p[0], space="disparity")
        with pytest.raises(ValueError, match="one size"):
            fn(D[0], A[0], torch.rand(3, 6))
        with pytest.raises(ValueError, match="2 depth maps but 1 prior"):
            fn([D[0], D[1]], [A[0], A[1]], [p[0]])
        with pytest.raises(ValueError, match="listed twice"):
            fn([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], mode="l1", table=c["table"], rows=[4, 4])
        with pytest.raises(ValueError, match=r"not in \[0, 23\)"):
            fn(D[0], A[0], p[0], mode="l1", table=c["table"], rows=[23])
        with pytest.raises(ValueError, match="needs rows"):
            fn(D[0], A[0], p[0], mode="l1", table=c["table"])
        with pytest.raises(ValueError, match="rows without a table"):
            fn(D[0], A[0], p[0], mode="l1", rows=[1])
        with pytest.raises(ValueError, match="must be a non-empty"):
            fn(torch.rand(2, 3, 5), A[0], p[0])
    with pytest.raises(ValueError, match="no images"):
        DepthPriorBank(0)
    with pytest.raises(ValueError, match="listed twice"):
        DepthPriorBank(3).loss([D[0], D[1]], [A[0], A[1]], [p[0], p[1]], [1, 1])


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
        if name != "bags_depth_prior_workspace_size":                                    # the stream comes last
            assert decl.rstrip().endswith("void* stream") and _lib.SYMBOLS[name][1][-1] is C.c_void_p, name
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert [f[0] for f in _lib.BagsDepthPrior._fields_] == _header_struct_fields("BagsDepthPrior") == \
        ["mode", "space", "H", "W", "min_weight", "n_rows", "N", "reserved", "table", "rows", "depth", "weights", "prior", "mask"]
    B = _lib.BagsDepthPrior
    assert (B.H.offset, B.min_weight.offset, B.N.offset, B.table.offset, B.rows.offset, B.depth.offset, B.mask.offset) == (8, 16, 24, 32, 40, 104, 488)
    assert C.sizeof(B) == 616
    for name, value in (("BLOCK", _lib.DEPTH_PRIOR_BLOCK), ("MIN_SLOTS", _lib.DEPTH_PRIOR_MIN_SLOTS), ("TILES_PER_SLOT", _lib.DEPTH_PRIOR_TILES_PER_SLOT),
                        ("STATS", _lib.DEPTH_PRIOR_STATS), ("PEARSON", _lib.DEPTH_PRIOR_PEARSON), ("L1", _lib.DEPTH_PRIOR_L1),
                        ("DEPTH", _lib.DEPTH_PRIOR_DEPTH), ("INVERSE", _lib.DEPTH_PRIOR_INVERSE)):
        assert re.search(r"#define BAGS_DEPTH_PRIOR_%s %d\b" % (name, value), header), name
    assert {"DepthPriorBank", "depth_prior_loss", "depth_prior_loss_torch"} <= set(bags_raster.__all__)
    assert all(hasattr(bags_raster, n) for n in ("DepthPriorBank", "depth_prior_loss", "depth_prior_loss_torch"))
    makefile = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "build/depth_prior.o" in makefile and "EXTRA_depth_prior = -ffp-contract=off" in makefile


def test_workspace_size(lib):
    """Monotone in n_rows, a multiple of 16, one row of 8 doubles per workgroup; 0 for arguments the entries refuse."""
    size = lib.bags_depth_prior_workspace_size
    for H, W in P.SHAPES + ((1080, 1920),):
        sizes = [size(n, H, W) for n in range(1, 17)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
        assert all(s >= n * P.slots(H, W) * 64 for n, s in zip(range(1, 17), sizes))
        assert sizes[15] < 16 * P.slots(H, W) * 64 + 256
    assert P.slots(1, 1) == 1 and P.slots(17, 67) == 2 and P.slots(*P.STRIDED) == 64 < P.tiles(*P.STRIDED) and P.slots(1080, 1920) == 507
    assert size(0, 8, 8) == 0 and size(17, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 8, -1) == 0 and size(1, 1 << 16, 1 << 15) == 0


def test_every_rejection_is_reached_without_a_device(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 8192)()
    addr = (C.addressof(buf) + 255) & ~255
    L1, PEARSON = _lib.DEPTH_PRIOR_L1, _lib.DEPTH_PRIOR_PEARSON

    def args(mode=L1, space=1, H=6, W=10, n_rows=2, N=23, table=addr, rows=(4, 1), **edit):
        k = max(0, min(n_rows, 16))
        a = _lib.BagsDepthPrior(mode, space, H, W, 0.5, n_rows, N, 0, table, (C.c_int32 * 16)(*rows), (_lib.c_fp * 16)(*[addr] * k),
                                (_lib.c_fp * 16)(*[addr] * k), (_lib.c_fp * 16)(*[addr] * k), (_lib.c_fp * 16)(*[addr] * k))
        for n, v in edit.items():
            setattr(a, n, v)
        return a

    ptrs = (_lib.c_fp * 16)(*[addr] * 16)
    need = lib.bags_depth_prior_workspace_size(2, 6, 10)

    def fwd(a, ws=addr + 256, ws_bytes=None, loss=addr + 2048, count=addr + 2112, stats=addr + 2176):
        return lib.bags_depth_prior_forward(C.byref(a) if a is not None else None, ws, need if ws_bytes is None else ws_bytes, loss, count, stats, None)

    def bwd(a, stats=addr + 2176, g_loss=addr + 2048, g_depth=ptrs, g_weights=ptrs, g_table=addr + 4096):
        return lib.bags_depth_prior_backward(C.byref(a) if a is not None else None, stats, g_loss, g_depth, g_weights, g_table, None)

    def refused(rc, text):
        msg = lib.bags_last_error().decode()
        assert rc == -1 and "depth_prior" in msg and text in msg, (rc, msg)                # BAGS_ERR_ARG

    assert "BAGS_ERR_ARG = -1" in open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for call in (fwd, bwd):
        refused(call(None), "null struct")
        refused(call(args(mode=2)), "unknown mode 2")
        refused(call(args(space=-1)), "unknown space -1")
        refused(call(args(mode=PEARSON)), "a table with the pearson mode")
        refused(call(args(N=0)), "N 0 < 1")
        refused(call(args(n_rows=0)), "n_rows 0 not in 1..16")
        refused(call(args(n_rows=17)), "n_rows 17 not in 1..16")
        refused(call(args(n_rows=0, table=None)), "n_rows 0 not in 1..16")
        refused(call(args(n_rows=17, table=None, mode=PEARSON)), "n_rows 17 not in 1..16")
        refused(call(args(rows=(4, 23))), "rows[1] = 23 is not in [0, 23)")
        refused(call(args(rows=(-1, 2))), "rows[0] = -1")
        refused(call(args(rows=(4, 4))), "row 4 is listed twice")
        refused(call(args(H=0)), "empty image")
        refused(call(args(W=-2)), "empty image")
        refused(call(args(H=1 << 16, W=1 << 15)), "2^31 pixels")
        refused(call(args(min_weight=float("nan"))), "min_weight is NaN")
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
    refused(bwd(args(), g_loss=None), "null g_loss")
    refused(bwd(args(table=None)), "no table was given")
    refused(bwd(args(), g_table=addr), "must not be the table")
    # nothing wanted: a successful no-op that launches nothing; a mask is optional
    assert bwd(args(), g_depth=None, g_weights=None, g_table=None) == 0
    assert bwd(args(), g_depth=(_lib.c_fp * 16)(), g_weights=None, g_table=None) == 0
    a = args()
    a.mask[0] = None
    assert bwd(a, g_depth=None, g_weights=None, g_table=None) == 0


# ---------------------------------------------------------------------------------------------------------------- the chain's scene
def test_chain_scene_threshold_on_the_oracle():
    """The scene of the GPU chain test through the CPU oracle's forward: with min_weight = P.CHAIN_MIN_WEIGHT at least a quarter of the
    pixels are valid (weights >= min_weight and depth > 0) and no weight is within 1e-3 of the threshold."""
    from depth_oracle import forward, leaves_of, oracle_inputs
    from scenes import make_case, oracle_settings
    scene, cam = make_case(24, 32, 32, 3.0, 1, seed=5, dist=3.0)
    leaf, s2 = leaves_of(oracle_inputs(scene), oracle_settings(cam, 1), torch.float32, want=False)
    st = forward(leaf, s2, torch.float32)
    A, D = st.weights[0], st.depth_img[0]
    valid = (A >= P.CHAIN_MIN_WEIGHT) & (D > 0)
    print("\nchain scene: valid share %.3f, smallest |A - min_weight| %.3g" % (valid.float().mean(), (A - P.CHAIN_MIN_WEIGHT).abs().min()))
    assert valid.float().mean() >= 0.25 and (A - P.CHAIN_MIN_WEIGHT).abs().min() >= 1e-3
