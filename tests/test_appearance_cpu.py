"""No-GPU checks of the appearance step (bags_raster/appearance.py, csrc/appearance.hip): the PyTorch statement against upstream's
literal one and against finite differences, the neutral row, the C ABI and every rejection of its entry points, the workspace
size, exposure.json, and the generators and conditioning of tests/appearance_cases.py."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import appearance_cases as A
import bags_raster
from bags_raster import AppearanceBank, _lib, appearance_torch, apply_appearance, load_exposure_json, save_exposure_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_appearance_forward", "bags_appearance_workspace_size", "bags_appearance_backward")
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the function
@pytest.mark.parametrize("center", (None, (4.3, 1.9)))
def test_formula_is_upstreams_exposure_on_the_vignetted_image(center):
    g = torch.Generator().manual_seed(3)
    H, W = 5, 7
    image = torch.rand(3, H, W, generator=g, dtype=F64)
    row = torch.randn(16, generator=g, dtype=F64)
    E, k = row[:12].reshape(3, 4), row[12:15]
    cx, cy = (W / 2, H / 2) if center is None else center
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    r2 = ((xs + 0.5 - cx) ** 2 + (ys + 0.5 - cy) ** 2) / ((W * W + H * H) / 4)
    f = 1 + k[0] * r2 + k[1] * r2 ** 2 + k[2] * r2 ** 3
    vignetted = f * image
    want = torch.matmul(vignetted.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]       # upstream, literally
    got = appearance_torch(image, row, center)
    assert got.shape == (3, H, W) and got.dtype == F64
    assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()
    if center is None:                                       # 0 at the centre, 1 at a corner
        assert r2.min().item() < 0.02 and abs(((0 - cx) ** 2 + (0 - cy) ** 2) / ((W * W + H * H) / 4) - 1) < 1e-15
    # the three forms of `images` are one function
    stack = torch.stack([image, 1 - image])
    rows = torch.stack([row, row.flip(0)])
    s = appearance_torch(stack, rows, center)
    q = appearance_torch([image, 1 - image], rows, center)
    assert torch.equal(s[0], got) and isinstance(q, list) and torch.equal(q[0], s[0]) and torch.equal(q[1], s[1])
    row2 = row.clone()
    row2[15] = float("nan")                                  # column 15 is never read
    assert torch.equal(appearance_torch(image, row2, center), got)


def test_gradcheck_in_float64():
    g = torch.Generator().manual_seed(4)
    images = torch.rand(2, 3, 5, 7, generator=g, dtype=F64, requires_grad=True)
    rows = (torch.tensor(bags_raster.appearance.NEUTRAL, dtype=F64) + 0.3 * torch.randn(2, 16, generator=g, dtype=F64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: appearance_torch(a, b, (3.1, 2.2)), (images, rows))
    assert torch.autograd.gradcheck(lambda a, b: appearance_torch(a, b), (images[0], rows[0]))


@pytest.mark.parametrize("dtype", (torch.float32, F64))
def test_neutral_row_returns_its_input_bit_for_bit(dtype):
    c = A.make_case(17, 67, 2)
    bank = AppearanceBank(A.N)
    assert len(bank) == A.N and tuple(bank.table.shape) == (A.N, 16) and isinstance(bank.table, torch.nn.Parameter)
    assert torch.equal(bank.exposure(3), torch.eye(3, 4)) and torch.equal(bank.vignetting(3), torch.zeros(3))
    assert bank.exposure(3).data_ptr() == bank.table[3].data_ptr() and bank.vignetting(3).data_ptr() == bank.table[3, 12:].data_ptr()
    img = c["images"].to(dtype)
    out = appearance_torch(img, bank.table.detach()[[5, 9]].to(dtype), c["center"])
    assert torch.equal(out, img)
    if dtype == torch.float32:                               # the bank on the host is appearance_torch
        assert torch.equal(bank.apply(img, [5, 9], c["center"]).detach(), img)
        assert torch.equal(bank.apply(img[0], 5).detach(), img[0])
        seq = bank.apply([img[0], img[1]], [5, 9])
        assert isinstance(seq, list) and torch.equal(seq[1].detach(), img[1])
        with torch.no_grad():
            bank.exposure(5)[0, 0] = 2.0                     # a view: the table is what changed
        assert bank.table[5, 0].item() == 2.0 and torch.equal(bank.apply(img[0], 5).detach()[0], 2 * img[0, 0])


def test_host_bank_trains_with_upstreams_one_adam():
    bank = AppearanceBank(4)
    opt = torch.optim.Adam([bank.table], lr=0.01)
    img = torch.rand(3, 6, 8)
    bank.apply(img, [2]).square().sum().backward()
    assert bank.table.grad[[0, 1, 3]].abs().max().item() == 0.0 and bank.table.grad[2, :15].abs().min().item() > 0.0
    assert bank.table.grad[2, 15].item() == 0.0
    before = bank.table.detach().clone()
    opt.step()
    moved = bank.table.detach() != before
    assert moved[2, :15].all() and not moved[2, 15] and not moved[[0, 1, 3]].any()


def test_wrapper_refuses_what_it_cannot_run():
    table = torch.tensor(bags_raster.appearance.NEUTRAL).repeat(3, 1)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        apply_appearance(torch.rand(3, 4, 4), table, [0])    # host tensors into the HIP path: refused, not copied
    with pytest.raises(ValueError, match="must be"):
        appearance_torch(torch.rand(4, 4), table[0])
    with pytest.raises(ValueError, match="one size"):
        appearance_torch([torch.rand(3, 4, 4), torch.rand(3, 4, 5)], table[:2])
    with pytest.raises(ValueError, match="table rows"):
        appearance_torch(torch.rand(2, 3, 4, 4), table)
    with pytest.raises(ValueError, match="listed twice"):
        AppearanceBank(3).apply(torch.rand(2, 3, 4, 4), [1, 1])
    with pytest.raises(ValueError, match=r"not in \[0, 3\)"):
        AppearanceBank(3).apply(torch.rand(3, 4, 4), [3])
    with pytest.raises(ValueError, match="no cameras"):
        AppearanceBank(0)


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
    assert [f[0] for f in _lib.BagsAppearance._fields_] == _header_struct_fields("BagsAppearance") == \
        ["N", "table", "n_rows", "rows", "C", "H", "W", "cx", "cy", "image", "out"]
    B = _lib.BagsAppearance
    assert (B.table.offset, B.n_rows.offset, B.rows.offset, B.C.offset, B.cx.offset, B.image.offset, B.out.offset) == (8, 16, 20, 84, 96, 104, 232)
    assert C.sizeof(B) == 360
    assert _lib.SYMBOLS["bags_appearance_forward"][1][-1] is C.c_void_p and _lib.SYMBOLS["bags_appearance_backward"][1][-1] is C.c_void_p
    for name, value in (("BLOCK", _lib.APPEARANCE_BLOCK), ("MIN_SLOTS", _lib.APPEARANCE_MIN_SLOTS), ("TILES_PER_SLOT", _lib.APPEARANCE_TILES_PER_SLOT)):
        assert re.search(r"#define BAGS_APPEARANCE_%s %d\b" % (name, value), header), name
    assert {"AppearanceBank", "apply_appearance", "appearance_torch", "save_exposure_json", "load_exposure_json"} <= set(bags_raster.__all__)
    assert "one ``torch.optim.Adam([bank.table]" in AppearanceBank.__doc__.replace("ONE", "one")
    makefile = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "build/appearance.o" in makefile and "EXTRA_appearance = -ffp-contract=off" in makefile


def test_workspace_size(lib):
    """Monotone in n_rows, a multiple of 16, one row of 16 doubles per workgroup; 0 for arguments the entries refuse."""
    size = lib.bags_appearance_workspace_size
    for H, W in A.SHAPES + ((1080, 1920),):
        sizes = [size(n, H, W) for n in range(1, 17)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
        assert all(s >= n * A.slots(H, W) * 128 for n, s in zip(range(1, 17), sizes))
        assert sizes[15] < 16 * A.slots(H, W) * 128 + 256
    assert A.slots(1, 1) == 1 and A.slots(17, 67) == 2 and A.slots(*A.STRIDED) == 64 < A.tiles(*A.STRIDED) and A.slots(1080, 1920) == 507
    assert size(0, 8, 8) == 0 and size(17, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 8, -1) == 0 and size(1, 1 << 16, 1 << 15) == 0


def test_every_rejection_is_reached_without_a_device(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 255) & ~255

    def args(N=23, n_rows=2, rows=(4, 1), Cn=3, H=6, W=10, **edit):
        a = _lib.BagsAppearance(N, addr, n_rows, (C.c_int32 * 16)(*rows), Cn, H, W, 5.0, 3.0,
                                (_lib.c_fp * 16)(*[addr] * max(0, min(n_rows, 16))), (_lib.c_fp * 16)(*[addr] * max(0, min(n_rows, 16))))
        for n, v in edit.items():
            setattr(a, n, v)
        return a

    ptrs = (_lib.c_fp * 16)(*[addr] * 16)
    need = lib.bags_appearance_workspace_size(2, 6, 10)

    def fwd(a):
        return lib.bags_appearance_forward(C.byref(a) if a is not None else None, None)

    def bwd(a, g_out=ptrs, ws=addr + 256, ws_bytes=None, g_image=ptrs, g_table=addr + 2048):
        return lib.bags_appearance_backward(C.byref(a) if a is not None else None, g_out, ws, need if ws_bytes is None else ws_bytes, g_image,
                                            g_table, None)

    def refused(rc, text):
        msg = lib.bags_last_error().decode()
        assert rc == -1 and "appearance" in msg and text in msg, (rc, msg)            # BAGS_ERR_ARG

    assert "BAGS_ERR_ARG = -1" in open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for call in (fwd, bwd):
        refused(call(None), "null struct")
        refused(call(args(table=None)), "null table")
        refused(call(args(N=0)), "N 0 < 1")
        refused(call(args(n_rows=0)), "n_rows 0 not in 1..16")
        refused(call(args(n_rows=17)), "n_rows 17 not in 1..16")
        refused(call(args(rows=(4, 23))), "rows[1] = 23 is not in [0, 23)")
        refused(call(args(rows=(-1, 2))), "rows[0] = -1")
        refused(call(args(rows=(4, 4))), "row 4 is listed twice")
        refused(call(args(H=0)), "empty image")
        refused(call(args(W=0)), "empty image")
        refused(call(args(H=-3)), "empty image")
        refused(call(args(Cn=4)), "C must be 3")
        refused(call(args(Cn=1)), "C must be 3")
        refused(call(args(H=1 << 16, W=1 << 15)), "2^31 pixels")
        refused(call(args(cx=float("nan"))), "centre is NaN")
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
    refused(bwd(args(), g_table=addr), "must not be the table")
    refused(bwd(args(), ws=None), "needs a workspace of %d bytes" % need)
    refused(bwd(args(), ws_bytes=need - 1), "needs a workspace of %d bytes (got %d)" % (need, need - 1))
    refused(bwd(args(), ws=addr + 256 + 8), "not 16-byte aligned")
    # nothing wanted: a successful no-op that needs no workspace and launches nothing
    assert bwd(args(), ws=None, ws_bytes=0, g_image=None, g_table=None) == 0
    assert bwd(args(), ws=None, ws_bytes=0, g_image=(_lib.c_fp * 16)(), g_table=None) == 0


# ---------------------------------------------------------------------------------------------------------------- exposure.json
def test_exposure_json_round_trips_bit_for_bit(tmp_path):
    g = torch.Generator().manual_seed(8)
    names = ["frame_%04d.jpg" % i for i in range(7)]
    bank = AppearanceBank(7)
    with torch.no_grad():
        bank.table[:, :15] += 0.3 * torch.randn(7, 15, generator=g)
        bank.table[2, 0] = 1.0 / 3.0
        bank.table[3, 7] = 1e-30
    path = str(tmp_path / "out" / "exposure.json")
    save_exposure_json(path, bank, names)
    plain = json.load(open(path))                            # what upstream reads: {image_name: 3x4 nested list}
    assert list(plain) == names and all(len(plain[n]) == 3 and all(len(r) == 4 for r in plain[n]) for n in names)
    assert torch.equal(torch.tensor(plain[names[4]], dtype=torch.float32), bank.exposure(4).detach())
    back = load_exposure_json(path, names)
    assert isinstance(back, AppearanceBank) and torch.equal(back.table[:, :12], bank.table[:, :12])
    assert back.table[:, 12:].abs().max().item() == 0.0      # the format has no field for k: state_dict carries it
    other = AppearanceBank(7)
    other.load_state_dict(bank.state_dict())
    assert torch.equal(other.table, bank.table)
    some = load_exposure_json(path, [names[5], names[0]])    # rows follow the names asked for
    assert torch.equal(some.exposure(0), bank.exposure(5)) and torch.equal(some.exposure(1), bank.exposure(0))
    with pytest.raises(KeyError, match="nobody"):
        load_exposure_json(path, ["nobody.jpg"])
    with pytest.raises(ValueError, match="image names"):
        save_exposure_json(path, bank, names[:3])


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_cases_are_what_the_gpu_tests_say_they_are():
    assert A.SHAPES[:5] == ((1, 1), (3, 5), (16, 64), (17, 67), (37, 259)) and A.VIEWS == (1, 2, 16, 17) and A.N == 23
    H, W = A.STRIDED
    assert H <= 160 and W <= 520 and W % 4 == 0 and A.tiles(H, W) > A.slots(H, W) > 1 and (H * W // 4) % A.QUADS_PER_TILE != 0
    assert A.tiles(17, 67) == 2 and (17 * 17) % A.QUADS_PER_TILE != 0          # more than one workgroup, the last one ragged
    for (H, W), V in (((37, 259), 17), (A.STRIDED, 2), ((3, 5), 16)):
        c = A.make_case(H, W, V)
        img, t = c["images"], c["table"]
        assert img.dtype == torch.float32 and (img > 1).any() and (img < 0).any() and ((img >= 0) & (img <= 1)).float().mean() > 0.9
        assert (t[:, :12] - torch.eye(3, 4).reshape(12)).abs().max() <= 0.3 and t[:, 12:15].abs().max() <= 0.5 and t[:, 15].isnan().all()
        assert len(set(c["rows"])) == V and (V == 1 or c["rows"] != sorted(c["rows"])) and all(0 <= r < A.N for r in c["rows"])
        assert (c["cot"] < 0).float().mean() > 0.2 and (c["cot"] > 0).float().mean() > 0.5
        assert A.make_case(H, W, V) is c and torch.equal(A.make_case.__wrapped__(H, W, V)["images"], img)       # seeded


@pytest.mark.parametrize("H,W", A.SHAPES)
def test_every_sum_of_every_case_is_well_conditioned(H, W):
    """|sum| >= 1e-3 * sum |terms| in float64 for each of the 15 sums of each view: the relative bars of the GPU tests are not
    vacuous.  The sums stated from the pieces of the formula are autograd's."""
    worst = 1.0
    for V in A.VIEWS:
        total, absum = A.term_sums(H, W, V)
        g_rows = A.reference(H, W, V)[2]
        assert ((total - g_rows)[:, A.USED].abs() <= 1e-12 * absum[:, A.USED]).all()
        ratio = (total.abs() / absum)[:, A.USED]
        worst = min(worst, float(ratio.min()))
        assert (ratio >= 1e-3).all(), (V, ratio.min())
        bar = A.bars(H, W, V)
        assert all(bool((b > 0).all()) for b in (bar[0], bar[1], bar[2][:, A.USED]))
    print("%dx%d: smallest |sum| / sum|terms| %.3g" % (H, W, worst))
