"""CPU checks of bags_raster.gaussian_normals: the PyTorch statements (float32 and float64) against independent float64 lines
written with build_rotation, F.normalize and torch.where on the named cases of tests/gaussian_normals_cases.py; gradcheck; the
argument errors of the Python names; the C entries' validation through the library, without a GPU."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import gaussian_normals_cases as K
from bags_raster import (_lib, gaussian_normals, gaussian_normals_torch, gaussian_normals_views, gaussian_normals_views_torch)

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def build_rotation(r):
    """3DGS's utils/general_utils.py build_rotation: R of the NORMALISED quaternion (w,x,y,z)."""
    q = r / r.norm(dim=1, keepdim=True)
    R = torch.zeros(q.shape[0], 3, 3, dtype=r.dtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def independent(name, v=0):
    """(normals (P,3) float64, usable (P,) bool): the recipe as a user writes it today."""
    c = K.case(name)
    q, x, V = c["rotations"].double(), c["means3D"].double(), c["views"][v].double()
    usable = torch.isfinite(q).all(1) & (q.norm(dim=1) > 0)
    R = build_rotation(torch.where(usable[:, None], q, torch.tensor([1.0, 0, 0, 0], dtype=F64)))
    k = K.first_minimum(c["scales"])
    axis = R[torch.arange(q.shape[0]), :, k]
    n = F.normalize(axis @ V[:3, :3], dim=1)
    t = x @ V[:3, :3] + V[3, :3]
    return torch.where(((n * t).sum(1) > 0)[:, None], -n, n), usable


@pytest.mark.parametrize("name", K.CASES)
def test_the_statements_against_independent_lines(name):
    """float64 statement: 1e-12 of the independent lines; float32 statement: the project's forward bar 1e-5 (1 + |x|).  `grazing`:
    without the rows whose sigma differs between the two statements; `dead`: without the dead rows, which are zeros in float32."""
    c = K.case(name)
    ref, usable = independent(name)
    o64 = gaussian_normals_torch(c["rotations"].double(), c["scales"].double(), c["means3D"].double(), c["views"][0].double())
    o32 = gaussian_normals_torch(c["rotations"], c["scales"], c["means3D"], c["views"][0])
    assert o32.dtype == F32 and o64.dtype == F64 and o32.shape == (K.P_FULL, 3)
    assert not torch.isnan(o32).any() and not torch.isnan(o64).any()
    keep = usable.clone()
    if name == "dead":
        keep &= ~K.dead_rows()
        assert (o32[K.dead_rows()] == 0).all() and (o64[~usable] == 0).all()
    e64 = (o64 - ref).abs()[keep].max().item()
    if name == "grazing":
        keep &= ~K.sigma_flips(name)
    e32 = ((o32.double() - ref).abs() / (1 + ref.abs()))[keep].max().item()
    print("\n%s: |f64 - independent| %.2e   |f32 - independent| / (1 + |x|) %.2e on %d rows" % (name, e64, e32, int(keep.sum())))
    assert e64 <= 1e-12 and e32 <= 1e-5
    assert ((o32.norm(dim=1) - 1).abs()[keep] <= 1e-6).all()
    # the normal faces the camera
    t = c["means3D"].double() @ c["views"][0].double()[:3, :3] + c["views"][0].double()[3, :3]
    assert ((o64 * t).sum(1)[keep] <= 0).all()


def test_the_views_statement_is_the_single_view_statement_per_view():
    c = K.case("scaled_view")
    outs = gaussian_normals_views_torch(c["rotations"], c["scales"], c["means3D"], c["views"])
    assert len(outs) == K.MAX_VIEWS
    for v in (0, 3, 16):
        assert torch.equal(outs[v], gaussian_normals_torch(c["rotations"], c["scales"], c["means3D"], c["views"][v]))
        ref, _ = independent("scaled_view", v)
        assert (outs[v].double() - ref).abs().max().item() <= 1e-5


def test_a_scale_on_the_view_block_cancels():
    g, s = K.case("generic"), K.case("scaled_view")
    assert torch.equal(g["rotations"], s["rotations"]) and torch.equal(g["scales"], s["scales"])
    a = gaussian_normals_torch(g["rotations"].double(), g["scales"].double(), g["means3D"].double(), g["views"][0].double())
    V = g["views"][0].double().clone()
    V[:3, :3] *= 1.7
    b = gaussian_normals_torch(g["rotations"].double(), g["scales"].double(), g["means3D"].double(), V)
    flip = (a * b).sum(1) < 0                              # the translation did not scale: t moved, sigma may differ
    assert (torch.where(flip[:, None], -b, b) - a).abs().max().item() <= 1e-12


def test_log_scales_and_ties():
    g, l, t = K.case("generic"), K.case("log_scales"), K.case("ties")
    assert torch.equal(gaussian_normals_torch(l["rotations"], l["scales"], l["means3D"], l["views"][0]),
                       gaussian_normals_torch(g["rotations"], g["scales"], g["means3D"], g["views"][0]))
    s = t["scales"]
    tied = (s[:, 0] == s[:, 1]) | (s[:, 1] == s[:, 2]) | (s[:, 0] == s[:, 2])
    assert int(tied.sum()) >= K.P_FULL // 3
    k = K.first_minimum(s)
    assert set(k[tied].tolist()) == {0, 1, 2}
    from bags_raster.gaussian_normals import _axis_torch
    assert torch.equal(_axis_torch(t["rotations"], s)[1], k)
    two_min = (s[:, 0] == s[:, 1]) & (s[:, 0] < s[:, 2])
    assert int(two_min.sum()) > 100 and (k[two_min] == 0).all()
    assert (k[(s[:, 0] == s[:, 1]) & (s[:, 1] == s[:, 2])] == 0).all()


def test_grazing_flips_stay_under_the_cap():
    """The two statements alone: sigma differs between float32 and float64 on at most P_FULL // 100 rows of `grazing` with
    |mh . th| uniform in [-1e-3, 1e-3] (the interval of the issue; it did not have to be widened).  No other case has a flip."""
    n = int(K.sigma_flips("grazing").sum())
    print("\ngrazing: %d rows of %d flip sigma between float32 and float64" % (n, K.P_FULL))
    assert n <= K.P_FULL // 100
    for name in ("generic", "scaled_view", "disks", "ties"):
        assert int(K.sigma_flips(name).sum()) == 0, name


def test_gradcheck_on_eight_rows():
    c = K.case("generic")
    s, x = c["scales"][:8].double(), c["means3D"][:8].double()
    q = c["rotations"][:8].double().requires_grad_()
    Va, Vb = c["views"][0].double().requires_grad_(), K.case("scaled_view")["views"][2].double().requires_grad_()
    assert torch.autograd.gradcheck(lambda q, Va, Vb: gaussian_normals_views_torch(q, s, x, [Va, Vb]), (q, Va, Vb))


@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
@pytest.mark.parametrize("zero_block", (False, True), ids=("rigid", "zero_block"))
def test_dead_rows_give_zeros_and_no_nan(dtype, zero_block):
    outs, grads = K.forward_backward(gaussian_normals_views_torch, "dead", dtype, "cpu", V=2, zero_block=zero_block)
    dead = torch.ones(K.P_FULL, dtype=torch.bool) if zero_block else (K.dead_rows() if dtype == F32 else torch.arange(K.P_FULL) % 37 <= 1)
    for o in outs:
        assert (o[dead] == 0).all() and not torch.isnan(o).any()
    assert (grads["rotations"][dead] == 0).all()
    for n, g in grads.items():
        assert torch.isfinite(g).all(), n
    for v in range(2):
        gv = grads["view%d" % v]
        assert (gv[3] == 0).all() and (gv[:, 3] == 0).all()
        assert (gv == 0).all() if zero_block else gv[:3, :3].abs().max() > 0


def test_argument_errors():
    c = K.case("generic")
    q, s, x, V = c["rotations"], c["scales"], c["means3D"], c["views"][0]
    for fn in (gaussian_normals_views_torch, gaussian_normals_views):
        with pytest.raises(ValueError):
            fn(q[:, :3], s, x, [V])
        with pytest.raises(ValueError):
            fn(q, s[:-1], x, [V])
        with pytest.raises(ValueError):
            fn(q, s, x[:, :2], [V])
        with pytest.raises(ValueError):
            fn(q, s, x, [V[:3]])
        with pytest.raises(ValueError):
            fn(q, s, x, [])
        with pytest.raises(TypeError):
            fn(q, s, x, V)                                  # a tensor where the list of views goes
    with pytest.raises(TypeError):
        gaussian_normals_torch(q, s, x, [V])
    # the HIP names take GPU tensors: no CPU fallback behind them
    with pytest.raises(RuntimeError, match="AMD GPU"):
        gaussian_normals(q, s, x, V)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        gaussian_normals_views(q, s, x, [V, V])


def test_the_c_entries_validate_their_arguments(lib):
    """Reported before anything is enqueued: no GPU touched.  Host addresses stand in for device pointers; validation never
    dereferences them."""
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)
    views = lambda n: (_lib.c_fp * _lib.MAX_SH_VIEWS)(*([addr] * n + [None] * (_lib.MAX_SH_VIEWS - n)))       # noqa: E731
    table = lambda n: (_lib.c_fp * _lib.MAX_SH_VIEWS)(*([addr] * n + [None] * (_lib.MAX_SH_VIEWS - n)))       # noqa: E731
    err = lambda: lib.bags_last_error()                                                                       # noqa: E731
    assert C.sizeof(_lib.BagsGaussianNormals) == 8 + 3 * 8 + 16 * 8
    ok = _lib.BagsGaussianNormals(100, 2, addr, addr, addr, views(2))
    for V in (0, -1, _lib.MAX_SH_VIEWS + 1):
        a = _lib.BagsGaussianNormals(100, V, addr, addr, addr, views(16))
        assert lib.bags_gaussian_normals_forward(C.byref(a), table(16), None) == -1 and b"V %d not in 1..16" % V in err()
        assert lib.bags_gaussian_normals_backward(C.byref(a), table(16), None, 0, addr, table(16), None) == -1 and b"not in 1..16" in err()
        assert lib.bags_gaussian_normals_workspace_size(100, V) == 0
    a = _lib.BagsGaussianNormals(-1, 1, addr, addr, addr, views(1))
    assert lib.bags_gaussian_normals_forward(C.byref(a), table(1), None) == -1 and b"P < 0" in err()
    assert lib.bags_gaussian_normals_forward(None, table(1), None) == -1 and b"null struct" in err()
    for field in ("rotations", "scales", "means3D"):
        a = _lib.BagsGaussianNormals(100, 2, addr, addr, addr, views(2))
        setattr(a, field, None)
        assert lib.bags_gaussian_normals_forward(C.byref(a), table(2), None) == -1 and b"NULL rotations / scales / means3D" in err()
    # fewer pointers than V says: view 1 is missing (in the struct, in the output table, in the cotangent table)
    a = _lib.BagsGaussianNormals(100, 2, addr, addr, addr, views(1))
    assert lib.bags_gaussian_normals_forward(C.byref(a), table(2), None) == -1 and b"viewmatrix[1] is NULL" in err()
    assert lib.bags_gaussian_normals_forward(C.byref(ok), table(1), None) == -1 and b"out[1] is NULL" in err()
    assert lib.bags_gaussian_normals_forward(C.byref(ok), None, None) == -1 and b"null out table" in err()
    assert lib.bags_gaussian_normals_backward(C.byref(ok), None, None, 0, addr, None, None) == -1 and b"null grad_out table" in err()
    # the view-matrix gradients need the workspace
    need = lib.bags_gaussian_normals_workspace_size(100, 2)
    assert need >= 9 * 2 * 4 and lib.bags_gaussian_normals_workspace_size(100_000, 16) >= 391 * 9 * 16 * 4
    assert lib.bags_gaussian_normals_workspace_size(1000, 2) < lib.bags_gaussian_normals_workspace_size(100_000, 2)
    assert lib.bags_gaussian_normals_backward(C.byref(ok), table(2), None, 0, addr, table(2), None) == -3 and b"workspace" in err()
    assert lib.bags_gaussian_normals_backward(C.byref(ok), table(2), addr, need - 1, None, table(1), None) == -3
    # nothing wanted, and an empty set: successful no-ops
    assert lib.bags_gaussian_normals_backward(C.byref(ok), table(2), None, 0, None, None, None) == 0
    empty = _lib.BagsGaussianNormals(0, 1, None, None, None, views(0))
    assert lib.bags_gaussian_normals_forward(C.byref(empty), None, None) == 0
    assert lib.bags_gaussian_normals_backward(C.byref(empty), None, None, 0, None, None, None) == 0
