"""No-GPU checks of Mip-Splatting's 3D smoothing filter (bags_raster/filter3d.py, csrc/filter3d.hip, the filtered instance of
csrc/activations.hip): the named cases of tests/filter3d_cases.py against what they claim to contain, the float32 statement against
float64, the filtered activations against a derivative written out by hand, the host path of GaussianBag, and the C ABI surface."""
import ctypes as C
import os
import re

import pytest
import torch

import bags_raster
import filter3d_cases as F
from bags_raster import GaussianBag, PipelineParams, _lib, filter_3D, filter_3D_torch, filtered_activations_torch
from bags_raster.synth import synth_scene
from scenes import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_filter3d_compute", "bags_activations_filtered_forward", "bags_activations_filtered_backward")
F32, F64 = torch.float32, torch.float64
CASE_N = [(name, N) for name in F.CASES for N in F.NS]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the cases
@pytest.mark.parametrize("name,N", CASE_N)
def test_cases_keep_the_decision_margin_and_the_flip_cap(name, N):
    xyz = F.points(name, N)
    P = xyz.shape[0]
    assert xyz.dtype == F32 and P == (F.P_MAX_ROW if name.startswith("max_") else F.P_FULL)
    assert F.margins(xyz, N).min().item() >= F.MARGIN
    n_flips = int(F.flips(name, N).sum())
    print(name, N, "flips", n_flips)
    assert n_flips <= P // 100


@pytest.mark.parametrize("N", F.NS)
def test_cases_contain_what_they_claim(N):
    V, K, wh = F.table(N)
    ring = F.decisions("ring", N, F64)
    assert ring["any"].sum().item() >= 0.5 * F.P_FULL
    if N > 1:
        assert ring["argfocal"] != 0 and len({tuple(r) for r in wh.tolist()}) > 1           # `focal` is not camera 0's; mixed sizes
    behind = F.decisions("behind", N, F64)
    hidden = int((~behind["any"]).sum())
    assert 0.12 * F.P_FULL <= hidden <= (0.6 if N == 1 else 0.3) * F.P_FULL, hidden
    assert not behind["any"][1] and not behind["any"][3]                                    # rows 1 and 3: sentinel rows at every size
    assert not F.decisions("none_valid", N, F64)["any"].any()
    # edge: rows within 2.5 % of each of the five thresholds of the cameras present, on both sides
    xyz = F.points("edge", N).double()
    v, k = V.double().reshape(-1, 16), K.double().reshape(-1, 16)
    W, H = wh.double().unbind(1)
    t = [xyz[:, 0:1] * v[:, a] + xyz[:, 1:2] * v[:, 4 + a] + xyz[:, 2:3] * v[:, 8 + a] + v[:, 12 + a] for a in range(3)]
    px, py = t[0] / t[2] * (k[:, 0] * 0.5 * W) + 0.5 * W, t[1] / t[2] * (k[:, 5] * 0.5 * H) + 0.5 * H
    front = t[2] > 0.2
    for i, signed in enumerate((t[2] - 0.2, px / W + 0.15, px / W - 1.15, py / H + 0.15, py / H - 1.15)):
        near = (signed.abs() <= 0.025) & (front if i else torch.ones_like(front))
        assert int((near & (signed > 0)).any(dim=1).sum()) >= 15 and int((near & (signed < 0)).any(dim=1).sum()) >= 15
    for name, row in (("max_last", F.P_MAX_ROW - 1), ("max_first", 0)):
        d = F.decisions(name, N, F64)
        dist = torch.where(d["any"], d["dist"], torch.full_like(d["dist"], -1.0))
        assert int(dist.argmax()) == row and d["any"][row] and int((dist == dist[row]).sum()) == 1
        assert row // F.BLOCK == (2 if name == "max_last" else 0)


def test_sizes_sit_on_the_block_edges():
    src = open(os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc", "filter3d.hip")).read()
    assert "#define F3_BLOCK %d" % F.BLOCK in src
    assert F.SIZES == (1, 255, 256, 257, 513, 1000) and F.NS == (1, 3, 17, 70) and F.P_MAX_ROW == 513


# ---------------------------------------------------------------------------------------------------------------- 2. the statement
@pytest.mark.parametrize("name,N", CASE_N)
def test_float32_statement_against_float64(name, N):
    for P in F.sizes_of(name):
        o32, o64 = F.reference(name, N, F32, P), F.reference(name, N, F64, P)
        assert o32.shape == (P, 1) and o32.dtype == F32 and o64.dtype == F64 and not o32.requires_grad
        keep = ~F.flips(name, N, P)
        err = (o32.double() - o64).abs()[keep]
        assert (err <= 1e-5 * (1 + o64.abs()[keep])).all(), (P, err.max().item())
        assert torch.isfinite(o32).all() and (o32 > 0).all()


@pytest.mark.parametrize("N", F.NS)
def test_rows_no_camera_sees(N):
    """`none_valid`: every output is 100000 / focal * sqrt(variance); `behind`: the hidden rows all carry dmax, the largest valid dist."""
    for dtype in (F32, F64):
        d = F.decisions("none_valid", N, dtype)
        want = (torch.tensor(100000.0, dtype=dtype) / d["focal"]) * torch.sqrt(torch.tensor(F.VARIANCE, dtype=dtype).double()).to(dtype)
        assert torch.equal(F.reference("none_valid", N, dtype), want.expand(F.P_FULL, 1))
        d = F.decisions("behind", N, dtype)
        out = F.reference("behind", N, dtype)
        dmax = d["dist"][d["any"]].max()
        sv = torch.sqrt(torch.tensor(F.VARIANCE, dtype=dtype).double()).to(dtype)
        assert torch.equal(out[~d["any"]], ((dmax / d["focal"]) * sv).expand(int((~d["any"]).sum()), 1))
        assert (out[d["any"]] <= out[~d["any"]][0]).all()


def test_statement_arguments():
    V, K, wh = F.table(3)
    xyz = F.points("ring", 3)[:5]
    with pytest.raises(ValueError, match="at least one camera"):
        filter_3D_torch(xyz, V[:0], K[:0], wh[:0])
    for bad in (dict(xyz=xyz[:, :2]), dict(xyz=xyz.reshape(-1)), dict(viewmatrices=V.reshape(3, 16)), dict(intrinsics=K[:2]), dict(sizes=wh[:2]),
                dict(sizes=wh.reshape(-1)), dict(sizes=wh.float()), dict(variance=-1.0)):
        a = dict(xyz=xyz, viewmatrices=V, intrinsics=K, sizes=wh, variance=0.2)
        a.update(bad)
        with pytest.raises(ValueError, match="filter_3D_torch"):
            filter_3D_torch(**a)
    assert filter_3D_torch(xyz[:0], V, K, wh).shape == (0, 1)
    assert filter_3D_torch(xyz.double().requires_grad_(True), V, K, wh).requires_grad is False
    assert torch.equal(filter_3D_torch(xyz, V, K, wh.long()), filter_3D_torch(xyz, V, K, wh))
    # the variance is a plain factor sqrt(variance)
    a, b = filter_3D_torch(xyz.double(), V, K, wh, 0.2), filter_3D_torch(xyz.double(), V, K, wh, 0.8)
    assert torch.allclose(b, 2.0 * a, rtol=1e-14, atol=0.0)
    with pytest.raises(NotImplementedError, match="filter_3D runs only on an AMD GPU.*filter_3D_torch"):
        filter_3D(xyz, V, K, wh)


# ---------------------------------------------------------------------------------------------------------------- 3. the activations
@pytest.mark.parametrize("kind", F.FILTERS)
@pytest.mark.parametrize("which", F.COTANGENTS)
def test_filtered_activations_against_the_derivative_by_hand(kind, which):
    P = 257
    r, f, ct = F.raw(P), F.filter_values(kind, P), F.cotangents(P)
    o_raw = r["opacity"].double().requires_grad_(True)
    s_raw = r["scaling"].double().requires_grad_(True)
    fd = f.double().requires_grad_(True)
    op, sc = filtered_activations_torch(o_raw, s_raw, fd)
    want = F.by_hand_f64(kind, P, which)
    assert op.shape == (P, 1) and sc.shape == (P, 3)
    assert (op - want[0]).abs().max().item() <= 1e-12 and rel_err(sc, want[1]) <= 1e-14
    loss = (op * ct["opacity"]).sum() * (which != "scales") + (sc * ct["scales"]).sum() * (which != "opacity")
    loss.backward()
    assert rel_err(o_raw.grad, want[2]) <= 1e-10 if which != "scales" else o_raw.grad.abs().max().item() == 0.0
    assert rel_err(s_raw.grad, want[3]) <= 1e-10
    assert fd.grad is None                                            # not differentiable in the filter
    if kind == "zero":                                                # f = 0: the plain activations
        assert rel_err(op, torch.sigmoid(o_raw)) <= 1e-15 and rel_err(sc, torch.exp(s_raw)) <= 1e-15
    if kind == "huge":
        assert op.max().item() < 1e-6 and (sc.detach() >= 1e3).all()


# ---------------------------------------------------------------------------------------------------------------- 4. GaussianBag on the host
def _bag(P=300, deg=1):
    return GaussianBag.from_activated(synth_scene(P, 3, 1.0, deg), deg)


def test_host_bag_without_and_with_a_filter():
    V, K, wh = F.table(17)
    pc = _bag()
    assert pc.filter_3D is None and GaussianBag(1).filter_3D is None
    before = pc.activated()
    assert torch.equal(before[2], pc.get_opacity) and torch.equal(before[3], pc.get_scaling)
    with pytest.raises(RuntimeError, match="no 3D filter is set"):
        pc.get_scaling_with_3D_filter
    f = pc.compute_3D_filter(V, K, wh)
    assert f is pc.filter_3D and f.shape == (300, 1) and not f.requires_grad
    assert torch.equal(f, filter_3D_torch(pc._xyz.detach(), V, K, wh, 0.2))
    assert torch.equal(pc.compute_3D_filter(V, K, wh, variance=0.8), filter_3D_torch(pc._xyz.detach(), V, K, wh, 0.8))
    f = pc.compute_3D_filter(V, K, wh)
    for features in (True, False):
        xyz, feats, op, sc, rot = pc.activated(features=features)
        assert (feats is None) == (not features)
        assert torch.equal(op, pc.get_opacity_with_3D_filter) and torch.equal(sc, pc.get_scaling_with_3D_filter)
        assert torch.equal(rot, before[4]) and xyz is pc._xyz
    want_op, want_sc = filtered_activations_torch(pc._opacity, pc._scaling, f)
    assert torch.equal(op, want_op) and torch.equal(sc, want_sc)
    assert (op < before[2]).all() and (sc > before[3]).all()
    # the raw properties stay unfiltered (densification and MCMC read them)
    assert torch.equal(pc.get_opacity, before[2]) and torch.equal(pc.get_scaling, before[3])
    (op.sum() + sc.sum()).backward()
    assert pc._opacity.grad.abs().max().item() > 0 and pc._scaling.grad.abs().max().item() > 0


def test_a_stale_filter_raises():
    V, K, wh = F.table(3)
    pc = _bag()
    pc.compute_3D_filter(V, K, wh)
    for rows in (299, 301):
        pc.filter_3D = torch.ones(rows, 1)
        for use in (lambda: pc.activated(), lambda: pc.get_opacity_with_3D_filter, lambda: pc.get_scaling_with_3D_filter,
                    lambda: pc.fuse_3D_filter()):
            with pytest.raises(RuntimeError, match="stale.*compute_3D_filter"):
                use()
    pc.filter_3D = None
    pc.activated()


def test_fuse_3D_filter_round_trips():
    V, K, wh = F.table(17)
    pc = _bag()
    with pytest.raises(RuntimeError, match="no 3D filter is set"):
        pc.fuse_3D_filter()
    pc.compute_3D_filter(V, K, wh)
    fused = pc.fuse_3D_filter()
    assert fused is not pc and fused.filter_3D is None and pc.filter_3D is not None
    assert fused.active_sh_degree == pc.active_sh_degree and fused.max_sh_degree == pc.max_sh_degree
    op, sc = pc.get_opacity_with_3D_filter.detach(), pc.get_scaling_with_3D_filter.detach()
    a = fused.activated()
    assert ((a[2] - op).abs() <= 1e-6 * (1 + op.abs())).all() and ((a[3] - sc).abs() <= 1e-6 * (1 + sc.abs())).all()
    for n in ("_xyz", "_features_dc", "_features_rest", "_rotation"):
        assert torch.equal(getattr(fused, n), getattr(pc, n)) and getattr(fused, n).data_ptr() != getattr(pc, n).data_ptr()
    assert all(t.is_leaf and t.requires_grad for t in fused.leaves())


def test_render_refuses_the_python_covariance_path_with_a_filter():
    from bags_raster.render import render
    from bags_raster.synth import look_at_origin_camera
    V, K, wh = F.table(3)
    pc = _bag()
    pc.compute_3D_filter(V, K, wh)
    with pytest.raises(NotImplementedError, match="compute_cov3D_python.*unfiltered"):
        render(look_at_origin_camera(32, 24), pc, PipelineParams(compute_cov3D_python=True), torch.zeros(3), 0.0, None)


def test_docstrings_say_who_recomputes_the_filter():
    from bags_raster import io
    assert "compute_3D_filter" in GaussianBag.relocate.__doc__ and "filter_3D" in io.__doc__ and "12-tuple" in io.__doc__


# ---------------------------------------------------------------------------------------------------------------- 5. the C ABI
def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in FUNCS + ("bags_filter3d_workspace_size",):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    for name in FUNCS:
        assert _lib.SYMBOLS[name][1][-1] is C.c_void_p                                                            # the stream comes last
    assert len(_lib.SYMBOLS["bags_activations_filtered_forward"][1]) == len(_lib.SYMBOLS["bags_activations_forward"][1]) + 1
    assert len(_lib.SYMBOLS["bags_activations_filtered_backward"][1]) == len(_lib.SYMBOLS["bags_activations_backward"][1]) + 1
    sizes = [lib.bags_filter3d_workspace_size(P) for P in (0, 1, 256, 257, 1000, 500_000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert sizes[-1] >= 500_000 * 4 + (500_000 + 255) // 256 * 4
    for name in ("filter_3D", "filter_3D_torch", "filtered_activations_torch"):
        assert callable(getattr(bags_raster, name)) and name in bags_raster.__all__


def test_argument_validation(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 15) & ~15
    big = 1 << 40

    def refused(rc, text, code=-1):
        msg = lib.bags_last_error()
        assert rc == code and text in msg, (rc, msg)

    def compute(xyz=addr, P=10, V=addr, K=addr, wh=addr, N=3, variance=0.2, ws=addr, ws_bytes=big, out=addr):
        return lib.bags_filter3d_compute(xyz, P, V, K, wh, N, variance, ws, ws_bytes, out, None)
    refused(compute(P=-1), b"filter3d_compute: P < 0")
    refused(compute(N=0), b"filter3d_compute: needs at least one camera")
    refused(compute(N=-2), b"filter3d_compute: needs at least one camera")
    refused(compute(variance=-0.5), b"filter3d_compute: variance")
    refused(compute(variance=float("nan")), b"filter3d_compute: variance")
    for null in ("xyz", "V", "K", "wh", "out"):
        refused(compute(**{null: None}), b"filter3d_compute: NULL")
    refused(compute(ws=None), b"needs a workspace", code=-3)
    refused(compute(ws_bytes=lib.bags_filter3d_workspace_size(10) - 1), b"needs a workspace", code=-3)
    assert compute(P=0, xyz=None, ws=None, ws_bytes=0, out=None) == 0                     # an empty set: a successful no-op
    refused(compute(P=0, N=0), b"needs at least one camera")
    raw = _lib.BagsRawGaussians(10, 4, addr, addr, addr, addr, addr)
    refused(lib.bags_activations_filtered_forward(C.byref(raw), None, addr, addr, addr, addr, None), b"activations_filtered_forward: NULL filter_3D")
    refused(lib.bags_activations_filtered_backward(C.byref(raw), None, *([addr] * 9), None), b"activations_filtered_backward: NULL filter_3D")
    assert lib.bags_activations_filtered_forward(None, addr, addr, addr, addr, addr, None) == -1
    empty = _lib.BagsRawGaussians(0, 4, None, None, None, None, None)
    assert lib.bags_activations_filtered_forward(C.byref(empty), None, None, None, None, None, None) == 0
    assert lib.bags_activations_filtered_backward(C.byref(empty), None, *([None] * 9), None) == 0
