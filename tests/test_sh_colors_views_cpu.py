"""sh_colors_views / render_views without a GPU: the three symbols exist everywhere they must, the ABI number did not move, the C
entry points refuse a view count outside 1..16 and name the limit, and the Python entry point refuses what it cannot run."""
import inspect
import os
import re

import pytest
import torch

import bags_raster
from bags_raster import _lib, render, render_views, sh_colors_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bags_sh_colors_views_forward", "bags_sh_colors_views_backward", "bags_sh_colors_views_workspace_size")


def test_symbols_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    declared = set(re.findall(r"\b(bags_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct BagsShColorsViews" in header
    assert bags_raster.sh_colors_views is sh_colors_views and bags_raster.render_views is render_views
    assert "sh_colors_views" in bags_raster.__all__ and "render_views" in bags_raster.__all__


def test_abi_version_is_still_11():
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    assert re.search(r"#define\s+BAGS_ABI_VERSION\s+11\b", header)
    assert re.search(r"#define\s+BAGS_MAX_SH_VIEWS\s+16\b", header)
    assert _lib.ABI_VERSION == 11 and _lib.MAX_SH_VIEWS == 16
    assert _lib.load().bags_abi_version() == 11


def test_struct_layout_matches_the_header():
    S = _lib.BagsShColorsViews
    assert [f[0] for f in S._fields_] == ["P", "K", "sh_degree", "V", "shs", "shs_rest", "xyz", "campos"]
    assert S.shs.offset == 16 and S.campos.offset == 40 and S.campos.size == 8 * 16


def test_view_count_outside_1_to_16_is_refused_and_the_limit_named():
    lib = _lib.load()
    ok = dict(P=0, K=16, sh_degree=3)
    for V in (0, 17, -1):
        a = _lib.BagsShColorsViews(V=V, **ok)
        assert lib.bags_sh_colors_views_forward(a, None, None) != 0
        assert f"V {V}" in lib.bags_last_error().decode() and "1..16" in lib.bags_last_error().decode()
        assert lib.bags_sh_colors_views_backward(a, None, None, 0, None, None, None, None, None) != 0
        assert f"V {V}" in lib.bags_last_error().decode() and "1..16" in lib.bags_last_error().decode()
    for V in (1, 16):                                                   # P == 0: nothing to launch
        a = _lib.BagsShColorsViews(V=V, **ok)
        assert lib.bags_sh_colors_views_forward(a, None, None) == 0
        assert lib.bags_sh_colors_views_backward(a, None, None, 0, None, None, None, None, None) == 0
    for bad, word in ((dict(ok, K=5), "K 5"), (dict(ok, K=9), "needs 16"), (dict(ok, sh_degree=4), "sh_degree 4"), (dict(ok, P=-1), "P < 0"),
                      (dict(ok, P=3), "must be given")):               # what the views share: the single-view rules
        assert lib.bags_sh_colors_views_forward(_lib.BagsShColorsViews(V=2, **bad), None, None) != 0
        assert word in lib.bags_last_error().decode(), (bad, lib.bags_last_error())
    assert lib.bags_sh_colors_views_forward(None, None, None) != 0


def test_workspace_size_grows_with_views_and_gaussians():
    size = _lib.load().bags_sh_colors_views_workspace_size
    assert size(0, 1) > 0
    assert size(500_000, 5) >= 5 * ((500_000 + 255) // 256) * 16
    assert size(500_000, 1) < size(500_000, 5) < size(500_000, 16)
    assert size(1000, 5) < size(1_000_000, 5)


def _inputs(P=5, K=16, V=3, split=False, dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    xyz = torch.rand(P, 3, generator=g).to(dtype)
    camposes = [torch.tensor([0.3 + v, -0.2, 4.0], dtype=dtype) for v in range(V)]
    shs = torch.randn(P, K, 3, generator=g).to(dtype)
    if split:
        return shs[:, :1].contiguous(), xyz, camposes, shs[:, 1:].contiguous()
    return shs, xyz, camposes, None


def test_cpu_tensors_raise_and_name_the_argument():
    for split in (False, True):
        shs, xyz, camposes, rest = _inputs(split=split)
        with pytest.raises(RuntimeError, match=r"sh_colors_views runs only on an AMD GPU: shs must be on a 'cuda' \(ROCm\) device, got cpu.*no CPU fallback"):
            sh_colors_views(3, shs, xyz, camposes, shs_rest=rest)


def test_view_count_out_of_range_raises():
    shs, xyz, _, _ = _inputs()
    with pytest.raises(ValueError, match=r"1\.\.16, got 0"):
        sh_colors_views(3, shs, xyz, [])
    with pytest.raises(ValueError, match=r"1\.\.16, got 17"):
        sh_colors_views(3, shs, xyz, _inputs(V=17)[2])
    with pytest.raises(ValueError, match="0..3"):
        sh_colors_views(4, shs, xyz, _inputs()[2])
    with pytest.raises(TypeError, match="camposes must be a list or tuple"):
        sh_colors_views(3, shs, xyz, torch.zeros(2, 3))


def test_wrong_shapes_and_dtypes_raise():
    dc, xyz, camposes, rest = _inputs(P=5, split=True)
    with pytest.raises(RuntimeError, match=r"shs_rest must be \(5,K-1,3\).*\(4, 15, 3\)"):
        sh_colors_views(3, dc, xyz, camposes, shs_rest=rest[:4].contiguous())
    with pytest.raises(RuntimeError, match=r"\(4, 1, 3\)"):
        sh_colors_views(3, dc[:4].contiguous(), xyz, camposes, shs_rest=rest)
    with pytest.raises(RuntimeError, match=r"camposes\[1\] must be \(3,\), got \(1, 3\)"):
        sh_colors_views(3, dc, xyz, [camposes[0], camposes[1].view(1, 3)], shs_rest=rest)
    with pytest.raises(RuntimeError, match=r"xyz must be \(P,3\), got \(5, 4\)"):
        sh_colors_views(3, dc, torch.zeros(5, 4), camposes, shs_rest=rest)
    with pytest.raises(RuntimeError, match=r"degree 2 needs 9 coefficients.*4.*\(5, 4, 3\)"):
        sh_colors_views(2, _inputs(K=4)[0], xyz, camposes)
    with pytest.raises(RuntimeError, match=r"K = 5 .*must be 1, 4, 9 or 16"):
        sh_colors_views(1, _inputs(K=5)[0], xyz, camposes)
    with pytest.raises(TypeError, match=r"camposes\[2\] must be float32, got torch.float64"):
        sh_colors_views(3, dc, xyz, camposes[:2] + [camposes[2].double()], shs_rest=rest)
    with pytest.raises(TypeError, match=r"camposes\[0\] must be a tensor, got tuple"):
        sh_colors_views(3, dc, xyz, [(0.0, 0.0, 1.0)], shs_rest=rest)


def test_render_views_has_renders_keywords():
    a, b = inspect.signature(render), inspect.signature(render_views)
    pa, pb = list(a.parameters.values()), list(b.parameters.values())
    assert pb[0].name == "cameras"
    assert [(p.name, p.default, p.kind) for p in pa[1:]] == [(p.name, p.default, p.kind) for p in pb[1:]]
