"""sh_colors without a GPU: the three symbols exist everywhere they must, the ABI number did not move, and the Python entry point
refuses what it cannot run (host tensors, too few coefficients, mismatched pairs, other dtypes) with a message that names the culprit."""
import os
import re

import pytest
import torch

import bags_raster
from bags_raster import _lib, sh_colors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bags_sh_colors_forward", "bags_sh_colors_backward", "bags_sh_colors_workspace_size")


def test_symbols_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    declared = set(re.findall(r"\b(bags_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct BagsShColors" in header
    assert bags_raster.sh_colors is sh_colors


def test_abi_version_is_still_11():
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    assert re.search(r"#define\s+BAGS_ABI_VERSION\s+11\b", header)
    assert _lib.ABI_VERSION == 11
    assert _lib.load().bags_abi_version() == 11


def test_workspace_size_and_argument_validation():
    lib = _lib.load()
    assert lib.bags_sh_colors_workspace_size(0) > 0
    assert lib.bags_sh_colors_workspace_size(500_000) >= (500_000 + 255) // 256 * 16
    assert lib.bags_sh_colors_workspace_size(1000) < lib.bags_sh_colors_workspace_size(1_000_000)
    ok = dict(P=0, K=16, sh_degree=3, reserved=0)
    assert lib.bags_sh_colors_forward(_lib.BagsShColors(**ok), None, None) == 0          # P == 0: nothing to launch
    assert lib.bags_sh_colors_backward(_lib.BagsShColors(**ok), None, None, 0, None, None, None, None, None) == 0
    for bad, word in ((dict(ok, K=5), "K 5"), (dict(ok, K=9), "needs 16"), (dict(ok, sh_degree=4), "sh_degree 4"), (dict(ok, P=-1), "P < 0"),
                      (dict(ok, P=3), "must be given")):
        assert lib.bags_sh_colors_forward(_lib.BagsShColors(**bad), None, None) != 0
        assert word in lib.bags_last_error().decode(), (bad, lib.bags_last_error())
    assert lib.bags_sh_colors_forward(None, None, None) != 0


def _inputs(P=5, K=16, split=False, dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    xyz = torch.rand(P, 3, generator=g).to(dtype)
    campos = torch.tensor([0.3, -0.2, 4.0], dtype=dtype)
    shs = torch.randn(P, K, 3, generator=g).to(dtype)
    if split:
        return shs[:, :1].contiguous(), xyz, campos, shs[:, 1:].contiguous()
    return shs, xyz, campos, None


def test_cpu_tensors_raise_and_name_the_argument():
    for split in (False, True):
        shs, xyz, campos, rest = _inputs(split=split)
        with pytest.raises(RuntimeError, match=r"shs must be on a 'cuda' \(ROCm\) device, got cpu.*no CPU fallback"):
            sh_colors(3, shs, xyz, campos, shs_rest=rest)


def test_too_few_coefficients_raise():
    shs, xyz, campos, _ = _inputs(K=4)
    with pytest.raises(RuntimeError, match=r"degree 2 needs 9 coefficients.*4.*\(5, 4, 3\)"):
        sh_colors(2, shs, xyz, campos)
    dc, xyz, campos, rest = _inputs(K=9, split=True)
    with pytest.raises(RuntimeError, match=r"degree 3 needs 16 coefficients"):
        sh_colors(3, dc, xyz, campos, shs_rest=rest)
    with pytest.raises(RuntimeError, match=r"K = 5 .*must be 1, 4, 9 or 16"):
        sh_colors(1, _inputs(K=5)[0], xyz, campos)
    with pytest.raises(ValueError, match="0..3"):
        sh_colors(4, shs, xyz, campos)


def test_mismatched_split_pair_raises():
    dc, xyz, campos, rest = _inputs(P=5, split=True)
    with pytest.raises(RuntimeError, match=r"shs_rest must be \(5,K-1,3\).*\(4, 15, 3\)"):
        sh_colors(3, dc, xyz, campos, shs_rest=rest[:4].contiguous())
    with pytest.raises(RuntimeError, match=r"\(4, 1, 3\)"):
        sh_colors(3, dc[:4].contiguous(), xyz, campos, shs_rest=rest)
    with pytest.raises(RuntimeError, match=r"campos must be \(3,\), got \(1, 3\)"):
        sh_colors(3, dc, xyz, campos.view(1, 3), shs_rest=rest)
    with pytest.raises(RuntimeError, match=r"xyz must be \(P,3\), got \(5, 4\)"):
        sh_colors(3, dc, torch.zeros(5, 4), campos, shs_rest=rest)


@pytest.mark.parametrize("which", ["shs", "xyz", "campos", "shs_rest"])
def test_non_float32_raises(which):
    dc, xyz, campos, rest = _inputs(split=True)
    args = {"shs": dc, "xyz": xyz, "campos": campos, "shs_rest": rest}
    args[which] = args[which].double()
    with pytest.raises(TypeError, match=rf"{which} must be float32, got torch.float64"):
        sh_colors(3, args["shs"], args["xyz"], args["campos"], shs_rest=args["shs_rest"])
