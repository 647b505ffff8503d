"""distCUDA2 (csrc/knn.hip behind bags_knn_mean_dist2) against the brute-force oracle and scipy's cKDTree.

The paths of knn.hip and the case of tests/knn_cases.py (or the test here) that reaches each:
  exact ties at the stop rule ``b2 <= reach * reach``     lattice_cube, lattice_far (large offset), lattice_slab (grid one cell thick)
  growth loop of knn_setup_kernel (cells <= P)             line_short (1024 cells for 100 points), thin_box (from the volume rule)
  clamp at 1024 cells per axis                              line_even (1025 before the clamp, the last point on the clamped index)
  ``cell = 1`` reset for a cloud of zero extent             all_coincident
  stop at shell 0 with reach = 0                            coincident_64
  one long axis, rows of one contiguous run                 needle_box
  cancellation in dx at a large offset                      offset_1e4
  two occupied cells, brute force inside one                far_blobs
  tile edges of the scan, ``out[n]`` at a tile's end        scan_edges_2046 .. scan_edges_4096 (n = P + 1 around 2048 and 4096)
  carry of knn_scan_top_kernel (more than 256 partials)     test_knn_top_scan_carry (uniform P = 524 287, 524 288, 1 050 000: the loop;
                                                            plane P = 662 000: occupied cells behind the carry)
  result independent of the grid it was found through       test_knn_is_scale_free (2^-20, 2^12)
  reach of the output index, order inside a cell            test_knn_commutes_with_permutation, test_knn_repeats_bit_equal
  a workspace that is not fresh, and its bounds             test_knn_dirty_fenced_workspace
  what the wrapper converts; P = 0                          test_knn_wrapper_conversions, test_knn_empty_cloud
"""
import ctypes

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import knn_cases as KC
from bags_raster import _lib as L
from bags_raster.knn import distCUDA2
from oracle import knn_oracle as KO

pytestmark = pytest.mark.gpu


def _hip(pts: np.ndarray) -> np.ndarray:
    return distCUDA2(torch.tensor(pts, device="cuda")).cpu().numpy()       # a copy: the clouds of knn_cases are read-only


def _cloud(kind, n, rng):
    if kind == "uniform":
        return (rng.random((n, 3)) * 2.6 - 1.3).astype(np.float32)
    if kind == "clustered":                      # dense blobs + a few far outliers: most grid cells are empty
        c = rng.normal(size=(8, 3)) * 5.0
        p = c[rng.integers(0, 8, n)] + rng.normal(size=(n, 3)) * 0.05
        p[:5] = rng.normal(size=(5, 3)) * 400.0
        return p.astype(np.float32)
    if kind == "plane":                          # degenerate extent along z
        p = rng.random((n, 3)); p[:, 2] = 0.25
        return p.astype(np.float32)
    if kind == "line":
        p = np.zeros((n, 3)); p[:, 0] = rng.random(n) * 100.0
        return p.astype(np.float32)
    if kind == "duplicates":
        p = rng.random((n // 4, 3))
        return np.repeat(p, 4, axis=0).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["uniform", "clustered", "plane", "line", "duplicates"])
def test_knn_matches_oracle(kind):
    rng = np.random.default_rng(11)
    pts = _cloud(kind, 4000, rng)
    got, want = _hip(pts), KO.dist_mean3(pts)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-30)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 257])
def test_knn_tiny_inputs(n):
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3)).astype(np.float32)
    got, want = _hip(pts), KO.dist_mean3(pts)
    big = want > 1e37                            # fewer than three neighbours: FLT_MAX terms (sum overflows to inf)
    assert np.array_equal(got > 1e37, big)
    np.testing.assert_allclose(got[~big], want[~big], rtol=2e-6)


def test_knn_full_size_against_kdtree_and_call_site():
    """500 k points of the bench scene: exact agreement with cKDTree, and the reference's use of the result
    (scene/gaussian_model.py:177-178) gives finite log-scales."""
    from bags_raster.synth import synth_scene
    pts = synth_scene(500_000, 0, 0.5, 0)["means3D"].numpy()
    t = torch.from_numpy(pts).cuda()
    distCUDA2(t); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = distCUDA2(t); e1.record(); torch.cuda.synchronize()
    print("distCUDA2(500k): %.3f ms" % e0.elapsed_time(e1))
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4, workers=-1)
    want = (d[:, 1:] ** 2).mean(axis=1)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=2e-5)
    scales = torch.log(torch.sqrt(torch.clamp_min(out, 1e-7)))[..., None].repeat(1, 3)
    assert torch.isfinite(scales).all()
    # the alias the reference imports
    from simple_knn._C import distCUDA2 as alias
    assert torch.equal(alias(t), out)


def test_knn_rejects_cpu_and_bad_shapes():
    with pytest.raises(RuntimeError, match="GPU tensor"):
        distCUDA2(torch.rand(10, 3))
    with pytest.raises(RuntimeError, match=r"\(P,3\)"):
        distCUDA2(torch.rand(10, 2).cuda())


# ------------------------------------------------------------------------------------------ the cases of tests/knn_cases.py
RTOL = 2e-6           # the bar of test_knn_matches_oracle.  Both sides form dx*dx + dy*dy + dz*dz, two adds and a division in float32
                      # from identical inputs; they differ by contraction only, a few roundings of 2^-24 = 6e-8 each


def _against_oracle(label, got, want):
    """The bar of this file: entries above 1e37 as a mask, exact zeros exact, everything else at RTOL.  Prints the worst relative error."""
    big = want > 1e37
    assert np.array_equal(got > 1e37, big)
    zero = want == 0
    assert np.all(got[zero] == 0), "%s: %d entries are 0 in the oracle and not in the kernel" % (label, np.count_nonzero(got[zero]))
    m = ~big & ~zero
    rel = np.abs(got[m].astype(np.float64) - want[m]) / want[m] if m.any() else np.zeros(1)
    print("%s: P = %d, worst relative error %.3e (%d exact zeros)" % (label, want.shape[0], rel.max(), np.count_nonzero(zero)))
    np.testing.assert_allclose(got[m], want[m], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", KC.CASES)
def test_knn_case_matches_oracle(name):
    _against_oracle(name, _hip(KC.cloud(name)), KC.oracle(name))


@pytest.mark.parametrize("name", sorted(KC.LATTICES))
def test_knn_lattice_is_exact(name):
    """Every lattice point has at least three neighbours at distance h, dy = dz = 0 makes the products exact, and 3 h^2 / 3 is exact
    for a power-of-two h: any correct 3-NN gives h * h bit for bit."""
    h = np.float32(KC.LATTICES[name])
    got = _hip(KC.cloud(name))
    assert np.array_equal(got, np.full(got.shape, h * h, np.float32))


@pytest.mark.parametrize("k", [-20, 12])
def test_knn_is_scale_free(k):
    """The grid is not scale-free (the 1e-30 floors and the cell = 1 reset are absolute); the answer is: the oracle's is, bit for
    bit (tests/test_knn_cases_cpu.py), so the scaled cloud is held to the unscaled oracle."""
    p = KC.uniform(3000, 5)
    s = np.float32(2.0 ** k)
    _against_oracle("uniform_3000 * 2^%d" % k, _hip(p * s), KO.dist_mean3(p) * (s * s))


@pytest.mark.parametrize("name", ["far_blobs", "uniform_3000"])
def test_knn_commutes_with_permutation(name):
    """The counting sort's atomics reorder a cell's points, but knn_push keeps the three smallest as a multiset and the sum is taken
    in sorted order: bit equality is the contract.  A failure here with test_knn_repeats_bit_equal passing means a value reached the
    wrong row; both failing means the sum depends on the order in which a cell's points are visited."""
    p = KC.uniform(3000, 6) if name == "uniform_3000" else KC.cloud(name)
    perm = np.random.default_rng(7).permutation(p.shape[0])
    assert np.array_equal(_hip(np.ascontiguousarray(p[perm])), _hip(p)[perm])


@pytest.mark.parametrize("name", ["far_blobs", "uniform_3000"])
def test_knn_repeats_bit_equal(name):
    p = KC.uniform(3000, 6) if name == "uniform_3000" else KC.cloud(name)
    t = torch.tensor(p, device="cuda")
    first = distCUDA2(t)
    assert torch.equal(distCUDA2(t), first) and torch.equal(distCUDA2(t), first)


@pytest.mark.parametrize("kind,P,nparts", [("uniform", 524_287, 256), ("uniform", 524_288, 257), ("uniform", 1_050_000, 513),
                                           ("plane", KC.CARRY_PLANE_P, 324)])
def test_knn_top_scan_carry(kind, P, nparts):
    """cdiv(P + 1, 2048) = 256 partials (one full pass of knn_scan_top_kernel), 257 (one element in the second pass), 513 (three
    passes): the smallest sizes that run the carry loop.  A volume-filling cloud has about P / 4 cells, so at these sizes the uniform
    clouds hand the later passes zero counts only; the plane has 660 969 cells (tests/test_knn_cases_cpu.py), a fifth of its points in
    cells whose cell_start is wrong without the carry, and there the error is gross."""
    assert -(-(P + 1) // 2048) == nparts
    pts = KC.uniform(P, P) if kind == "uniform" else KC.plane(P, 3)
    got = _hip(pts)
    p64 = pts.astype(np.float64)
    d, _ = cKDTree(p64).query(p64, k=4, workers=16)
    want = (d[:, 1:] ** 2).mean(axis=1)
    rel = np.abs(got - want) / want
    print("%s P = %d against cKDTree: worst relative error %.3e" % (kind, P, rel.max()))
    np.testing.assert_allclose(got, want, rtol=2e-5)


BAND, DIRT = 4096, 0xA5


@pytest.mark.parametrize("P,shift", [(4095, 0), (2048, 0), (2048, 1)])
def test_knn_dirty_fenced_workspace(P, shift):
    """bags_knn_mean_dist2 on a caller-owned region of exactly bags_knn_workspace_size(P) bytes, dirty, between two bands that are
    read back.  shift = 1 starts the region one byte past a 256-byte boundary, so that rounding the base up uses the whole slack."""
    pts = torch.tensor(KC.cloud("scan_edges_%d" % P), device="cuda")
    fresh = distCUDA2(pts)
    n = L.load().bags_knn_workspace_size(P)
    buf = torch.full((BAND + shift + n + BAND,), DIRT, dtype=torch.uint8, device=pts.device)
    region = buf[BAND + shift:BAND + shift + n]
    assert region.data_ptr() % 256 == shift and region.numel() == n

    def run():
        out = torch.full((P,), float("nan"), dtype=torch.float32, device=pts.device)
        L.call("bags_knn_mean_dist2", pts.device, pts.data_ptr(), P, region.data_ptr(), n, out.data_ptr())
        return out

    outs = [run(), run()]                              # dirty with 0xA5; then as the first call left it
    region.fill_(0xFF)
    outs.append(run())
    for out in outs:
        assert torch.equal(out, fresh)
    assert bool((buf[:BAND + shift] == DIRT).all()) and bool((buf[BAND + shift + n:] == DIRT).all())


def test_knn_wrapper_conversions():
    p = KC.cloud("scan_edges_2046")
    t = torch.tensor(p, device="cuda")
    want = distCUDA2(t)
    assert torch.equal(distCUDA2(t.double()), want)                                    # float64 holding float32 values
    q = torch.zeros(p.shape[0], 4, device=t.device); q[:, :3] = t; q[:, 3] = 7.0
    view = q[:, :3]
    assert not view.is_contiguous()
    assert torch.equal(distCUDA2(view), want)


def test_knn_empty_cloud():
    out = distCUDA2(torch.empty(0, 3, device="cuda"))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.is_cuda
    # the entry point returns before it looks at a pointer: with P = 0 there is nothing it could launch on
    assert L.load().bags_knn_mean_dist2(None, 0, None, 0, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
