"""Named point clouds for distCUDA2 (csrc/knn.hip), each aimed at one path of the grid sizing, the scan or the shell walk -- numpy
only, so that tests/test_knn_cases_cpu.py can check the clouds and their reference without a GPU.

``cloud(name)``        the (P, 3) float32 cloud of one case, seeded by its name; read-only, built once.
``oracle(name)``       ``oracle.knn_oracle.dist_mean3`` of that cloud; read-only, computed once and shared by every test.
``uniform(P, seed)``   the uniform cloud in [-1.3, 1.3]^3 that the scan, scale and permutation tests use.
``plane(P, seed)``     the same cloud flattened to z = 0.25: the shape whose occupied cells reach past the first pass of the top scan.
``grid_facts(points)`` a float32 restatement of ``knn_setup_kernel`` and ``cell_of``: which grid the kernel builds for a cloud.  It
                       exists only to show that a case reaches the path it is named for; no bar is derived from it.
"""
import functools
import zlib

import numpy as np

from oracle import knn_oracle as KO

SCAN_EDGE_SIZES = (2046, 2047, 2048, 4095, 4096)        # n = P + 1 against the scan tile of 2048: one below, equal, one above; one tile and two
LATTICES = {"lattice_cube": 0.25, "lattice_far": 1.0, "lattice_slab": 0.5}             # name -> spacing h; the result is h * h everywhere


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _lattice(nx, ny, nz, h, origin):
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    ijk = np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(np.float64)
    return (ijk * h + np.asarray(origin, dtype=np.float64)).astype(np.float32)          # every coordinate is exact in float32


def uniform(P, seed):
    return (np.random.default_rng(seed).random((P, 3)) * 2.6 - 1.3).astype(np.float32)


def plane(P, seed):
    """x, y uniform in [-1.3, 1.3], z = 0.25.  A flat cloud gets up to 1024 x 1024 x 1 cells, cut down to <= P by the growth loop: the
    one shape whose cell count comes close to P.  At P = CARRY_PLANE_P the grid is 813 x 813 = 660 969 cells, so cells beyond
    256 * 2048 = 524 288 are occupied and their cell_start needs the carry of knn_scan_top_kernel's second pass.  (A volume-filling
    cloud has about P / 4 cells: below 2 M points its counts past 524 288 are all zero and the carry moves only empty cells.)"""
    p = uniform(P, seed)
    p[:, 2] = 0.25
    return p


CARRY_PLANE_P = 662_000
SCAN_TOP_PASS = 256 * 2048                                # counts that one pass of knn_scan_top_kernel covers


def _lattice_cube(rng):                                  # exact ties: every neighbour distance is h
    return _lattice(12, 12, 12, 0.25, (3.0, -7.5, 100.0))


def _lattice_far(rng):                                    # the same ties at a large offset
    return _lattice(12, 12, 12, 1.0, (4096.0, 4096.0, 4096.0))


def _lattice_slab(rng):                                   # ties in a grid one cell thick
    return _lattice(40, 40, 2, 0.5, (-3.0, -3.0, -3.0))


def _line_short(rng):                                     # P = 100 on a line: 1024 cells along x would exceed P, the growth loop runs
    p = np.zeros((100, 3)); p[:, 0] = rng.random(100) * 100.0
    return p.astype(np.float32)


def _line_even(rng):                                      # ex / cell = 1024: 1025 cells before the clamp, the last point on the clamped index
    p = np.zeros((1500, 3)); p[:, 0] = 0.125 * np.arange(1500)
    return p.astype(np.float32)


def _offset_1e4(rng):                                     # dx = p.x - q.x cancels four digits
    return (rng.random((1500, 3)) + 1.0e4).astype(np.float32)


def _far_blobs(rng):                                      # two occupied cells; each thread walks its whole blob
    p = rng.normal(size=(1500, 3)) * 0.01
    p[750:] += 1.0e5                                      # float32 spacing 2^-7 there: points fall together
    return p.astype(np.float32)


def _needle_box(rng):
    return (rng.random((2000, 3)) * np.array([1000.0, 1.0, 1.0])).astype(np.float32)


def _thin_box(rng):                                       # the volume rule gives a cell far below the spacing: the growth loop runs
    return (rng.random((2000, 3)) * np.array([1.0, 1.0, 1.0e-4])).astype(np.float32)


def _coincident_64(rng):                                  # the third-best distance is 0: the walk stops at shell 0 with reach = 0
    return np.repeat(rng.random((60, 3)), 64, axis=0).astype(np.float32)


def _all_coincident(rng):                                 # zero extent: cell = 0 is reset to 1
    return np.repeat(np.array([[0.3, -1.7, 42.0]]), 300, axis=0).astype(np.float32)


_BUILDERS = {
    "lattice_cube": _lattice_cube, "lattice_far": _lattice_far, "lattice_slab": _lattice_slab, "line_short": _line_short,
    "line_even": _line_even, "offset_1e4": _offset_1e4, "far_blobs": _far_blobs, "needle_box": _needle_box, "thin_box": _thin_box,
    "coincident_64": _coincident_64, "all_coincident": _all_coincident,
}
for _P in SCAN_EDGE_SIZES:
    _BUILDERS["scan_edges_%d" % _P] = (lambda P: lambda rng: (rng.random((P, 3)) * 2.6 - 1.3).astype(np.float32))(_P)
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def cloud(name):
    p = np.ascontiguousarray(_BUILDERS[name](_rng(name)), dtype=np.float32)
    assert p.ndim == 2 and p.shape[1] == 3 and p.shape[0] <= 4096 and np.isfinite(p).all()          # brute-force cases stay small
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def oracle(name):
    want = KO.dist_mean3(cloud(name))
    want.setflags(write=False)
    return want


def grid_facts(points):
    """The grid ``knn_setup_kernel`` builds for ``points`` and how ``cell_of`` fills it, in float32 as the kernel states them:
    extent (3,), cell, growth (steps of the ``cell *= 1.26`` loop taken), n_unclamped / n (per-axis cell counts before and after the
    clamp at 1024, at the final cell), fallback (the single-cell reset after 64 steps), reset (the ``cell = 1`` reset), ncells,
    cell_index (P, 3) as ``cell_of`` clamps it, clamped (P,) bool: the point's own index lay beyond the last cell on some axis,
    max_occupancy."""
    f32 = np.float32
    p = np.ascontiguousarray(points, dtype=f32)
    P = p.shape[0]
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = np.maximum(hi - lo, f32(0))
    emax = ext.max()
    target = max(f32(1), f32(0.25) * f32(P))
    with np.errstate(under="ignore"):
        vol = np.maximum(ext[0], f32(1e-30)) * np.maximum(ext[1], f32(1e-30)) * np.maximum(ext[2], f32(1e-30))
        cell = np.cbrt(f32(vol / target), dtype=f32)
    cell = max(cell, f32(emax / f32(1024)))
    reset = not (cell > 0) or not np.isfinite(cell)
    if reset:
        cell = f32(1)
    cap = max(P, 1)
    growth = 0
    for it in range(64):
        raw = (ext / cell).astype(np.int64) + 1
        n = np.minimum(1024, raw)
        if int(n[0]) * int(n[1]) * int(n[2]) <= cap:
            break
        cell = f32(cell * f32(1.26))
        growth += 1
    fallback = int(n[0]) * int(n[1]) * int(n[2]) > cap
    if fallback:
        n = np.array([1, 1, 1]); cell = f32(max(emax, f32(1)) * f32(2))
    inv = f32(1) / cell
    own = ((p - lo) * inv).astype(np.int64)                                        # (int) of a non-negative float: truncation
    idx = np.minimum(n - 1, np.maximum(0, own))
    flat = (idx[:, 2] * n[1] + idx[:, 1]) * n[0] + idx[:, 0]
    return dict(extent=ext, cell=float(cell), growth=growth, n_unclamped=tuple(int(v) for v in raw), n=tuple(int(v) for v in n),
                fallback=bool(fallback), reset=bool(reset), ncells=int(n[0]) * int(n[1]) * int(n[2]), cell_index=idx,
                clamped=(own > (n - 1)).any(axis=1), max_occupancy=int(np.bincount(flat).max()))
