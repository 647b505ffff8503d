"""tests/knn_cases.py without a GPU: every cloud's reference against an independent exact k-NN, the grid path each cloud is named
for (through ``grid_facts``), and the three properties of oracle/knn_oracle.py that tests/test_knn_gpu.py leans on."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import knn_cases as KC
from oracle import knn_oracle as KO


def _kdtree(pts):
    p64 = pts.astype(np.float64)
    d, _ = cKDTree(p64).query(p64, k=4)
    return (d[:, 1:] ** 2).mean(axis=1)


@pytest.mark.parametrize("name", KC.CASES)
def test_case_oracle_matches_kdtree(name):
    pts, got = KC.cloud(name), KC.oracle(name)
    assert pts.dtype == np.float32 and got.dtype == np.float32
    want = _kdtree(pts)
    zero = want == 0
    assert np.all(got[zero] == 0)                                     # exactly 0 where the reference is 0
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=2e-5, atol=0)


def test_case_clouds_are_seeded():
    for name in ("line_short", "far_blobs", "scan_edges_2047"):
        assert np.array_equal(KC._BUILDERS[name](KC._rng(name)), KC.cloud(name))


# ---------------------------------------------------------------------------------- the path each case is named for
def test_facts_lattice_cube():
    f = KC.grid_facts(KC.cloud("lattice_cube"))
    assert f["n"] == (8, 8, 8) and f["growth"] == 0
    assert np.array_equal(KC.oracle("lattice_cube"), np.full(12 ** 3, 0.0625, np.float32))


def test_facts_lattice_far():
    assert np.array_equal(KC.oracle("lattice_far"), np.full(12 ** 3, 1.0, np.float32))


def test_facts_lattice_slab():
    f = KC.grid_facts(KC.cloud("lattice_slab"))
    assert f["n"] == (32, 32, 1)
    assert np.array_equal(KC.oracle("lattice_slab"), np.full(40 * 40 * 2, 0.25, np.float32))


def test_facts_line_short():
    pts = KC.cloud("line_short")
    f = KC.grid_facts(pts)
    assert f["growth"] >= 3 and not f["fallback"]
    assert f["n"][0] <= pts.shape[0] and f["n"][1:] == (1, 1)


def test_facts_line_even():
    pts = KC.cloud("line_even")
    f = KC.grid_facts(pts)
    assert f["n_unclamped"][0] == 1025 and f["n"] == (1024, 1, 1) and f["growth"] == 0
    assert f["clamped"][-1] and f["cell_index"][-1, 0] == 1023        # the last point's own index is 1024: it sits on the clamped one


def test_facts_far_blobs():
    f = KC.grid_facts(KC.cloud("far_blobs"))
    assert f["max_occupancy"] >= 700
    want = KC.oracle("far_blobs")
    assert (want[750:] == 0).any()                                    # coordinates at 1e5 quantise to 2^-7: four or more points fall together
    assert (want > 0).any()


def test_facts_needle_box():
    f = KC.grid_facts(KC.cloud("needle_box"))
    assert f["n"][0] > 500 and f["n"][1:] == (1, 1)


def test_facts_thin_box():
    f = KC.grid_facts(KC.cloud("thin_box"))
    assert f["growth"] >= 3 and not f["fallback"] and f["n"][2] == 1


def test_facts_coincident_64():
    pts = KC.cloud("coincident_64")
    assert pts.shape[0] == 3840 and np.unique(pts, axis=0).shape[0] == 60
    assert np.all(KC.oracle("coincident_64") == 0)


def test_facts_all_coincident():
    pts = KC.cloud("all_coincident")
    f = KC.grid_facts(pts)
    assert pts.shape[0] == 300 and np.all(f["extent"] == 0)
    assert f["reset"] and f["cell"] == 1.0 and f["n"] == (1, 1, 1)
    assert np.all(KC.oracle("all_coincident") == 0)


def test_facts_scan_edges():
    tile = 2048                                                       # KSCAN_TILE of csrc/knn.hip; the scan runs over n = P + 1 counts
    sizes = [KC.cloud("scan_edges_%d" % P).shape[0] for P in KC.SCAN_EDGE_SIZES]
    assert sizes == list(KC.SCAN_EDGE_SIZES)
    assert [(P + 1) % tile for P in sizes] == [tile - 1, 0, 1, 0, 1]
    assert [-(-(P + 1) // tile) for P in sizes] == [1, 1, 2, 2, 3]


def test_facts_top_scan_carry_clouds():
    """Which clouds of test_knn_top_scan_carry make the carry visible.  The scan runs over P + 1 counts, but only the first ncells
    are non-zero: the carry of the second pass is added to cell_start of cells >= 524 288 alone.  The uniform clouds run the loop and
    have every such cell empty; the plane has occupied cells there."""
    for P in (524_287, 524_288, 1_050_000):
        assert KC.grid_facts(KC.uniform(P, P))["ncells"] < KC.SCAN_TOP_PASS
    pts = KC.plane(KC.CARRY_PLANE_P, 3)
    f = KC.grid_facts(pts)
    assert f["n"] == (813, 813, 1) and f["growth"] == 1
    flat = f["cell_index"][:, 1] * 813 + f["cell_index"][:, 0]
    assert np.count_nonzero(flat >= KC.SCAN_TOP_PASS) > 100_000       # a fifth of the cloud sits behind the carry


# ---------------------------------------------------------------------------------- what the GPU tests take from the oracle
def test_oracle_is_scale_free_by_powers_of_two():
    p = KC.uniform(3000, 5)
    base = KO.dist_mean3(p)
    for k in (-20, 12):
        s = np.float32(2.0 ** k)
        assert np.array_equal(KO.dist_mean3(p * s), base * (s * s))


def test_oracle_commutes_with_permutation():
    p = KC.uniform(3000, 6)
    perm = np.random.default_rng(7).permutation(p.shape[0])
    assert np.array_equal(KO.dist_mean3(p[perm]), KO.dist_mean3(p)[perm])


@pytest.mark.parametrize("name", sorted(KC.LATTICES))
def test_oracle_lattice_is_exact(name):
    h = np.float32(KC.LATTICES[name])
    want = KC.oracle(name)
    assert np.array_equal(want, np.full(want.shape, h * h, np.float32))
