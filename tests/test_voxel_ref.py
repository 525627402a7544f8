"""The yardsticks of the coarse-to-fine tests themselves (tests/voxel_ref.py), on the CPU: the
any-order bound holds for a plain fp64 sum, the named cases are what their names say, the numpy
coarse-to-fine twin halves the cow pair's full-resolution iterations, and the measured gap between
a composed total and the moved scene is the constant the device tests scale their bound from."""
import numpy as np
import pytest

import datasets
import voxel_ref as V


@pytest.fixture(scope="module")
def icp_amd(icp_lib):
    return icp_lib


@pytest.fixture(scope="module")
def cow(icp_amd):
    return icp_amd.load_matrix(datasets.path("cow_ref")), icp_amd.load_matrix(datasets.path("cow_tr2"))


@pytest.fixture(scope="module")
def cow_plain(cow):
    m, p = cow
    return V.icp_steps(m, p, 60)


@pytest.mark.parametrize("name", V.CASES)
def test_fp64_sum_inside_bound(name, icp_amd):
    xyz, voxel, origin = V.case(name)
    mean, counts, rank = V.downsample_ref(xyz, voxel, origin)
    assert counts.sum() == xyz.shape[0] and counts.min() >= 1
    seq = V.sequential_means(xyz, rank, counts.size)
    gap = np.abs(seq.astype(np.longdouble) - mean).astype(np.float64)
    bound = V.mean_bound(xyz, rank, counts)
    print(f"{name}: {counts.size} cells, largest {counts.max()}, worst gap / bound {np.max(gap / np.maximum(bound, 1e-300)):.3f}")
    assert (gap <= bound).all()


def test_cases_are_what_they_say(icp_amd):
    for n in V.SIZES:
        assert V.case("n%d" % n)[0].shape == (n, 3)
    for n in (4097, 70000):
        xyz, voxel, origin = V.case("one_cell%d" % n)
        assert V.downsample_ref(xyz, voxel, origin)[1].tolist() == [n]
    xyz, voxel, origin = V.case("own_cell")
    assert (V.downsample_ref(xyz, voxel, origin)[1] == 1).all()
    xyz, voxel, origin = V.case("mixed")
    counts = V.downsample_ref(xyz, voxel, origin)[1]
    assert sorted(counts.tolist())[-2:] == [65, 4097] and (np.sort(counts)[:-2] == 1).all()
    xyz, voxel, origin = V.case("duplicates")
    assert np.unique(xyz, axis=0).shape[0] * 3 == xyz.shape[0]
    a, b = V.case("shared_a"), V.case("shared_b")
    assert a[1] == b[1] and a[2] == b[2] and a[2] is not None


@pytest.mark.parametrize("name", ["boundary_tenth", "boundary_eighth"])
def test_boundary_points_sit_on_faces(name):
    xyz, voxel, origin = V.case(name)
    q = (xyz - np.asarray(origin)) / voxel
    on_face = (q == np.floor(q)).any(axis=1)
    print(f"{name}: {int(on_face.sum())} of {xyz.shape[0]} points with an integer (x - lo) / voxel")
    assert on_face.sum() >= 100


def test_wide_case_needs_more_than_32_key_bits():
    xyz, voxel, origin = V.case("wide")
    lo, g, key, keys, _ = V.partition(xyz, voxel, origin)
    assert g.tolist() == [4097, 4097, 4097]
    assert int(keys.max()).bit_length() > 32
    # both words matter: cells that share a low word, cells that share a high word
    assert np.unique(keys >> 32).size > 1 and np.unique(keys & 0xFFFFFFFF).size > 1
    assert keys.size < xyz.shape[0]  # (some cells hold two points)


def test_twin_halves_the_cow_pairs_iterations(cow, cow_plain):
    m, p = cow
    _, errs, _ = cow_plain
    h = V.extent(m) / V.COW_VOXEL_DIV
    _, fine_errs, _, levels = V.pyramid_twin(m, p, [h], 60, 30)
    print(f"cow_ref / cow_tr2: plain {len(errs)} iterations, after a coarse pass at extent/{V.COW_VOXEL_DIV} "
          f"({levels[0][0]} / {levels[0][1]} points, {levels[0][2]} iterations) {len(fine_errs)}")
    assert errs[-1] < 1e-5 and fine_errs[-1] < 1e-5
    assert 2 * len(fine_errs) <= len(errs)


def test_total_against_moved_scene(cow, cow_plain):
    _, p = cow
    moved, _, steps = cow_plain
    total = V.compose(steps)
    total_ld = V.compose(steps, np.longdouble)
    scale = np.abs(p).max()
    G = np.abs(V.apply(total, p) - moved).max()
    G_ld = float(np.abs(V.apply(total_ld, p) - moved).max())
    comp = float(np.abs(V.apply(total, p) - V.apply(total_ld, p)).max())
    print(f"G = {G:.3e} ({G / scale:.3e} of max |p| = {scale:.4g}) over {len(steps)} iterations; against the "
          f"longdouble composition of the same steps {G_ld:.3e}; fp64 against longdouble composition {comp:.3e}")
    # the constant the device tests use: not below the measurement, not idly above it
    assert G / scale <= V.G_REL <= 4.0 * max(G, G_ld) / scale
    assert comp <= G  # (composing in fp64 is not what the gap comes from: the moved scene's own rounding is)


def test_too_few_case_stops_after_two_iterations(oracle):
    import gated_ref
    m, p, dmax, completed = V.too_few_case()
    ref = gated_ref.gated_ref(oracle, m, p, dmax, 8, -1.0)
    print("K", ref["K"], "then", ref.get("K_fail"), "margin", ref["margin"])
    assert ref["status"] == "few" and ref["iterations"] == completed and ref["K"] == [4, 5]
    assert ref["margin"] > 1e-3  # (no pair near the gate: the device's K cannot differ)
