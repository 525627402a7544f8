"""The yardsticks of the coarse-to-fine tests themselves (tests/voxel_ref.py), on the CPU: the
any-order bound holds for a plain fp64 sum, the named cases are what their names say, the numpy
coarse-to-fine twin halves the cow pair's full-resolution iterations, and the measured gap between
a composed total and the moved scene is the constant the device tests scale their bound from.
rule_means, the header's order of the sum, is the rule written out cell by cell, lies inside the
any-order bound, starts from +0 and is not a sum in input order; the twin's pyramids stop clear of
the threshold and do not feel how the coarse means are rounded."""
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


_BIG = {}


def big(name):
    """(xyz, voxel, origin, means longdouble, counts, rank) of a case, once."""
    if name not in _BIG:
        xyz, voxel, origin = V.case(name)
        _BIG[name] = (xyz, voxel, origin) + V.downsample_ref(xyz, voxel, origin)
    return _BIG[name]


def test_big_cases_are_what_they_say():
    xyz, voxel, origin, _, counts, _ = big("lengths")
    assert sorted(counts.tolist()) == V.LENGTHS and xyz.shape[0] == 99547 and (counts > 4096).sum() == 5
    # (the cells are consecutive along x, so key order is x order) some wave's eight cells hold a cell of
    # at most eight points, a whole-wave cell and a listed one
    kinds = [{0 if c <= 8 else 1 if c <= 4096 else 2 for c in counts[k:k + 8]} for k in range(0, counts.size, 8)]
    assert len(kinds) == 3 and {0, 1, 2} in kinds
    xyz, voxel, origin, _, counts, _ = big("many_cells")
    print(f"many_cells: {counts.size} cells, largest {counts.max()}")
    assert xyz.shape[0] == 200000 and counts.size > 2 * 65536 and counts.max() <= 8
    xyz, voxel, origin, _, counts, _ = big("long_many")
    assert origin is None and counts.tolist() == [4097] * 260
    assert xyz.shape[0] > 1024 * 1024 + 2  # more than 1,024 tiles and box workgroups; the last two past 2^20
    # the last two points alone set the box: without them the lattice moves and cells change
    assert (xyz[-2] < xyz[:-2].min(axis=0)).all() and (xyz[-1] > xyz[:-2].max(axis=0)).all()
    assert V.downsample_ref(xyz[:-2], voxel, origin)[1].tolist() != [4096] + [4097] * 258 + [4096]
    assert V.downsample_ref(xyz[:-1], voxel, origin)[1].tolist() == [4097] * 259 + [4096]  # (the greatest: no cell moves)


@pytest.mark.parametrize("name,bits", [("wide48", 48), ("wide63", 63)])
def test_wide_big_cases_use_both_key_words(name, bits):
    xyz, voxel, origin, _, counts, _ = big(name)
    _, g, _, keys, _ = V.partition(xyz, voxel, origin)
    assert g.tolist() == [2 ** (bits // 3)] * 3 and int(keys.max()).bit_length() == bits and keys.min() == 0
    lo, hi = keys & 0xFFFFFFFF, keys >> 32
    share_lo, share_hi = keys.size - np.unique(lo).size, keys.size - np.unique(hi).size
    print(f"{name}: {keys.size} cells of {xyz.shape[0]} points; {share_lo} share a low word with another cell, "
          f"{share_hi} a high word")
    assert share_lo >= 1000 and share_hi >= 1000
    assert (counts == 2).sum() >= 500 and xyz.shape[0] > 8 * 1024  # (runs of two; several tiles)
    # exact cells: the coordinates are dyadic
    q = xyz / voxel
    assert np.array_equal(q * voxel, xyz) and (np.floor(q) < 2 ** (bits // 3)).all()


@pytest.mark.parametrize("name", V.CASES + V.BIG_CASES)
def test_rule_means_inside_bound(name, icp_amd):
    xyz, voxel, origin, mean, counts, rank = big(name)
    got = V.rule_means(xyz, rank, counts.size)
    gap = np.abs(got.astype(np.longdouble) - mean).astype(np.float64)
    bound = V.mean_bound(xyz, rank, counts)
    print(f"{name}: {counts.size} cells, largest {counts.max()}, worst gap / bound {np.max(gap / np.maximum(bound, 1e-300)):.3f}")
    assert (gap <= bound).all()


def test_rule_means_is_not_a_sequential_sum():
    xyz, _, _, _, counts, rank = big("n4097")
    a, b = V.rule_means(xyz, rank, counts.size), V.sequential_means(xyz, rank, counts.size)
    differ = (a.view(np.uint64) != b.view(np.uint64)).any(axis=1)
    print(f"n4097: {int(differ.sum())} of {counts.size} cells differ in bits from the sequential sum")
    assert differ.sum() > counts.size // 2
    assert not differ[counts <= 2].any()  # (one addition: no order to differ in)


def test_rule_means_restates_the_rule_cell_by_cell():
    """The vectorised form against the rule written out for one cell at a time, on the length switches."""
    xyz, _, _, _, counts, rank = big("lengths")
    got = V.rule_means(xyz, rank, counts.size)
    for v in range(counts.size):
        pts = xyz[rank == v]
        total = np.zeros(3)
        for c in range(0, pts.shape[0], 1024):
            lanes = np.zeros((64, 3))
            for l in range(64):
                for q in pts[c:c + 1024][l::64]:
                    lanes[l] += q
            for o in (32, 16, 8, 4, 2, 1):
                lanes = np.array([lanes[l] + lanes[l ^ o] for l in range(64)])
            total += lanes[0]
        assert np.array_equal((total / pts.shape[0]).view(np.uint64), got[v].view(np.uint64)), counts[v]


def test_rule_means_start_from_plus_zero():
    xyz, voxel, origin = V.negative_zero_case()
    _, counts, rank = V.downsample_ref(xyz, voxel, origin)
    assert counts.tolist() == [3, 70] and np.signbit(xyz[:, 0]).all()
    got = V.rule_means(xyz, rank, 2)
    assert got[:, 0].view(np.uint64).tolist() == [0, 0]
    assert np.signbit(xyz[0, 0] + xyz[1, 0])  # (a sum that starts from its first point keeps the sign)


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


@pytest.mark.parametrize("divs", V.COW_PYRAMIDS)
def test_twin_stops_clear_of_the_threshold(cow, divs):
    """With the default threshold every run of the twin's pyramid stops (or does not) by a margin: no err
    of the iteration before a stop or at it lies within a relative 1e-6 of 1e-5, so an engine that agrees
    with the twin to rounding makes the same iteration counts."""
    m, p = cow
    _, fine_errs, _, levels = V.pyramid_twin(m, p, [V.extent(m) / d for d in divs], 60, 30, 1e-5, V.coarse_rule)
    for what, errs in [("extent/%d" % d, l[3]) for d, l in zip(divs, levels)] + [("fine", fine_errs)]:
        print(f"{divs} {what}: {len(errs)} iterations, the last errs {errs[-2:].tolist()}")
        assert (np.abs(errs[-2:] - 1e-5) > 1e-6 * 1e-5).all()
    assert fine_errs[-1] < 1e-5 and len(fine_errs) == V.PYRAMID_FINE_ITERS


@pytest.mark.parametrize("divs", V.COW_PYRAMIDS)
def test_twin_does_not_feel_the_coarse_means_rounding(cow, divs):
    """The twin on the order rule's coarse clouds (the engine's bits) and on the longdouble means rounded
    to fp64: the gap stays below a hundredth of the tolerances tests/test_gpu_pyramid.py compares the engine
    with the twin at (errs rtol 1e-9, R 1e-9, t and points 1e-9 x max |m|).  Measured: errs 8.5e-15
    (extent/16) and 8.6e-16 (extent/8, extent/16) relative; points 1.3e-15 and 1.8e-15; R 1.1e-15 and
    1.9e-15.  (With eight fine iterations err sits at its floor of 2.3e-11 from the third on and the errs'
    gap is 1.3e-12 and 6.7e-12: voxel_ref.PYRAMID_FINE_ITERS says why the tests run two.)"""
    m, p = cow
    voxels = [V.extent(m) / d for d in divs]
    a = V.pyramid_twin(m, p, voxels, V.PYRAMID_FINE_ITERS, V.PYRAMID_LEVEL_ITERS, -1.0, V.coarse_rule)
    b = V.pyramid_twin(m, p, voxels, V.PYRAMID_FINE_ITERS, V.PYRAMID_LEVEL_ITERS, -1.0, V.coarse_longdouble)
    scale = float(np.abs(m).max())
    g_err = float(np.max(np.abs(a[1] - b[1]) / b[1]))
    g_pts = float(np.abs(a[0] - b[0]).max())
    g_s, g_R, g_t = abs(a[2][0] - b[2][0]), float(np.abs(a[2][1] - b[2][1]).max()), float(np.abs(a[2][2] - b[2][2]).max())
    print(f"{divs}: rule against longdouble coarse means: errs {g_err:.3e} relative, points {g_pts:.3e}, "
          f"s {g_s:.3e}, R {g_R:.3e}, t {g_t:.3e} (max |m| = {scale:.4g})")
    assert [l[:3] for l in a[3]] == [l[:3] for l in b[3]] and len(a[1]) == len(b[1]) == V.PYRAMID_FINE_ITERS
    assert g_err < 1e-11 and g_s < 1e-11 and g_R < 1e-11
    assert g_pts < 1e-11 * scale and g_t < 1e-11 * scale


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
