"""tests/global_ref.py pinned on the CPU: the numpy restatement of icp_fpfh, icp_match_features and
icp_ransac_pose that tests/test_gpu_global.py compares the kernels with, and the conditions that
comparison rests on (the f1 filter, the count's bracket, the seed of the purpose test).
"""
import numpy as np
import pytest

import global_ref as G
import normals_ref as N
import plane_ref as P
import voxel_ref as V

_REF = {}


def descriptor(name, icp_lib):
    """(x, k, normals, fpfh_ref(...)) of a named cloud with the numpy estimator's normals: once, shared"""
    if name not in _REF:
        x, k = G.cloud(name, icp_lib.load_matrix)
        nrm = N.normals_ref(x, min(G.K_NORMALS, x.shape[0]))["normals"]
        _REF[name] = (x, k, nrm, G.fpfh_ref(x, nrm, k))
    return _REF[name]


def test_descriptors_are_invariant_under_a_rigid_motion():
    x, nrm = P.ellipsoid(300, 41)
    R = P.rot((0.2, 1.0, -0.7), 73.0)
    a = G.fpfh_ref(x, nrm, 24)
    b = G.fpfh_ref(x @ R.T + np.array([3.0, -1.0, 0.5]), nrm @ R.T, 24)
    assert np.array_equal(a["idx"], b["idx"])  # (a generic cloud: no near-ties in d2)
    assert a["fpfh_ok"].all() and b["fpfh_ok"].all()  # (no f1 near a bin edge: every row is compared)
    # the histograms' counts are equal; the weights 1 / d2 move by rounding only
    assert np.array_equal(a["spfh"], b["spfh"])
    assert np.abs(a["fpfh"] - b["fpfh"]).max() <= 1e-9


@pytest.mark.parametrize("name", G.FPFH_CASES)
def test_thirds_sum_to_200_and_the_filter_keeps_the_rows(name, icp_lib):
    x, k, nrm, ref = descriptor(name, icp_lib)
    thirds = ref["fpfh"].reshape(-1, 3, 11).sum(axis=2)
    spfh_thirds = ref["spfh"].reshape(-1, 3, 11).sum(axis=2)
    some = ref["counted"] > 0
    print(f"{name}: n {x.shape[0]}, k {k}, rows with a counted pair {int(some.sum())}, "
          f"left out by the filter {int((~ref['fpfh_ok']).sum())}")
    assert np.abs(spfh_thirds[some] - 100.0).max(initial=0.0) <= 1e-9
    # each third of a row with a counted pair: its own SPFH's 100 and the weighted neighbours' 100
    assert np.abs(thirds[some] - 200.0).max(initial=0.0) <= 1e-9
    assert (ref["fpfh"][~some] == 0.0).all()
    assert (~ref["fpfh_ok"]).mean() <= G.FILTER_MAX  # a condition, not a measurement


def test_line_gives_zero_rows(icp_lib):
    _, _, nrm, ref = descriptor("line", icp_lib)
    assert (nrm == 0.0).all() and (ref["fpfh"] == 0.0).all() and (ref["counted"] == 0).all()


def test_duplicates_are_skipped(icp_lib):
    x, k, _, ref = descriptor("duplicates", icp_lib)
    assert (ref["d2"][:, 1] == 0.0).sum() >= 80  # (a duplicated point lists its twin at distance 0)
    assert np.isfinite(ref["fpfh"]).all()


@pytest.mark.parametrize("C", [3, 4, 5])
def test_the_draw_gives_three_distinct_pairs(C):
    ids = G.draw(12345, 5000, C)
    assert ids.min() >= 0 and ids.max() < C
    assert (ids[:, 0] != ids[:, 1]).all() and (ids[:, 0] != ids[:, 2]).all() and (ids[:, 1] != ids[:, 2]).all()
    # every ordered triple occurs: the three draws are uniform over what is left
    assert len({tuple(r) for r in ids.tolist()}) == C * (C - 1) * (C - 2)
    # a pure function of (seed, h, C), restated with Python's integers
    M = (1 << 64) - 1

    def sm(v):
        v ^= v >> 30
        v = (v * 0xBF58476D1CE4E5B9) & M
        v ^= v >> 27
        v = (v * 0x94D049BB133111EB) & M
        return v ^ (v >> 31)
    for h in (0, 1, 4999):
        z = [sm((12345 + (3 * h + r + 1) * 0x9E3779B97F4A7C15) & M) for r in range(3)]
        i0 = z[0] % C
        i1 = z[1] % (C - 1)
        i1 += i1 >= i0
        i2 = z[2] % (C - 2)
        i2 += i2 >= min(i0, i1)
        i2 += i2 >= max(i0, i1)
        assert ids[h].tolist() == [i0, i1, i2]


def test_match_rule():
    r = np.random.default_rng(3)
    fb = r.uniform(0, 100, (40, G.DIM))
    fb[17] = fb[5]  # a duplicated row: the lowest index wins
    fa = fb[[5, 17, 30]].copy()
    fa = np.concatenate([fa, np.full((1, G.DIM), np.nan)])
    idx, d = G.match_ref(fa, fb)
    assert idx.tolist() == [5, 5, 30, -1] and d[:3].tolist() == [0.0, 0.0, 0.0] and np.isnan(d[3])
    fb[0, 3] = np.nan  # a NaN row never wins
    assert (G.match_ref(r.uniform(0, 100, (9, G.DIM)), fb)[0] > 0).all()
    assert G.mutual(np.array([1, 0, -1, 0]), np.array([1, 0])).tolist() == [0, 1]


@pytest.mark.parametrize("name", list(G.RANSAC_CASES))
def test_the_count_bracket_is_narrow(name, icp_lib):
    p, q, H, seed, max_dist, edge = G.ransac_case(name)
    ref = G.ransac_ref(p, q, H, seed, max_dist, edge, icp_lib.horn_solve)
    print(f"{name}: kept {int(ref['kept'].sum())} of {H}, bracket open for {ref['open']}")
    assert ref["kept"].any() and (ref["lo"] <= ref["hi"]).all()
    assert ref["open"] <= G.BRACKET_MAX * H  # a condition, not a measurement


def test_planted_pose_is_found_by_the_reference(icp_lib):
    p, q, R, t = G.planted()
    ref = G.ransac_ref(p, q, 2000, 1, 1e-6, 0.9, icp_lib.horn_solve)
    h, count = G.winner(ref["mid"])
    assert count >= 120
    Rw, tw = ref["poses"][h]
    assert np.abs(Rw - R).max() <= 1e-9 and np.abs(tw - t).max() <= 1e-9


def test_the_purpose_seed_lands_within_5_degrees(icp_lib):
    """The condition of the GPU purpose test, checked with the reference alone: the cow against itself turned
    120 degrees, voxel 0.12, the defaults (k 16 / 32, mutual matches, H = 100000, 1.5 voxel, 0.9)."""
    m, p, R_true, t_true = G.cow_pair(icp_lib.load_matrix)
    mc, pc = V.coarse_rule(m, G.COW_VOXEL), V.coarse_rule(p, G.COW_VOXEL)
    fm = G.fpfh_ref(mc, N.normals_ref(mc, 16)["normals"], 32)["fpfh"]
    fp = G.fpfh_ref(pc, N.normals_ref(pc, 16)["normals"], 32)["fpfh"]
    pm, mp = G.match_ref(fp, fm)[0], G.match_ref(fm, fp)[0]
    keep = G.mutual(pm, mp)
    ref = G.ransac_ref(pc[keep], mc[pm[keep]], 100000, G.PURPOSE_SEED, 1.5 * G.COW_VOXEL, 0.9, icp_lib.horn_solve)
    h, count = G.winner(ref["mid"])
    Rw, tw = ref["poses"][h]
    ang = G.angle_deg(Rw, R_true)
    print(f"coarse {mc.shape[0]} / {pc.shape[0]}, matches {keep.size}, kept {int(ref['kept'].sum())}, "
          f"winner h {h} with {count} inliers, {ang:.3f} degrees and |dt| {np.abs(tw - t_true).max():.4f} from the truth")
    assert ang < 5.0
