"""tests/eval_ref.py pinned on the CPU: the numpy restatement of icp_evaluate (include/icp_capi.h) that
tests/test_gpu_eval.py compares the device with gives the counts the cases were chosen for, its two forms
of the information matrix agree, and the matrix has the properties a pose graph relies on."""
import numpy as np
import pytest

import eval_ref as E


@pytest.mark.parametrize("name", E.CASES)
def test_reference_counts(oracle, name):
    for d, K, Km in E.COUNTS[name]:
        m, p, md, r = E.reference(name, d, oracle.load_matrix)
        print(name, "nm", m.shape[0], "np", p.shape[0], "max_dist", md, "K", r["correspondences"], "K_m",
              r["model_correspondences"], "fitness", r["fitness"], "rmse", r["inlier_rmse"], "max d2", r["max_inlier_d2"])
        assert r["correspondences"] == K
        if Km is not None:
            assert r["model_correspondences"] == Km
        assert r["scene_points"] == p.shape[0] and r["model_points"] == m.shape[0]
        assert np.all((r["idx"] >= 0) == np.isfinite(r["d2"]))
        assert int((r["idx"] >= 0).sum()) == K


def test_what_the_cases_exercise(oracle):
    m, p, _, r = E.reference("lattice_tie", 1.0)
    assert np.all(r["d2"] == 0.75)  # an eight-way exact tie: the first minimum is the lowest index
    lo = np.minimum(np.floor(p), 8 - 1)  # the corner (i, j, k) of the query's cell, kept inside the lattice
    want = (np.minimum(lo[:, 0], 7) * 81 + np.minimum(lo[:, 1], 7) * 9 + np.minimum(lo[:, 2], 7)).astype(np.int32)
    inside = np.all(p < 8, axis=1)
    np.testing.assert_array_equal(r["idx"][inside], want[inside])
    _, _, _, r = E.reference("lattice_edge", 0.5)
    assert np.all(r["d2"] == 0.25) and r["fitness"] == 1.0  # d2 == D is kept
    _, _, _, r = E.reference("lattice_edge", 0.49)
    assert r["correspondences"] == 0 and r["fitness"] == 0.0 and r["inlier_rmse"] == 0.0
    assert r["max_inlier_d2"] == 0.0 and not r["information"].any() and np.all(r["idx"] == -1)
    m, p, _, r = E.reference("far", 0.2)
    assert np.all(r["idx"][-8:] == -1) and np.all(r["model_idx"][-8:] == -1)  # the eight points at x = 40 never pair
    m, p, _, r = E.reference("shell", 0.3)
    assert np.all(r["d2"][-40:] == 0.0) and np.all(r["idx"][-40:] == np.arange(40))  # 40 points at distance 0
    lo_, hi_ = m.min(axis=0), m.max(axis=0)
    for a in range(3):  # queries outside the model's box on every side
        assert (p[:, a] < lo_[a]).any() and (p[:, a] > hi_[a]).any()
    m, p, _, r = E.reference("synth257", 0.08)
    assert (p[:, 0] > m[:, 0].max() + 1).sum() == 64  # the quarter of outliers sits outside the model's box
    _, _, _, r = E.reference("cow_partial", float("inf"), oracle.load_matrix)
    assert abs(r["max_inlier_d2"] - 1.47755) < 5e-6  # the one-sided Hausdorff distance squared
    assert r["fitness"] == 1.0 and r["model_fitness"] == 1.0


@pytest.mark.parametrize("name", E.CASES)
def test_information_two_ways(oracle, name):
    for d, _K, _Km in E.COUNTS[name]:
        m, p, md, r = E.reference(name, d, oracle.load_matrix)
        A, B = r["information"], r["information_bound"]
        A2 = E.information_pairwise(m, r["idx"])
        n = p.shape[0]
        print(name, md, "largest |A - A2| / bound", float(np.max(np.abs(A - A2) / np.where(B > 0, B, 1.0))))
        assert np.all(np.abs(A - A2) <= (n + 4) * 2.0 ** -53 * B)
        np.testing.assert_array_equal(A, A.T)


def test_information_of_synth257_is_positive_definite():
    for d in E.SYNTH_DISTS:
        _, _, _, r = E.reference("synth257", d)
        A = r["information"]
        np.testing.assert_array_equal(A, A.T)
        w = np.linalg.eigvalsh(A)
        print(d, "eigenvalues", w)
        assert w.min() > 0
