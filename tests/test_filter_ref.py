"""tests/filter_ref.py pinned on the CPU: the numpy restatement of icp_filter_statistical and
icp_filter_radius (include/icp_capi.h) that tests/test_gpu_filter.py compares the device with.

1. Every statistical case the GPU test runs keeps its mean distances clear of the threshold: the least
   |dbar_j - T| / T is at least 1e-9.  A condition on the inputs, not a tolerance: the device's dbar may
   differ from the reference's by a few ulp and T by n 2^-53, and with this margin neither can move a
   point across T, so the masks are compared exactly.
2. What the filter is for.  cow_ref with n / 50 planted points (uniform in its box scaled by 1.5, seed
   20): the reference removes at least 9 in 10 of the planted points and at most 1 in 20 of the cow's
   own.  Measured on the reference: (k, ratio) = (16, 2.0) removes 47 of 58 planted (81 %) and 0 of 2,903
   of the cow's, which misses the first condition; (16, 1.0) removes 53 of 58 (91 %) and 100 of 2,903
   (3.4 %) and is the pair this test pins.
3. The fp64 reference's mu and sigma lie within 1e-12 relative of the same sums in np.longdouble.
"""
import numpy as np
import pytest

import filter_ref as F


@pytest.mark.parametrize("name", F.CASES)
def test_thresholds_are_clear_of_every_mean(oracle, name):
    for prm in F.STAT_PARAMS[name]:
        m, r = F.reference("stat", name, prm, oracle.load_matrix)
        print(name, "n", m.shape[0], "(k, ratio)", prm, "T", r["T"], "kept", int(r["mask"].sum()), "margin", r["margin"])
        assert r["margin"] >= F.MARGIN
        assert r["mean"].shape == (m.shape[0],) and np.all(r["mean"] >= 0)


def test_reference_is_the_rule_on_small_inputs():
    # four collinear points at 0, 1, 3, 7 and k = 2: the lists and the means by hand
    m = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    r = F.statistical(m, 2, 1.0)
    np.testing.assert_array_equal(r["mean"], [(0 + 1 + 3) / 2, (0 + 1 + 2) / 2, (0 + 2 + 3) / 2, (0 + 4 + 6) / 2])
    mu = (2.0 + 1.5 + 2.5 + 5.0) / 4
    assert r["mu"] == mu and r["sigma"] == np.sqrt(((np.array([2.0, 1.5, 2.5, 5.0]) - mu) ** 2).sum() / 3)
    np.testing.assert_array_equal(r["mask"], [True, True, True, False])
    np.testing.assert_array_equal(F.radius_counts(m, 2.0), [2, 3, 2, 1])  # (1 and 3: d2 == r2 counts)
    d, _ = F.reference("stat", "duplicates", (F.K, 2.0))
    _, rd = F.reference("stat", "duplicates", (F.K, 2.0))
    equal = np.all(d == d[5], axis=1)
    assert int(equal.sum()) == 20 >= F.K + 2
    np.testing.assert_array_equal(rd["mean"][equal], 0.0)


def test_lattice_counts_at_radius_one_include_the_ties():
    m, c = F.reference("radius", "lattice", 1.0)
    inner = np.all((m > 0) & (m < 8), axis=1)
    assert np.all(c[inner] == 7) and c.min() == 4  # (six neighbours at d2 == r2 and the point; a corner has three)


def test_cow_clutter_shares(oracle):
    m, planted = F.cow_clutter(oracle.load_matrix)
    assert int(planted.sum()) == 58 and m.shape[0] == 2961
    _, r2 = F.reference("stat", "cow_clutter", (16, 2.0), oracle.load_matrix)
    _, r1 = F.reference("stat", "cow_clutter", (16, 1.0), oracle.load_matrix)
    gone2, gone1 = ~r2["mask"], ~r1["mask"]
    print("(16, 2.0): planted removed", int((gone2 & planted).sum()), "cow's removed", int((gone2 & ~planted).sum()))
    print("(16, 1.0): planted removed", int((gone1 & planted).sum()), "cow's removed", int((gone1 & ~planted).sum()))
    assert (int((gone2 & planted).sum()), int((gone2 & ~planted).sum())) == (47, 0)  # (misses 9 in 10)
    assert (int((gone1 & planted).sum()), int((gone1 & ~planted).sum())) == (53, 100)
    assert (gone1 & planted).sum() >= 0.9 * planted.sum()
    assert (gone1 & ~planted).sum() <= 0.05 * (~planted).sum()


@pytest.mark.parametrize("name", ["ell257", "ell4097", "cow_clutter", "far"])
def test_fp64_moments_sit_on_extended_precision(oracle, name):
    m = F.cloud(name, oracle.load_matrix)
    _, r = F.reference("stat", name, (F.K, 2.0), oracle.load_matrix)
    x = r["mean"].astype(np.longdouble)
    mu = x.sum() / np.longdouble(x.size)
    sigma = np.sqrt(((x - mu) * (x - mu)).sum() / np.longdouble(x.size - 1))
    e_mu, e_sigma = abs(float((mu - r["mu"]) / mu)), abs(float((sigma - r["sigma"]) / sigma))
    print(name, "n", m.shape[0], "rel. difference of mu", e_mu, "of sigma", e_sigma)
    assert e_mu <= 1e-12 and e_sigma <= 1e-12
