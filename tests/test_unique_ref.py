"""CPU checks of the one-to-one loop's reference (tests/unique_ref.py): every multi-iteration input of
tests/test_gpu_unique.py satisfies the precondition its exact comparisons rest on -- at every model
point chosen more than once the second-smallest d2 is no closer than 1e-6 (relative) to the smallest,
no pair within that of a gate, and the (T+1)-th distance no closer than that to a trim's cut -- with
the reference's own K lists pinned."""
import numpy as np
import pytest

import gated_ref as G
import unique_ref as U


def test_mask_and_margin_on_a_hand_case():
    idx = np.array([0, 0, 1, 2, 2, 2, 3])
    d2 = np.array([4.0, 1.0, 9.0, 2.0, 2.0, 8.0, np.nan])
    assert U.unique_mask(idx, d2, 5).tolist() == [False, True, True, True, True, False, False]  # the tie whole, no NaN
    assert U.unique_margin(idx, d2) == 0.0  # the tie at model point 2
    assert U.unique_margin(idx[:3], d2[:3]) == 0.75  # (4 - 1) / 4
    assert U.unique_margin(np.array([0, 1, 2]), np.ones(3)) == np.inf


@pytest.mark.parametrize("n", list(U.SIZES))
def test_size_cases(oracle, n):
    _m, _p, _d, _f, _it, r = U.reference(oracle, ("size", n))
    print(n, r["K"], r["margin"])
    assert r["K"] == U.SIZES[n] and r["status"] == "ok"
    assert r["margin"] > 1e-6


def test_partial_overlap_converges_only_one_to_one(oracle):
    m, p, _d, _f, iters, r = U.reference(oracle, ("partial",))
    print(r["K"], r["err"], r["margin"])
    assert m.shape == p.shape == (2177, 3)
    assert r["K"] == U.PARTIAL_K and r["K"][15:] == [1451] * 5
    assert r["err"][-1] < 1e-9 and abs(r["s"] - 1.0) < 1e-9
    assert oracle.icp(m, p, iters)["err"][-1] > 0.05  # the plain loop stays off
    assert r["margin"] > 1e-6


def test_clump_case(oracle):
    _m, _p, _d, _f, _it, r = U.reference(oracle, ("clump",))
    print(r["K"], r["err"], r["margin"])
    assert r["K"] == U.CLUMP_K
    assert r["margin"] > 1e-6


@pytest.mark.parametrize("n,how", list(U.NOISY))
def test_noisy_cases_with_the_gate_and_the_trim(oracle, n, how):
    _m, _p, dmax, f, _it, r = U.reference(oracle, ("noisy", n, how))
    print(n, how, dmax, f, r["K"], r["margin"])
    assert r["K"] == U.NOISY[(n, how)]
    assert r["margin"] > 1e-6


def test_the_first_iteration_is_a_prefix(oracle):
    for key in U.MULTI:
        one, many = U.reference(oracle, key, iters=1)[5], U.reference(oracle, key)[5]
        assert one["K"] == many["K"][:1]


def test_ties_are_kept_whole(oracle):
    m, p = G.synth(257, 357, 0.25)
    a = U.one_to_one_ref(oracle, m, p, 1, -1.0)
    b = U.one_to_one_ref(oracle, m, np.repeat(p, 2, axis=0), 1, -1.0)
    assert a["K"] == [178] and b["K"] == [356]
    np.testing.assert_array_equal(b["mask"][0::2], a["mask"])
    np.testing.assert_array_equal(b["mask"][1::2], a["mask"])


def test_too_few(oracle):
    m, p = U.few_case()
    r = U.one_to_one_ref(oracle, m, p, 3, -1.0)
    assert r["status"] == "few" and r["K"] == [] and r["K_fail"] == 3
    np.testing.assert_array_equal(r["new_p"], p)


def test_one_address(oracle):
    m, p = U.one_address()
    r = U.one_to_one_ref(oracle, m, p, 2, -1.0)
    assert np.bincount(r["idx"], minlength=8).max() >= 4090 - 7 and r["K"] == [8, 8]
    assert r["margin"] > 1e-6
