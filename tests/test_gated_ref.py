"""CPU checks of the gated loop's reference (tests/gated_ref.py): without a gate it is the
oracle's loop bit for bit, and every input of tests/test_gpu_gated.py satisfies the precondition
its exact comparisons rest on -- no pair within 1e-6 (relative, squared distance) of the gate, so
that an engine trajectory that differs from the oracle's in the last bits cannot flip a gate
decision -- with the K lists the issue quotes."""
import numpy as np
import pytest

import gated_ref as G


@pytest.mark.parametrize("scene,iters", [("cow_tr1", 7), ("cow_tr2", 12)])
def test_ungated_reference_is_the_oracle_loop(oracle, scene, iters):
    ref, tr1, tr2 = G.load_cow(oracle)
    p = tr1 if scene == "cow_tr1" else tr2
    want = oracle.icp(ref, p, 20)
    got = G.gated_ref(oracle, ref, p, np.inf, 20)
    assert want["iterations"] == iters and got["iterations"] == iters
    np.testing.assert_array_equal(got["err"], want["err"])
    np.testing.assert_array_equal(got["new_p"], want["new_p"])
    assert got["K"] == [ref.shape[0]] * iters and got["mask"].all() and got["status"] == "ok"


@pytest.mark.parametrize("n", list(G.SIZES))
def test_size_cases(oracle, n):
    _m, _p, _d, r = G.reference(oracle, ("size", n))
    print(n, r["K"], r["margin"])
    assert r["K"] == [G.SIZES[n]] * G.SIZES_ITERS
    assert r["margin"] >= 0.96 and r["status"] == "ok"


@pytest.mark.parametrize("n,dmax", list(G.BITES))
def test_biting_cases(oracle, n, dmax):
    _m, _p, _d, r = G.reference(oracle, ("bite", n, dmax))
    print(n, dmax, r["K"], r["margin"])
    assert (r["K"][0], r["K"][-1]) == G.BITES[(n, dmax)] and len(r["K"]) == G.BITES_ITERS
    assert r["margin"] > 1e-6
    assert len(set(r["K"])) > 2  # the gate moves


def test_partial_overlap_case(oracle):
    m, p, _d, r = G.reference(oracle, ("partial",))
    print(r["K"], r["margin"])
    assert m.shape == p.shape == (2177, 3)
    assert r["K"][0] == 712 and max(r["K"]) == 1530 and r["K"][-1] == 1527 and len(r["K"]) == 20
    assert r["margin"] > 1e-6


def test_clump_case(oracle):
    m, p, dmax, r = G.reference(oracle, ("clump",))
    print(r["K"], r["err"], r["margin"])
    assert r["iterations"] == 16 and r["K"] == [2201] + [2203] * 15
    assert r["err"][-1] < 1e-5 and np.all(r["err"][:-1] >= 1e-5)
    want = np.ones(p.shape[0], dtype=bool)
    want[-700:] = False
    np.testing.assert_array_equal(r["mask"], want)  # exactly "not the clump"
    assert r["margin"] > 1e-6
    # the same input ungated does not converge in 30 iterations
    u = oracle.icp(m, p, 30)
    assert u["iterations"] == 30 and u["err"][-1] > 1e-2
    # the 3-iteration prefix (state hygiene, ranks) is the same trajectory
    _m, _p, _d, r3 = G.reference(oracle, ("clump", 3))
    np.testing.assert_array_equal(r3["err"], r["err"][:3])


def test_too_few_case(oracle):
    m, p = G.synth(300, 1, 0.0)
    p = p + np.array([10.0, 0.0, 0.0])
    r = G.gated_ref(oracle, m, p, 1.0, 5, -1.0)
    assert r["status"] == "few" and r["K"] == [] and r["K_fail"] == 0 and r["iterations"] == 0
    np.testing.assert_array_equal(r["new_p"], p)
