"""CPU checks of the trimmed loop's reference (tests/trim_ref.py): with f = 1 it is the oracle's
loop bit for bit, and every multi-iteration input of tests/test_gpu_trim.py satisfies the
precondition its exact comparisons rest on -- the (T+1)-th distance no closer than 1e-6 (relative,
squared) to the cut, and no pair within that of a gate -- with the K lists the issue quotes."""
import numpy as np
import pytest

import gated_ref as G
import trim_ref as TR


def test_untrimmed_reference_is_the_oracle_loop(oracle):
    ref, _tr1, tr2 = G.load_cow(oracle)
    want = oracle.icp(ref, tr2, 20)
    got = TR.trimmed_ref(oracle, ref, tr2, 1.0, 0.0, 20)
    assert got["iterations"] == want["iterations"] == 12
    np.testing.assert_array_equal(got["err"], want["err"])
    np.testing.assert_array_equal(got["new_p"], want["new_p"])
    assert got["K"] == [ref.shape[0]] * 12 and got["mask"].all() and got["status"] == "ok"


def test_trim_count_is_the_truncated_fp64_product():
    assert [TR.trim_count(0.7, n) for n in (5, 63, 64, 65, 257, 4096, 4097, 9001)] == [3, 44, 44, 45, 179, 2867, 2867, 6300]
    assert TR.trim_count(0.5, 514) == 257 and TR.trim_count(0.4987, 514) == 256
    assert TR.trim_count(1e-9, 10) == 1 and TR.trim_count(0.999999, 4097) == 4096


def test_keys_order_the_doubles():
    v = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan])
    k = TR.key_of(v)
    assert np.all(k[1:] > k[:-1])
    assert TR.key_of(np.array([-np.nan]))[0] == k[-1]  # (every NaN: one key, the last)


@pytest.mark.parametrize("n", list(TR.SIZES))
def test_size_cases(oracle, n):
    _m, _p, _f, _d, _it, _th, r = TR.reference(oracle, ("size", n))
    print(n, r["K"], r["C"], r["margin"])
    assert r["K"] == [TR.SIZES[n]] * TR.SIZES_ITERS and r["status"] == "ok"
    assert r["margin"] > 1e-6


def test_too_few_case(oracle):
    m, p = G.synth(5, 105, 0.25)
    r = TR.trimmed_ref(oracle, m, p, TR.SIZES_F, 0.0, TR.SIZES_ITERS, -1.0)
    assert r["T"] == 3 and r["status"] == "few" and r["K"] == [] and r["iterations"] == 0
    np.testing.assert_array_equal(r["new_p"], p)


@pytest.mark.parametrize("n,f", list(TR.NOISY))
def test_noisy_cases(oracle, n, f):
    _m, _p, _f, _d, _it, _th, r = TR.reference(oracle, ("noisy", n, f))
    print(n, f, r["K"], r["C"], r["margin"])
    assert r["K"] == [TR.NOISY[(n, f)]] * TR.NOISY_ITERS
    assert r["margin"] > 1e-6
    assert r["C"][-1] < r["C"][0]  # the cut falls as the clouds meet


def test_gate_and_trim_each_bind_in_turn(oracle):
    _m, _p, _f, dmax, _it, _th, r = TR.reference(oracle, ("both",))
    print(r["K"], r["C"], r["margin"])
    assert r["K"] == TR.BOTH_K
    D = dmax * dmax
    assert all(c > D for c in r["C"][:4]) and all(c < D for c in r["C"][4:])
    assert r["margin"] > 1e-6


def test_partial_overlap_case(oracle):
    m, p, _f, _d, _it, _th, r = TR.reference(oracle, ("partial",))
    print(r["K"], r["err"], r["margin"])
    assert m.shape == p.shape == (2177, 3)
    assert r["K"] == [TR.PARTIAL_K] * TR.PARTIAL_ITERS
    assert r["err"][-1] < 1e-3 and r["margin"] > 1e-6


@pytest.mark.parametrize("key", [("clump",), ("clump_gate",)])
def test_clump_cases(oracle, key):
    m, p, _f, _d, _it, _th, r = TR.reference(oracle, key)
    print(r["K"], r["err"], r["margin"])
    assert r["iterations"] == TR.CLUMP_ITERS and r["K"] == [TR.CLUMP_K] * TR.CLUMP_ITERS
    assert r["err"][-1] < 1e-5 and np.all(r["err"][:-1] >= 1e-5)
    assert not r["mask"][-700:].any()  # none of the clump
    assert r["margin"] > 1e-6


def test_ties_are_kept_whole(oracle):
    m, p = G.synth(257, 357, 0.25)
    p2 = np.repeat(p, 2, axis=0)
    a = TR.trimmed_ref(oracle, m, p2, 0.5, 0.0, 1, -1.0)
    b = TR.trimmed_ref(oracle, m, p2, 0.4987, 0.0, 1, -1.0)
    assert (a["T"], a["K"]) == (257, [258]) and (b["T"], b["K"]) == (256, [256])
