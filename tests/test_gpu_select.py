"""icp_select_kth (icp_select.hip: the radix select that cuts a trimmed icp_run) against np.sort on
the keys (tests/trim_ref.py key_of), compared as uint64: the result is one of the input's values, so
the comparison is exact, NaN and the zeros' signs included."""
import numpy as np
import pytest

import trim_ref as TR

pytestmark = pytest.mark.gpu

# the wave tail, one workgroup, kRedSingle, the first multi-workgroup counts; 1,048,577 crosses the
# grid-stride bound of a red_blocks-sized launch
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65537, 1048577)
PATTERNS = ("uniform", "equal", "two", "chain", "powers", "mix")


def pattern(name, n):
    r = np.random.default_rng(1000 + n)
    if name == "uniform":  # positives
        return r.uniform(0.0, 10.0, n)
    if name == "equal":
        return np.full(n, 3.25)
    if name == "two":
        return r.choice(np.array([1.5, 2.5]), n)
    if name == "chain":  # 1, nextafter(1), ...: keys that differ only in the lowest digits
        return r.permutation(1.0 + np.arange(n) * 2.0 ** -52)
    if name == "powers":  # 0, every power of two from the smallest denormal to 2^1023, +inf: the highest digits
        pool = np.concatenate([[0.0], np.ldexp(1.0, np.arange(-1074, 1024)), [np.inf]])
        return pool[r.integers(0, pool.size, n)] if n < pool.size else r.permutation(np.resize(pool, n))
    v = r.standard_normal(n)  # negatives, both zeros, NaNs of both signs, both infinities
    special = np.array([-0.0, 0.0, np.nan, -np.nan, np.inf, -np.inf, -5e-324, 5e-324])
    where = r.random(n) < 0.3
    v[where] = special[r.integers(0, special.size, int(where.sum()))]
    return v


def ranks(n):
    return sorted({min(max(k, 1), n) for k in (1, 2, n // 2, n - 1, n)})


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_kth_is_the_sorted_keys(icp_lib, n, name):
    v = pattern(name, n)
    want = np.sort(TR.key_of(v))
    for k in ranks(n):
        got = icp_lib.select_kth(v, k)
        gk = TR.key_of(np.array([got]))[0]
        assert gk == want[k - 1], (n, name, k, got, hex(int(gk)), hex(int(want[k - 1])))
        if np.isnan(got):  # (returned as a quiet NaN)
            assert np.array([got]).view(np.uint64)[0] & np.uint64(0x7FF8000000000000) == np.uint64(0x7FF8000000000000)


def test_chain_keys_differ_in_the_lowest_digit_only():
    k = TR.key_of(pattern("chain", 257))
    assert len(set((k >> np.uint64(9)).tolist())) == 1 and len(set(k.tolist())) == 257


def test_argument_errors(icp_lib):
    amd = icp_lib
    v = np.arange(8.0)
    for vals, k in ((v, 0), (v, 9), (v[:0], 1), (v, -1)):
        with pytest.raises(amd.ICPError) as ei:
            amd.select_kth(vals, k)
        assert ei.value.code == amd.ICP_E_ARG
    out = np.zeros(1)
    import ctypes as C
    dp = C.POINTER(C.c_double)
    assert amd.lib().icp_select_kth(0, None, 8, 1, out.ctypes.data_as(dp)) == amd.ICP_E_ARG
    assert amd.lib().icp_select_kth(0, v.ctypes.data_as(dp), 8, 1, None) == amd.ICP_E_ARG
    assert amd.lib().icp_select_kth(0, v.ctypes.data_as(dp), 2 ** 31, 1, out.ctypes.data_as(dp)) == amd.ICP_E_ARG
    assert amd.select_kth(v, 3) == 2.0


def test_two_calls_give_the_same_bits(icp_lib):
    v = pattern("mix", 65537)
    for k in (1, 30000, 65537):
        a = np.array([icp_lib.select_kth(v, k), icp_lib.select_kth(v, k)])
        assert a.view(np.uint64)[0] == a.view(np.uint64)[1]
