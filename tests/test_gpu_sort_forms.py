"""Every form of the engine's radix sort (icp_sort.hip, through icp_sort_pairs) against numpy's
stable argsort of the masked keys.

The sort's workgroup is 4, 8 or 16 waves over one 4,096-item tile (ICP_SORT_WAVES), and a table of
at most ICP_SORT_PREFIX tiles (default 256: n <= 2^20) has each scatter workgroup sum its digits'
prefixes itself instead of a sort_rows_kernel launch (ICP_SORT_PREFIX=0: always the launch).  The
form before is ICP_SORT_WAVES=4 ICP_SORT_PREFIX=0.  Which lane holds which item changes with the
form; the order may not: ascending (key & mask), ties in input order.  The switches are read once,
so each form runs in a subprocess of its own, which checks every case and prints a count.

Cases per form: sizes 1, 63, 64, 4,095, 4,096, 4,097, 2^16 + 37 and 2^21 + 4,097 (513 tiles: past
the prefix bound, the sort_rows form that 8M-point models take); 1, 7, 8, 9, 19, 20, 21, 24
and 32 bits (1 to 4 passes, both ping-pong ends, partial digits); random keys with bits above
`bits` set (ignored), all keys equal, one digit holding all but one item (in every pass), sorted
and reversed.  The largest size runs the four structured inputs at 20 and 24 bits only (the
model's and the scene's key widths), to keep a form within a few seconds.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import icp_amd
sizes = [1, 63, 64, 4095, 4096, 4097, (1 << 16) + 37, (1 << 21) + 4097]
bit_counts = [1, 7, 8, 9, 19, 20, 21, 24, 32]
checked = 0
for n in sizes:
    big = n > (1 << 20)
    rng = np.random.default_rng(n)
    base = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    for bits in bit_counts:
        mask = np.uint32((1 << bits) - 1)
        inputs = {"random": base}
        if not big or bits in (20, 24):
            lone = np.full(n, 0x5A5A5A5A, dtype=np.uint32)
            lone[n // 2] ^= np.uint32(0xFFFFFFFF)  # (differs in every digit of every pass)
            srt = np.sort(base & mask) | (base & ~mask)
            inputs.update(equal=np.full(n, base[0], dtype=np.uint32), lone=lone, sorted=srt,
                          reversed=srt[::-1].copy())
        for name, keys in inputs.items():
            order, out = icp_amd.sort_pairs(keys, bits)
            want = np.argsort((keys & mask).astype(np.int64), kind="stable").astype(np.int32)
            assert np.array_equal(order, want), (n, bits, name, "order")
            assert np.array_equal(out, keys[want]), (n, bits, name, "keys")
            checked += 1
print("sort forms ok", checked)
"""

# 7 sizes x 9 bit counts x 5 inputs, and the largest: 9 random + 2 bit counts x 4 structured
N_CASES = 7 * 9 * 5 + 9 + 2 * 4


@pytest.mark.parametrize("prefix", ["256", "0"])
@pytest.mark.parametrize("waves", ["4", "8", "16"])
def test_sort_form_matches_stable_argsort(icp_lib, waves, prefix):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    env = dict(os.environ, ICP_SORT_WAVES=waves, ICP_SORT_PREFIX=prefix)
    r = subprocess.run([sys.executable, "-c", SCRIPT, os.path.join(ROOT, "iterative-closest-point_amd")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"sort forms ok {N_CASES}" in r.stdout, r.stdout + r.stderr
