"""Sorts 2^20 random keys (20 and 24 bits, 6 times each) through icp_sort_pairs: for rocprofv3 kernel stats."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "iterative-closest-point_amd"))
import icp_amd
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
rng = np.random.default_rng(1)
keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
for bits in (20, 24):
    for _ in range(6):
        icp_amd.sort_pairs(keys, bits)
print("probe ok")
