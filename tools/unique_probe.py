#!/usr/bin/env python3
"""A one-to-one registration (icp_set_one_to_one) beside the same loop without the new pass: a gated
run whose gate keeps every pair.  Whole registrations from a fresh scene, each timed
by the host clock around icp_run (which ends in a stream synchronise), medians over --regs of them
after a warm-up.

  python3 tools/unique_probe.py --case clump|spread|cow --mode unique [--regs 10]
  python3 tools/unique_probe.py --case clump|spread|cow --mode gate    (dmax = 10 x the model's extent)

--case clump: the 2^20 synthetic pair with a quarter of the scene moved to a far clump (the input of
tools/trim_probe.py --case synth), 8 iterations: a quarter of the scatter lands on a handful of
model points, the contended case; --case spread: the same pair without the clump; --case cow:
cow_ref against the cow clump (tests/gated_ref.py), 30 iterations.  Every run has threshold -1, so
both modes run the same number of iterations.  --mode gate uses icp_set_max_distance only, so it
also runs on a library built before icp_set_one_to_one existed (ICP_AMD_LIB): the yardstick.  A
library built with -DICP_UNIQUE_ALWAYS_ATOMIC (make OUT=build_noskip EXTRA=-DICP_UNIQUE_ALWAYS_ATOMIC)
is the min pass without its load-before-atomic skip.  Under `rocprofv3 --kernel-trace --stats` the
kernels' own times are in the trace (tools/trace_medians.py); the algorithmic bytes of the new
passes are printed here.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "iterative-closest-point_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import icp_amd as amd  # noqa: E402

# bytes a point of the min pass, from what the kernel reads and writes: p, idx, y gathered, y
# stored (0 when the search stored it), the 8-byte atomic; the memset is 8 B a model point; the
# streamed moments add idx and an 8-byte gather from the table
MIN_BYTES = 24 + 4 + 32 + 24 + 8
MEMSET_BYTES = 8
MOMENTS_EXTRA_BYTES = 4 + 8


def inputs(case, n):
    if case in ("clump", "spread"):
        m, p = amd.synthetic_pair(n)
        if case == "clump":
            r = np.random.default_rng(5)
            k = n // 4
            p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
        return m, p, 8
    import datasets
    import gated_ref as G
    ref = amd.load_matrix(datasets.path("cow_ref"))
    tr2 = amd.load_matrix(datasets.path("cow_tr2"))
    return ref, G.cow_clump(ref, tr2), 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["clump", "spread", "cow"], default="clump")
    ap.add_argument("--mode", choices=["unique", "gate"], default="unique")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--regs", type=int, default=10)
    a = ap.parse_args()
    m, p, iters = inputs(a.case, a.n)
    n, nm = p.shape[0], m.shape[0]
    dmax = 10.0 * float(np.abs(m).max())
    print(f"case {a.case}: n = {n}, nm = {nm}, mode {a.mode}" + (f", dmax = {dmax!r}" if a.mode == "gate" else "") +
          f", library {amd.LIB_PATH}")
    if a.mode == "unique":
        print(f"  algorithmic bytes: min pass {MIN_BYTES} B x n = {MIN_BYTES * n / 1e6:.2f} MB, memset {MEMSET_BYTES} B x nm = "
              f"{MEMSET_BYTES * nm / 1e6:.2f} MB, the moments' extra {MOMENTS_EXTRA_BYTES} B x n = {MOMENTS_EXTRA_BYTES * n / 1e6:.2f} MB")
    ms, per_it = [], []
    with amd.Context() as ctx:
        ctx.set_model(m)
        if a.mode == "unique":
            ctx.set_one_to_one(True)
        else:
            ctx.set_max_distance(dmax)
        for reg in range(a.regs + 1):  # (registration 0 warms up: code objects, buffers, model images)
            ctx.set_scene(p)
            t0 = time.perf_counter()
            res, errs = ctx.run(iters, -1.0)  # (returns after a stream synchronise)
            dt = (time.perf_counter() - t0) * 1e3
            if reg:
                ms.append(dt)
                per_it.append(dt / max(res.iterations, 1))
        k = ctx.inlier_trace()
        print(f"  {res.iterations} iterations, K {int(k[0])} .. {int(k[-1])}, err {errs[-1]:.6g}")
    print(f"{a.case} {a.mode}: median {statistics.median(ms):.4f} ms a registration (min {min(ms):.4f}, max {max(ms):.4f}), "
          f"{statistics.median(per_it) * 1e3:.1f} us an iteration, over {len(ms)} registrations")


if __name__ == "__main__":
    main()
