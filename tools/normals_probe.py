#!/usr/bin/env python3
"""The cost of icp_estimate_model_normals: one process, one context a model.

  python3 tools/normals_probe.py [--n 1048576] [--ks 16,30] [--reps 5] [--models synthetic,ellipsoid]
                                 [--counts]

Models: `synthetic`, icp_synthetic_pair's model (a uniform volume, the project's C4 cloud), and
`ellipsoid`, n points of the tri-axial ellipsoid of the plane tests (a surface: the occupied cells
are dense, most of the box is empty).  For each model and k: one warm-up call (code object, buffers),
then --reps timed calls (host wall time around the synchronous call), their median, min and max, and
neighbours a second = n k / median.  --counts instead sets ICP_NORMALS_DEBUG before the library
loads and makes one call each: the library then prints to stderr how many queries needed the second
scan or the scan of every point, and the candidates evaluated (here: per neighbour kept).
Under `rocprofv3 --kernel-trace --stats` the kernel's own time is in the trace.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--ks", default="16,30")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--models", default="synthetic,ellipsoid")
ap.add_argument("--counts", action="store_true")
args = ap.parse_args()
if args.counts:
    os.environ["ICP_NORMALS_DEBUG"] = "1"  # (read once, at the library's first estimate)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "iterative-closest-point_amd"))
import icp_amd as amd  # noqa: E402


def ellipsoid(n, seed=1):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * np.array([1.0, 0.7, 0.45])


def main():
    for name in args.models.split(","):
        m = amd.synthetic_pair(args.n)[0] if name == "synthetic" else ellipsoid(args.n)
        with amd.Context() as ctx:
            t0 = time.perf_counter()
            ctx.set_model(m)
            print(f"{name}: n = {args.n}, set_model {1e3 * (time.perf_counter() - t0):.2f} ms (first call of the context)",
                  flush=True)
            for k in (int(x) for x in args.ks.split(",")):
                deg = ctx.estimate_model_normals(k)  # warm-up (with --counts: the counted call)
                if args.counts:
                    sys.stderr.flush()
                    continue
                ms = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    ctx.estimate_model_normals(k)
                    ms.append(1e3 * (time.perf_counter() - t0))
                med = statistics.median(ms)
                print(f"{name} k = {k}: median {med:.3f} ms a call (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} calls), "
                      f"{args.n * k / med / 1e6:.2f} G neighbours/s, {deg} undetermined", flush=True)


if __name__ == "__main__":
    main()
