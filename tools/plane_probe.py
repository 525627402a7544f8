#!/usr/bin/env python3
"""The point-to-plane loop beside the gated loop at one size, alternated in one process
(DESIGN §3.10): per-iteration time of icp_run(iters) from a fresh scene, both with a gate nothing
reaches (dmax = 1e6), so both run the same searches' cascade, the launch loop and the gate's mask.

  python3 tools/plane_probe.py [--n 1048576] [--iters 8] [--reps 5] [--only gated|plane]

The clouds are icp_synthetic_pair's, the normals seeded unit vectors (the metric's arithmetic does
not care that they are not a surface's).  Under `rocprofv3 --kernel-trace --stats` (with --only) the
kernels' own times are in the trace; the stated algorithmic bytes per point are printed here.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "iterative-closest-point_amd"))
import icp_amd as amd  # noqa: E402

# bytes a point of one launch, from what each kernel reads and writes (y gathered through idx / kpos)
BYTES = {
    "gated_moments_kernel": 24 + 4 + 32 + 24,             # p, idx, y gather, y store
    "gated_transform_kernel": 24 + 24 + 24,               # p, y, p store
    "plane_moments_kernel<*, *, false>": 24 + 4 + 32 + 24 + 32,  # ... + the normal's gather
    "plane_transform_kernel<>": 24 + 24 + 4 + 32 + 24,    # p, y, idx, normal gather, p store
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["gated", "plane"], default=None)
    a = ap.parse_args()
    m, p = amd.synthetic_pair(a.n)
    nrm = np.random.default_rng(7).standard_normal((a.n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    print(f"n = nm = {a.n}, {a.iters} iterations a run")
    for k, v in BYTES.items():
        print(f"  algorithmic bytes a launch, {k}: {v} B x n = {v * a.n / 1e6:.1f} MB")
    modes = [a.only] if a.only else ["gated", "plane"]
    ms = {k: [] for k in modes}
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_max_distance(1e6)
        for rep in range(a.reps + 1):  # (rep 0 warms up: code objects, buffers, the bundle images)
            for mode in modes:
                ctx.set_metric(amd.METRIC_POINT_TO_PLANE if mode == "plane" else amd.METRIC_POINT_TO_POINT)
                ctx.set_scene(p)
                t0 = time.perf_counter()
                res, errs = ctx.run(a.iters, -1.0)  # (returns after a stream synchronise)
                dt = (time.perf_counter() - t0) * 1e3 / max(res.iterations, 1)
                k = ctx.inlier_trace()
                print(f"rep {rep} {mode:5s}: {dt:.4f} ms an iteration ({res.iterations} iterations, K {int(k[-1])}, "
                      f"err {errs[-1]:.6g})" + (" (warm-up)" if rep == 0 else ""))
                if rep:
                    ms[mode].append(dt)
    for mode in modes:
        if ms[mode]:
            print(f"{mode:5s}: median {statistics.median(ms[mode]):.4f} ms an iteration, min {min(ms[mode]):.4f}, "
                  f"max {max(ms[mode]):.4f} over {len(ms[mode])} runs")


if __name__ == "__main__":
    main()
