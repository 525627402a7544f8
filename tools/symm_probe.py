#!/usr/bin/env python3
"""The symmetric point-to-plane loop beside the one-sided one at one size, alternated in one process
(DESIGN §3.15): per-iteration time of icp_run(iters) from a fresh scene, both with a gate nothing
reaches (dmax = 1e6), so both run the same searches, the launch loop and the gate's mask.

  python3 tools/symm_probe.py [--n 1048576] [--iters 30] [--reps 3] [--only plane|symm] [--estimate K]

The clouds are icp_synthetic_pair's, both clouds' normals seeded unit vectors (the metric's
arithmetic does not care that they are not a surface's).  --estimate K times
icp_estimate_scene_normals(K) on the scene as well.  Under `rocprofv3 --kernel-trace --stats` the
kernels' own times are in the trace; the stated algorithmic bytes per point are printed here.
--only plane touches nothing this form added, so it runs against an older library too (ICP_AMD_LIB).
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
    "plane_moments_kernel<*, *, false>": 24 + 4 + 32 + 24 + 32,                # p, idx, y gather, y store, the normal's gather
    "plane_transform_kernel<>": 24 + 24 + 4 + 32 + 24,                         # p, y, idx, normal gather, p store
    "plane_moments_kernel<*, *, true, SymmArgs>": 24 + 4 + 32 + 24 + 32 + 24,  # ... + u0
    "plane_transform_kernel<SymmArgs>": 24 + 24 + 4 + 32 + 24 + 24,            # ... + u0
}


def unit(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["plane", "symm"], default=None)
    ap.add_argument("--estimate", type=int, default=0)
    a = ap.parse_args()
    m, p = amd.synthetic_pair(a.n)
    nrm, u0 = unit(a.n, 7), unit(a.n, 8)
    print(f"n = nm = {a.n}, {a.iters} iterations a run")
    for k, v in BYTES.items():
        print(f"  algorithmic bytes a launch, {k}: {v} B x n = {v * a.n / 1e6:.1f} MB")
    modes = [a.only] if a.only else ["plane", "symm"]
    ms = {k: [] for k in modes}
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_max_distance(1e6)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        for rep in range(a.reps + 1):  # (rep 0 warms up: code objects, buffers)
            for mode in modes:
                ctx.set_scene(p)
                if mode == "symm":
                    ctx.set_scene_normals(u0)
                    ctx.set_plane_symmetric(True)
                t0 = time.perf_counter()
                res, errs = ctx.run(a.iters, -1.0)  # (returns after a stream synchronise)
                dt = (time.perf_counter() - t0) * 1e3 / max(res.iterations, 1)
                if mode == "symm":
                    ctx.set_plane_symmetric(False)
                k = ctx.inlier_trace()
                print(f"rep {rep} {mode:5s}: {dt:.4f} ms an iteration ({res.iterations} iterations, K {int(k[-1])}, "
                      f"err {errs[-1]:.6g})" + (" (warm-up)" if rep == 0 else ""))
                if rep:
                    ms[mode].append(dt)
        for mode in modes:
            if ms[mode]:
                print(f"{mode:5s}: median {statistics.median(ms[mode]):.4f} ms an iteration, min {min(ms[mode]):.4f}, "
                      f"max {max(ms[mode]):.4f} over {len(ms[mode])} runs")
        if a.estimate:
            est = []
            for rep in range(a.reps + 1):
                ctx.set_scene(p)
                t0 = time.perf_counter()
                deg = ctx.estimate_scene_normals(a.estimate)
                dt = (time.perf_counter() - t0) * 1e3
                print(f"rep {rep} estimate_scene_normals({a.estimate}): {dt:.3f} ms a call (grid build, search + PCA, "
                      f"read-back), {deg} undetermined" + (" (warm-up)" if rep == 0 else ""))
                if rep:
                    est.append(dt)
            print(f"estimate: median {statistics.median(est):.3f} ms a call over {len(est)} calls")


if __name__ == "__main__":
    main()
