#!/usr/bin/env python3
"""The plane-to-plane loop (icp_set_plane_to_plane) beside the symmetric and the one-sided plane loops at
one size, alternated in one process: per-iteration time of icp_run(iters) from a fresh
scene, all under a gate nothing reaches (dmax = 1e6), so all run the same searches, the launch loop and
the gate's mask.

  python3 tools/gicp_probe.py [--n 1048576] [--iters 30] [--reps 3] [--modes gicp,symm,plane] [--epsilon 1e-3]

The clouds are icp_synthetic_pair's, both clouds' normals seeded unit vectors (the metrics' arithmetic
does not care that they are not a surface's).  Under `rocprofv3 --kernel-trace --stats` the kernels' own
times are in the trace; the stated algorithmic bytes per point are printed here.  --modes symm,plane
touches nothing this form added, so it runs against an older library too (ICP_AMD_LIB): the yardstick is
the parent commit's symmetric iteration.
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
    "gicp_moments_kernel<*, *>": 24 + 4 + 32 + 24 + 32 + 24,                   # the symmetric moments' bytes
    "gicp_transform_kernel": 24 + 24 + 4 + 32 + 24 + 24,                       # the symmetric transform's bytes
}


def unit(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="gicp,symm,plane")
    ap.add_argument("--epsilon", type=float, default=1e-3)
    a = ap.parse_args()
    modes = a.modes.split(",")
    assert set(modes) <= {"gicp", "symm", "plane"}, modes
    m, p = amd.synthetic_pair(a.n)
    nrm, u0 = unit(a.n, 7), unit(a.n, 8)
    print(f"n = nm = {a.n}, {a.iters} iterations a run, library {amd.LIB_PATH}")
    for k, v in BYTES.items():
        print(f"  algorithmic bytes a launch, {k}: {v} B x n = {v * a.n / 1e6:.1f} MB")
    ms = {k: [] for k in modes}
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_max_distance(1e6)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        for rep in range(a.reps + 1):  # (rep 0 warms up: code objects, buffers)
            for mode in modes:
                ctx.set_scene(p)
                if mode != "plane":
                    ctx.set_scene_normals(u0)
                if mode == "symm":
                    ctx.set_plane_symmetric(True)
                if mode == "gicp":
                    ctx.set_plane_to_plane(a.epsilon)
                t0 = time.perf_counter()
                res, errs = ctx.run(a.iters, -1.0)  # (returns after a stream synchronise)
                dt = (time.perf_counter() - t0) * 1e3 / max(res.iterations, 1)
                if mode == "symm":
                    ctx.set_plane_symmetric(False)
                if mode == "gicp":
                    ctx.set_plane_to_plane(0.0)
                k = ctx.inlier_trace()
                print(f"rep {rep} {mode:5s}: {dt:.4f} ms an iteration ({res.iterations} iterations, K {int(k[-1])}, "
                      f"err {errs[-1]:.6g})" + (" (warm-up)" if rep == 0 else ""))
                if rep:
                    ms[mode].append(dt)
        for mode in modes:
            if ms[mode]:
                print(f"{mode:5s}: median {statistics.median(ms[mode]):.4f} ms an iteration, min {min(ms[mode]):.4f}, "
                      f"max {max(ms[mode]):.4f} over {len(ms[mode])} runs")
        if "gicp" in ms and "symm" in ms and ms["gicp"] and ms["symm"]:
            print(f"gicp / symm: {statistics.median(ms['gicp']) / statistics.median(ms['symm']):.3f}")


if __name__ == "__main__":
    main()
