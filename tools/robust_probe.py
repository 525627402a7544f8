#!/usr/bin/env python3
"""The robust kept-pairs loops beside the unweighted ones at one size, alternated in one process
(DESIGN §3.12): per-iteration time of icp_run(iters) from a fresh scene for the gated point-to-point
loop and the point-to-plane loop, each without weights and with Tukey weights, all with a gate
nothing reaches (dmax = 1e6), so every loop runs the same searches' cascade and the gate's mask.

  python3 tools/robust_probe.py [--n 1048576] [--iters 8] [--rounds 2] [--k 0.05] [--kind tukey]

The clouds are icp_synthetic_pair's, the normals seeded unit vectors (the metric's arithmetic does
not care that they are not a surface's).  Under `rocprofv3 --kernel-trace --stats` the kernels' own
times are in the trace: a weighted instantiation of a moments kernel (gated_moments_kernel<YIN, KIND>,
plane_moments_kernel<YIN, KIND, false>) reads and writes the bytes of the unweighted one (KIND = 0), whose
time in the same trace is its yardstick; the stated algorithmic bytes per point are printed here.
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
    "gated_moments_kernel<false, KIND>": 24 + 4 + 32 + 24,              # p, idx, y gather, y store
    "plane_moments_kernel<false, KIND, false>": 24 + 4 + 32 + 24 + 32,  # ... + the normal's gather
}
KINDS = {"huber": amd.ROBUST_HUBER, "tukey": amd.ROBUST_TUKEY, "cauchy": amd.ROBUST_CAUCHY}
LOOPS = [("gated", False, False), ("gated+w", False, True), ("plane", True, False), ("plane+w", True, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--k", type=float, default=0.05)
    ap.add_argument("--kind", choices=list(KINDS), default="tukey")
    a = ap.parse_args()
    m, p = amd.synthetic_pair(a.n)
    nrm = np.random.default_rng(7).standard_normal((a.n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    print(f"n = nm = {a.n}, {a.iters} iterations a run, weights {a.kind} k = {a.k}")
    for k, v in BYTES.items():
        print(f"  algorithmic bytes a launch, {k}: {v} B x n = {v * a.n / 1e6:.1f} MB")
    ms = {name: [] for name, _, _ in LOOPS}
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_max_distance(1e6)
        for rnd in range(a.rounds + 1):  # (round 0 warms up: code objects, buffers, the bundle images)
            for name, plane, weighted in LOOPS:
                ctx.set_metric(amd.METRIC_POINT_TO_PLANE if plane else amd.METRIC_POINT_TO_POINT)
                ctx.set_robust(KINDS[a.kind] if weighted else amd.ROBUST_NONE, a.k)
                ctx.set_scene(p)
                t0 = time.perf_counter()
                res, errs = ctx.run(a.iters, -1.0)  # (returns after a stream synchronise)
                dt = (time.perf_counter() - t0) * 1e3 / max(res.iterations, 1)
                k = ctx.inlier_trace()
                extra = ""
                if weighted:
                    w, kpos = ctx.robust_trace()
                    extra = f", W {w[-1]:.1f}, K+ {int(kpos[-1])}"
                print(f"round {rnd} {name:8s}: {dt:.4f} ms an iteration ({res.iterations} iterations, K {int(k[-1])}{extra}, "
                      f"err {errs[-1]:.6g})" + (" (warm-up)" if rnd == 0 else ""))
                if rnd:
                    ms[name].append(dt)
    for name, _, _ in LOOPS:
        if ms[name]:
            print(f"{name:8s}: median {statistics.median(ms[name]):.4f} ms an iteration, min {min(ms[name]):.4f}, "
                  f"max {max(ms[name]):.4f} over {len(ms[name])} runs")


if __name__ == "__main__":
    main()
