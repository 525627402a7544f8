#!/usr/bin/env python3
"""The cost and the effect of the outlier filters.

  python3 tools/filter_probe.py [--n 1048576] [--reps 10] [--iters 60]

1. icp_filter_statistical_device at --n synthetic points (icp_synthetic_pair's model, uniform in
   [-1, 1]^3), k = 16, beside icp_estimate_model_normals(17) on the same cloud as the resident model in
   the same process: the same search with 17 entries, without the temporary grid's build.  Host wall time
   around each synchronous call (median, min, max of --reps after a warm-up call), and, with
   ICP_FILTER_DEBUG set here, the filter's own phases from events on the engine's stream (stderr): the
   grid's build, the per-point kernel, the rest.  The ratio printed is whole call over whole call.
2. icp_filter_radius_device on that cloud at a radius of three median nearest-neighbour distances
   (icp_model_knn's second column), min_neighbors 8, with the full counts and without.
3. cow_ref against cow_tr1 with n / 50 planted points around the scene (tests/filter_ref.py's clutter):
   the final err and the kept pairs' share without a filter, with the scene through (16, 2.0) and
   through (16, 1.0), --iters iterations each, and how many planted points each pair removed.
"""
import argparse
import os
import statistics
import sys
import time

os.environ.setdefault("ICP_FILTER_DEBUG", "1")

import numpy as np
import torch  # (before the first HIP call: torch then sees the device)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "iterative-closest-point_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import icp_amd as amd  # noqa: E402
import datasets  # noqa: E402
import filter_ref as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--iters", type=int, default=60)
args = ap.parse_args()


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), f"median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {reps} calls)"


def cost():
    n = args.n
    m = amd.synthetic_pair(n)[0]
    d = torch.from_numpy(m).cuda()
    out = torch.empty_like(d)
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with amd.Context() as ctx:
        ctx.set_model_device(d.data_ptr(), n)
        t_n, line = timed(lambda: ctx.estimate_model_normals(17), args.reps)
        print(f"n = {n}; estimate_model_normals(17): {line}", flush=True)
        kept = []
        t_f, line = timed(lambda: kept.append(ctx.filter_statistical_device(d.data_ptr(), n, 16, 2.0, out.data_ptr(),
                                                                            mask.data_ptr())), args.reps)
        print(f"filter_statistical_device(k 16, ratio 2): kept {kept[-1][0]}, (mu, sigma, T) {tuple(kept[-1][1])}: {line}")
        print(f"ratio to estimate_model_normals(17), whole calls: {t_f / t_n:.2f}", flush=True)
        _, d2 = ctx.model_knn(3, distances=True)
        radius = 3.0 * float(np.median(np.sqrt(d2[:, 1])))
        for with_counts in (True, False):
            kept = []
            _, line = timed(lambda: kept.append(ctx.filter_radius_device(d.data_ptr(), n, radius, 8, out.data_ptr(),
                                                                         mask.data_ptr(),
                                                                         cnt.data_ptr() if with_counts else None)), args.reps)
            print(f"filter_radius_device(radius {radius:.5f} = 3 median NN distances, min_neighbors 8, "
                  f"{'full counts' if with_counts else 'early stop'}): kept {kept[-1]}"
                  + (f", median count {int(cnt.median())}" if with_counts else "") + f": {line}", flush=True)


def effect():
    model = amd.load_matrix(datasets.path("cow_ref"))
    scene, planted = F.cow_clutter(amd.load_matrix, "cow_tr1")
    with amd.Context() as ctx:
        ctx.set_allow_unequal(True)
        ctx.set_model(model)
        for label, ratio in (("no filter", None), ("sor 16,2", 2.0), ("sor 16,1", 1.0)):
            p, note = scene, ""
            if ratio is not None:
                p, mask = ctx.filter_statistical(scene, 16, ratio, mask=True)
                gone = mask == 0
                note = (f", removed {int((gone & planted).sum())} of {int(planted.sum())} planted and "
                        f"{int((gone & ~planted).sum())} of {int((~planted).sum())} of the cow's")
            ctx.set_scene(p)
            res, _errs = ctx.run(args.iters)
            print(f"cow_ref <- cow_tr1 + clutter, {label}: {p.shape[0]} scene points{note}; {res.iterations} iterations, "
                  f"converged {res.converged}, err {res.err:.6g}", flush=True)


cost()
effect()
