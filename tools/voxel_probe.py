#!/usr/bin/env python3
"""The cost of the voxel downsample and of a coarse-to-fine registration.

  python3 tools/voxel_probe.py downsample [--n 1048576] [--reps 20]
  python3 tools/voxel_probe.py register [--pairs bunny,horse] [--iters 60] [--reps 5]

downsample: icp_voxel_downsample_device on icp_synthetic_pair's model (uniform in [-1, 1]^3) with the
voxel that gives about eight points a cell and the one that gives about one, a warm-up call and --reps
timed calls each (host wall time around the synchronous call: median, min, max), beside
icp_set_scene_device of the same cloud.  Under `rocprofv3 --kernel-trace --stats` the kernels' own
times are in the trace.
register: whole registrations from host arrays, plain (set_model, set_scene, run) against
icp_amd.register_pyramid with two levels (extent / 16, extent / 32; 30 iterations a level), the
bunny pair (sizes differ: the check lifted) and the horse pair: median wall time, iterations, final err.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the first HIP call: torch then sees the device)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "iterative-closest-point_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import icp_amd as amd  # noqa: E402
import datasets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["downsample", "register"])
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--pairs", default="bunny,horse")
ap.add_argument("--iters", type=int, default=60)
args = ap.parse_args()


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return f"median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {reps} calls)"


def downsample():
    m = amd.synthetic_pair(args.n)[0]
    d = torch.from_numpy(m).cuda()
    out = torch.empty_like(d)
    cnt = torch.empty(args.n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with amd.Context() as ctx:
        ctx.set_model_device(d.data_ptr(), args.n)
        print(f"n = {args.n}; set_scene_device: " + timed(lambda: ctx.set_scene_device(d.data_ptr(), args.n), args.reps))
        for per_cell in (8, 1):
            voxel = (8.0 * per_cell / args.n) ** (1.0 / 3.0)
            cells = []
            line = timed(lambda: cells.append(ctx.voxel_downsample_device(d.data_ptr(), args.n, voxel, out.data_ptr(),
                                                                          None, cnt.data_ptr())), args.reps)
            print(f"voxel {voxel:.5f} (about {per_cell} a cell): {cells[-1]} cells, largest "
                  f"{int(cnt[:cells[-1]].max())}; " + line)


def register():
    pairs = {"bunny": ("bun000", "bun045"), "horse": ("horse_ref", "horse_tr2"), "cow": ("cow_ref", "cow_tr2")}
    for name in args.pairs.split(","):
        m, p = (amd.load_matrix(datasets.path(x)) for x in pairs[name])
        ext = float((m.max(axis=0) - m.min(axis=0)).max())
        with amd.Context() as ctx:
            ctx.set_allow_unequal(True)
            last = {}

            def plain():
                ctx.set_model(m)
                ctx.set_scene(p)
                last["plain"] = ctx.run(args.iters)[0]

            def pyramid():
                last["pyr"] = amd.register_pyramid(ctx, m, p, [ext / 16, ext / 32], args.iters, 30)

            lp = timed(plain, args.reps)
            ly = timed(pyramid, args.reps)
            r = last["plain"]
            print(f"{name} ({m.shape[0]} / {p.shape[0]} points): plain {r.iterations} iterations, err {r.err:.4g}, "
                  f"converged {r.converged}: {lp}")
            res, _, rec = last["pyr"]
            lv = ", ".join(f"h=ext/{round(ext / x['voxel'])} {x['model_points']}/{x['scene_points']} pts "
                           f"{x['iterations']} it" for x in rec[:-1])
            print(f"{name}: pyramid [{lv}] then {res.iterations} iterations, err {res.err:.4g}, converged "
                  f"{res.converged}: {ly}")


downsample() if args.what == "downsample" else register()
