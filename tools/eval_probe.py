#!/usr/bin/env python3
"""The cost of icp_evaluate.

  python3 tools/eval_probe.py [--n 1048576] [--reps 5] [--what big,cow,clump]

Host wall time around each synchronous call (median, min, max of --reps after a warm-up call) and, with
ICP_EVAL_DEBUG set here, the call's own phases from events on the engine's stream (stderr, one line a
call): the queries' rows or the scene's temporary grid, the forward search, the reverse search, the terms
and sums.  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats` once a case and
distance (`--what big --dists finite --no-yardsticks --reps 2`, then `--dists inf`, ...): the trace's
statistics are over every launch of the process, so one process must hold one case.

  big    icp_synthetic_pair at --n points, 30 iterations, then evaluate forward alone and both, at
         max_dist 0.01 and at infinity.  Yardsticks on the same clouds: the first, unseeded search of an
         icp_run (icp_stats.nn_ms after run(1) on a fresh context) for the forward search, and the whole
         icp_estimate_scene_normals(8) call (its temporary grid, then its 8-NN and PCA) for the reverse
         direction's grid.
  cow    cow_ref against cow_tr1 after 30 iterations, the same four calls at 0.1 and infinity.
  clump  a scene of --n points with a quarter of them in a far clump (tests/gated_ref.py's synth), as given,
         at max_dist 0.08 only: at infinity every far point scans every model point (see the header).
"""
import argparse
import os
import statistics
import sys
import time

os.environ.setdefault("ICP_EVAL_DEBUG", "1")
os.environ.setdefault("ICP_NN_TIMING_STRIDE", "1")  # (every iteration timed: else a run's iteration 0 never is)

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (before the first HIP call: torch then sees the device)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "iterative-closest-point_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import icp_amd as amd  # noqa: E402
import datasets  # noqa: E402
import gated_ref as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--what", default="big,cow,clump")
ap.add_argument("--dists", default="finite,inf", help="which of a case's distances (a kernel trace a case and distance)")
ap.add_argument("--no-yardsticks", action="store_true", help="the evaluate calls alone (for a kernel trace)")
args = ap.parse_args()


def pick(finite):
    """a case's distances: its finite one and infinity, as --dists asks"""
    want = args.dists.split(",")
    return tuple(d for d, w in ((finite, "finite"), (float("inf"), "inf")) if w in want)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return f"median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {reps} calls)"


def calls(ctx, label, dists):
    for d in dists:
        for both in (False, True):
            out = []
            line = timed(lambda: out.append(ctx.evaluate(d, both=both)), args.reps)
            e = out[-1]
            print(f"{label}: evaluate(max_dist {d}, {'both' if both else 'forward'}): K {e['correspondences']} of "
                  f"{e['scene_points']}, fitness {e['fitness']:.4f}, rmse {e['inlier_rmse']:.4e}, largest kept distance "
                  f"{e['max_inlier_d2'] ** 0.5:.4e}" + (f", K_m {e['model_correspondences']}" if both else "") + f": {line}",
                  flush=True)


def yardsticks(label, m, p):
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.reset_stats()
        ctx.run(1, -1.0)
        st = ctx.stats()
        if st["nn_launches"]:
            print(f"{label}: icp_run's first, unseeded search: nn_ms {st['nn_ms']:.3f} over {st['nn_launches']} launch(es)",
                  flush=True)
        else:  # (the one-launch path of small clouds has no search launch of its own to time)
            print(f"{label}: icp_run took the one-launch path: no search of its own was timed, no yardstick", flush=True)
    with amd.Context() as ctx:
        ctx.set_model(m)

        def normals():
            ctx.set_scene(p)
            ctx.estimate_scene_normals(8)

        t0 = time.perf_counter()
        ctx.set_scene(p)
        t_set = 1e3 * (time.perf_counter() - t0)
        print(f"{label}: set_scene + estimate_scene_normals(8), whole calls: {timed(normals, args.reps)}; set_scene alone "
              f"once {t_set:.3f} ms", flush=True)


def registered(label, m, p, dists, iters=30):
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        if iters:
            res, _ = ctx.run(iters, -1.0)
            print(f"{label}: nm {m.shape[0]} np {p.shape[0]}, {res.iterations} iterations, err {res.err:.4e}", flush=True)
        calls(ctx, label, dists)


what = args.what.split(",")
if "big" in what:
    m, p = amd.synthetic_pair(args.n)
    if not args.no_yardsticks:
        yardsticks(f"synthetic {args.n}", m, p)
    registered(f"synthetic {args.n}", m, p, pick(0.01))
if "cow" in what:
    m, p = amd.load_matrix(datasets.path("cow_ref")), amd.load_matrix(datasets.path("cow_tr1"))
    if not args.no_yardsticks:
        yardsticks("cow", m, p)
    registered("cow", m, p, pick(0.1))
if "clump" in what:
    m, p = G.synth(args.n, 100 + args.n, 0.25, sigma=0.05)
    registered(f"far clump {args.n}", m, p, (0.08,), iters=0)
