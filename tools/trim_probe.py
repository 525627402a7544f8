#!/usr/bin/env python3
"""A trimmed registration (icp_set_trim) beside the gated one that keeps the same pairs (DESIGN
§3.14): whole registrations from a fresh scene, each timed by the host clock around icp_run (which
ends in a stream synchronise), medians over --regs of them after a warm-up.

  python3 tools/trim_probe.py --case synth|cow --mode trim [--f 0.75] [--regs 10]
  python3 tools/trim_probe.py --case synth|cow --mode gate --dmax X   (X: sqrt of the trimmed run's final C;
      the cow converges, so its final C is the residual's size and keeps 2 pairs of a fresh scene: its
      yardstick is the gate tests' dmax, 0.25 x the model's extent = 0.70494, K = 2203 against 2177)

--case synth: the 2^20 synthetic pair with a quarter of the scene moved to a far clump (the input of
profiles/gated/gated_measure.txt (b)), 8 iterations; --case cow: cow_ref against the cow clump
(tests/gated_ref.py), threshold 1e-5.  --mode gate uses icp_set_max_distance only, so it also runs on
a library built before icp_set_trim existed (ICP_AMD_LIB).  Under `rocprofv3 --kernel-trace --stats`
the kernels' own times are in the trace; the algorithmic bytes of the trim's passes are printed here.
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

# bytes a point of one launch of the trim's passes, from what each kernel reads and writes
KEYS_BYTES = 24 + 4 + 32 + 24 + 8  # p, idx, y gathered, y stored, the key stored
COUNT_BYTES = 8                    # a selection pass reads every key


def inputs(case, n):
    if case == "synth":
        m, p = amd.synthetic_pair(n)
        r = np.random.default_rng(5)
        k = n // 4
        p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
        return m, p, 8, -1.0
    import datasets
    import gated_ref as G
    ref = amd.load_matrix(datasets.path("cow_ref"))
    tr2 = amd.load_matrix(datasets.path("cow_tr2"))
    return ref, G.cow_clump(ref, tr2), 30, 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["synth", "cow"], default="synth")
    ap.add_argument("--mode", choices=["trim", "gate"], default="trim")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--f", type=float, default=0.75)
    ap.add_argument("--dmax", type=float, default=0.0)
    ap.add_argument("--regs", type=int, default=10)
    a = ap.parse_args()
    m, p, iters, threshold = inputs(a.case, a.n)
    n = p.shape[0]
    print(f"case {a.case}: n = {n}, nm = {m.shape[0]}, mode {a.mode}, " + (f"f = {a.f}" if a.mode == "trim" else f"dmax = {a.dmax!r}"))
    if a.mode == "trim":
        print(f"  algorithmic bytes: keys pass {KEYS_BYTES} B x n = {KEYS_BYTES * n / 1e6:.2f} MB; "
              f"each of the 6 selection passes {COUNT_BYTES} B x n = {COUNT_BYTES * n / 1e6:.2f} MB")
    ms, per_it = [], []
    with amd.Context() as ctx:
        ctx.set_model(m)
        if a.mode == "trim":
            ctx.set_trim(a.f)
        else:
            ctx.set_max_distance(a.dmax)
        for reg in range(a.regs + 1):  # (registration 0 warms up: code objects, buffers, model images)
            ctx.set_scene(p)
            t0 = time.perf_counter()
            res, errs = ctx.run(iters, threshold)  # (returns after a stream synchronise)
            dt = (time.perf_counter() - t0) * 1e3
            if reg:
                ms.append(dt)
                per_it.append(dt / max(res.iterations, 1))
        k = ctx.inlier_trace()
        line = f"  {res.iterations} iterations, K {int(k[0])} .. {int(k[-1])}, err {errs[-1]:.6g}"
        if a.mode == "trim":
            c = ctx.trim_trace()
            line += f", C {float(c[0])!r} .. {float(c[-1])!r}"
            print(f"final_dmax {float(np.sqrt(c[-1]) * (1.0 + 1e-9))!r}")
        print(line)
    print(f"{a.case} {a.mode}: median {statistics.median(ms):.4f} ms a registration (min {min(ms):.4f}, max {max(ms):.4f}), "
          f"{statistics.median(per_it) * 1e3:.1f} us an iteration, over {len(ms)} registrations")


if __name__ == "__main__":
    main()
