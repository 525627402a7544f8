#!/usr/bin/env python3
"""Global registration (icp_fpfh, icp_match_features, icp_ransac_pose, icp_global_pose)
measured: the host wall time of each call, the kernels' own times, and what the bunny pair gains.

  python3 tools/global_probe.py --what calls  [--reps 7]     the four calls' wall times, medians after a warm-up:
        the cow at voxel 0.12 and the bunny pair at 0.004 (each call of the chain on its coarse clouds, and
        the chain), icp_fpfh and icp_match_features at 2^16 points, icp_ransac_pose at C = 1,000, H = 100,000
  python3 tools/global_probe.py --what bunny                 bun000 / bun045, 50 iterations: the share of the scene
        within 0.001 of the model and the median NN distance, plain, --trim 0.6 alone, and global 0.004 + trim 0.6
  python3 tools/global_probe.py --what kernels --case cow|bunny|big   one case's calls a few times, to be run under
        `rocprofv3 --kernel-trace --stats` for the kernels' own times (tools/trace_medians.py)
  python3 tools/global_probe.py --what bench --parent-lib PATH [--rounds 3] [--first parent|tree]
        bench.py's headline line (--gpus 1 --steps 30 --warmup 3) with the parent commit's library (PATH: what
        `tools/build_ab.sh REV` prints; loaded through ICP_AMD_LIB) and this tree's alternated --rounds times in one
        call, each run a fresh process: "== round R parent|tree", then bench.py's JSON line, and a closing line
        of both series.  profiles/global/bench_ab.txt is this mode's output, once with each side first.

Each call is synchronous and ends with its outputs on the host, so the host clock around it is the call.
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
import datasets  # noqa: E402


def median_ms(fn, reps):
    fn()  # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def report(label, fn, reps):
    med, lo, hi = median_ms(fn, reps)
    print(f"{label:58s} median {med:9.3f} ms  (min {lo:9.3f}, max {hi:9.3f}, {reps} calls)", flush=True)


def pair(name):
    if name == "cow":  # the cow against itself turned 120 degrees about (1, 2, 3) and shifted (tests/global_ref.py)
        m = amd.load_matrix(datasets.path("cow_ref"))
        ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        a = np.deg2rad(120.0)
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        shift = np.array([0.5, -0.3, 0.8])
        return m, m @ R.T + shift, 0.12, (R.T, -(R.T @ shift))  # (the pose that maps the scene back: the truth)
    return amd.load_matrix(datasets.path("bun000")), amd.load_matrix(datasets.path("bun045")), 0.004, None


def chain_calls(ctx, name, reps, timed=True):
    m, p, voxel, truth = pair(name)
    mc, pc = ctx.voxel_downsample(m, voxel), ctx.voxel_downsample(p, voxel)
    fm, fp = ctx.fpfh(mc, 32), ctx.fpfh(pc, 32)
    pm, mp = ctx.match_features(fp, fm), ctx.match_features(fm, fp)
    ok = pm >= 0
    keep = np.nonzero(ok & (mp[np.where(ok, pm, 0)] == np.arange(pm.size)))[0]
    ps, qs = pc[keep], mc[pm[keep]]
    run = report if timed else (lambda label, fn, reps: [fn() for _ in range(reps)])
    print(f"{name}: voxel {voxel}, coarse {mc.shape[0]} / {pc.shape[0]} points, {keep.size} mutual matches", flush=True)
    run(f"{name}: icp_fpfh (model, k 32, normals k 16)", lambda: ctx.fpfh(mc, 32), reps)
    run(f"{name}: icp_match_features (scene -> model)", lambda: ctx.match_features(fp, fm), reps)
    run(f"{name}: icp_ransac_pose (C {keep.size}, H 100000)", lambda: ctx.ransac_pose(ps, qs, 100000, 0, 1.5 * voxel, 0.9),
        reps)
    run(f"{name}: icp_global_pose (the chain, both downsamples too)", lambda: ctx.global_pose(m, p, voxel), reps)
    R, t, rep = ctx.global_pose(m, p, voxel)
    print(f"{name}: seed 0 {rep}", flush=True)
    if truth is not None:  # the seed of the tests (tests/global_ref.py PURPOSE_SEED), and how far each pose is off
        for seed in (0, 1):
            R, t, rep = ctx.global_pose(m, p, voxel, seed=seed)
            ang = np.degrees(np.arccos(np.clip((np.trace(R.T @ truth[0]) - 1.0) / 2.0, -1.0, 1.0)))
            print(f"{name}: seed {seed} hypothesis {rep['best_h']} with {rep['inliers']} inliers of {rep['matches']} matches: "
                  f"{ang:.3f} degrees and {np.abs(t - truth[1]).max():.4f} from the truth", flush=True)
        ctx.set_model(m)
        ctx.set_scene(p)
        plain, _ = ctx.run(30, -1.0)
        res, _, _, _, _ = amd.register_global(ctx, m, p, voxel, 30, -1.0, seed=1)
        print(f"{name}: 30 iterations end at err {plain.err:.3e} plain and at {res.err:.3e} from the seed-1 pose", flush=True)


def big_calls(ctx, reps, timed=True):
    r = np.random.default_rng(1)
    n = 1 << 16
    v = r.standard_normal((n, 3))
    x = v / np.linalg.norm(v, axis=1)[:, None] * np.array([1.0, 0.7, 0.45])
    run = report if timed else (lambda label, fn, reps: [fn() for _ in range(reps)])
    f = ctx.fpfh(x, 32)
    g = ctx.fpfh(x[::-1] * 1.01, 32)
    run("2^16 points: icp_fpfh (k 32, normals k 16)", lambda: ctx.fpfh(x, 32), reps)
    run("2^16 x 2^16: icp_match_features", lambda: ctx.match_features(f, g), reps)
    C = 1000
    p = r.uniform(-1, 1, (C, 3))
    q = p + 0.01 * r.standard_normal((C, 3))
    q[600:] = r.uniform(-1, 1, (C - 600, 3))
    run("C 1000, H 100000: icp_ransac_pose", lambda: ctx.ransac_pose(p, q, 100000, 0, 0.03, 0.9), reps)
    print("C 1000: " + str({k: v for k, v in ctx.ransac_pose(p, q, 100000, 0, 0.03, 0.9).items() if k not in ("R", "t")}),
          flush=True)


def bunny(ctx):
    m, p, voxel, _ = pair("bunny")
    ctx.set_allow_unequal(True)
    rows = []
    for label, trim, use_global in (("plain", 1.0, False), ("--trim 0.6", 0.6, False), ("--global 0.004 --trim 0.6", 0.6, True)):
        ctx.set_trim(trim)
        if use_global:
            res, _, _, _, rep = amd.register_global(ctx, m, p, voxel, 50, -1.0)
            print(f"[global] {rep}", flush=True)
        else:
            ctx.set_model(m)
            ctx.set_scene(p)
            res, _ = ctx.run(50, -1.0)
        # the resident scene where the run left it, against the resident model (icp_evaluate): the share
        # within 0.001 is its fitness there, the median from every point's d2
        share = ctx.evaluate(0.001)["fitness"]
        d = np.sqrt(ctx.evaluate(float("inf"), per_point=True)["d2"])
        rows.append((label, float(share), float(np.median(d)), float(res.err)))
    ctx.set_trim(1.0)
    for label, share, med, err in rows:
        print(f"bunny {label:28s} within 0.001: {share:.4f}   median NN distance {med:.3e}   err {err:.3e}", flush=True)


def bench_ab(parent_lib, rounds, first):
    import json
    import subprocess
    root = os.path.abspath(os.path.join(HERE, ".."))
    order = ("parent", "tree") if first == "parent" else ("tree", "parent")
    series = {"parent": [], "tree": []}
    for r in range(rounds):
        for side in order:
            env = dict(os.environ)
            env.pop("ICP_AMD_LIB", None)
            if side == "parent":
                env["ICP_AMD_LIB"] = os.path.abspath(parent_lib)
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup",
                                  "3"], cwd=root, env=env, capture_output=True, text=True, timeout=300, check=True)
            line = out.stdout.strip().splitlines()[-1]
            series[side].append(json.loads(line)["value"])
            print(f"== round {r} {side}\n{line}", flush=True)
    print("iterations/s  " + "  ".join(f"{k}: " + " / ".join(f"{v:.0f}" for v in vs) for k, vs in series.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["calls", "bunny", "kernels", "bench"], default="calls")
    ap.add_argument("--case", choices=["cow", "bunny", "big"], default="cow")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", help="--what bench: the parent commit's libicp_hip.so (tools/build_ab.sh)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--first", choices=["parent", "tree"], default="parent")
    a = ap.parse_args()
    if a.what == "bench":  # (this process opens no device: every run is a fresh child)
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            ap.error("--what bench needs --parent-lib PATH (tools/build_ab.sh REV builds it)")
        return bench_ab(a.parent_lib, a.rounds, a.first)
    with amd.Context(0, amd.NN_CERTIFIED) as ctx:
        if a.what == "calls":
            chain_calls(ctx, "cow", a.reps)
            chain_calls(ctx, "bunny", a.reps)
            big_calls(ctx, a.reps)
        elif a.what == "bunny":
            bunny(ctx)
        elif a.case == "big":
            big_calls(ctx, 3, timed=False)
        else:
            chain_calls(ctx, a.case, 3, timed=False)


if __name__ == "__main__":
    main()
