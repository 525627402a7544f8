#!/usr/bin/env python3
"""Everything the kept-pairs loop (icp_run under icp_set_max_distance, icp_set_metric, icp_set_robust,
icp_set_trim, icp_set_one_to_one and / or icp_set_plane_symmetric, icp_set_plane_to_plane) computes on the
cases of tests/test_gpu_gated.py, tests/test_gpu_plane.py and tests/test_gpu_symm.py and on every combination of its options at one
small size (matrix()), and what the normals' estimators and icp_model_knn return (normals()), dumped for a
bit-for-bit comparison of two libraries (ICP_AMD_LIB picks the library; tools/build_ab.sh builds
another revision's):

  ICP_AMD_LIB=.../build_ab/REV/libicp_hip.so python3 tools/kept_dump.py --out a.npz
  python3 tools/kept_dump.py --out b.npz
  python3 tools/kept_dump.py --compare a.npz b.npz      (exit status 1 if anything differs)

One process.  Per run: the return code and message, errs, the scene, s / R / t, the iterations, with
a gate the K trace, the mask and k, with weights the W and K+ traces, with a trim the C trace, and
the integer counters of stats() (run_path_bits, the searches' queue counts), and the scene's current
normals where the context has them.
"""
import argparse
import os
import sys
import threading

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "iterative-closest-point_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_amd as amd  # noqa: E402
import datasets  # noqa: E402
import gated_ref as G  # noqa: E402
import gicp_ref as GI  # noqa: E402
import normals_ref as NR  # noqa: E402
import plane_ref as P  # noqa: E402
import symm_ref as S  # noqa: E402
from test_gpu_gated import HostAllReduce  # noqa: E402

OUT = {}


def record(tag, ctx, iters, threshold=-1.0):
    """One ctx.run and everything it left, under tag."""
    rc, msg = 0, ""
    res = errs = None
    try:
        res, errs = ctx.run(iters, threshold)
    except amd.ICPError as e:
        rc, msg = e.code, str(e)
    OUT[tag + "/rc"] = np.array(rc)
    OUT[tag + "/msg"] = np.array(msg)
    OUT[tag + "/scene"] = ctx.get_scene()
    try:
        OUT[tag + "/scene_normals"] = ctx.scene_normals()
    except amd.ICPError:  # (the context has none)
        pass
    if res is not None:
        OUT[tag + "/errs"] = errs
        OUT[tag + "/srt"] = np.array([res.s] + list(res.R) + list(res.t))
        OUT[tag + "/iterations"] = np.array([res.iterations, res.converged])
    try:
        mask, k = ctx.inliers()
        OUT[tag + "/mask"] = mask
        OUT[tag + "/k"] = np.array(k)
        OUT[tag + "/inlier_trace"] = ctx.inlier_trace()
    except amd.ICPError as e:  # (no gated run since set_scene)
        OUT[tag + "/inliers_rc"] = np.array(e.code)
    for name, get in (("robust_trace", ctx.robust_trace), ("trim_trace", ctx.trim_trace)):
        try:
            got = get()
            for j, v in enumerate(got if isinstance(got, tuple) else (got,)):
                OUT[f"{tag}/{name}{j}"] = v
        except amd.ICPError as e:  # (no such run since set_scene)
            OUT[f"{tag}/{name}_rc"] = np.array(e.code)
    st = ctx.stats()
    OUT[tag + "/stats"] = np.array([int(v) & (2**64 - 1) for k, v in sorted(st.items()) if not isinstance(v, float)], dtype=np.uint64)


def options(ctx, dmax, robust, trim, uniq=False):
    """robust: (kind, k) or None; trim: the fraction or None; uniq: one-to-one"""
    if dmax:
        ctx.set_max_distance(dmax)
    if robust:
        ctx.set_robust(*robust)
    if trim:
        ctx.set_trim(trim)
    if uniq:
        ctx.set_one_to_one(True)


def symmetric(ctx, snrm, gicp=False):
    """snrm: the scene's normals, or None: the one-sided form; gicp: plane-to-plane, not the symmetric form"""
    if snrm is not None:
        ctx.set_scene_normals(snrm)
        if gicp:
            ctx.set_plane_to_plane(GI.EPS)
        else:
            ctx.set_plane_symmetric(True)


def unit_rows(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def fresh(tag, m, p, dmax, iters, nrm=None, threshold=-1.0, mode=0, variant=None, robust=None, trim=None, snrm=None,
          gicp=False, uniq=False, **ctx_args):
    with amd.Context(0, mode, **ctx_args) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        ctx.set_model(m)
        if nrm is not None:
            ctx.set_model_normals(nrm)
            ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_scene(p)
        symmetric(ctx, snrm, gicp)
        options(ctx, dmax, robust, trim, uniq)
        record(tag, ctx, iters, threshold)


def sharded(tag, m, p, dmax, world, iters, nrm=None, threshold=-1.0, robust=None, trim=None, snrm=None, gicp=False):
    red = HostAllReduce(world)
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                ctx.set_model(m)
                if nrm is not None:
                    ctx.set_model_normals(nrm)
                    ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
                ctx.set_scene(p[b:b + c], np_total=p.shape[0])
                symmetric(ctx, None if snrm is None else snrm[b:b + c], gicp)
                options(ctx, dmax, robust, trim)
                record(f"{tag}/rank{r}", ctx, iters, threshold)
        except Exception as e:
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    if errors:
        raise errors[0]


def slot_scene(n=65536):
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    nrm = r.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return m, p, nrm


# MATRIX_F: T = 77 of 193.  Under MATRIX_DMAX the gate keeps 72 pairs at first and 77 to 86 afterwards for the
# point, symmetric and (weighted) plane-to-plane cells, so in a gate-and-trim cell the gate binds first and
# the trim after it; the one-sided plane metric stays at 68 to 75 under the gate, where the gate alone binds.
# (0.75, T = 144, never bound under this gate: C stayed above 4 D.)
MATRIX_N, MATRIX_ITERS, MATRIX_K, MATRIX_F, MATRIX_DMAX = 193, 3, 0.1, 0.4, 0.08
KINDS = (("none", amd.ROBUST_NONE), ("huber", amd.ROBUST_HUBER), ("tukey", amd.ROBUST_TUKEY), ("cauchy", amd.ROBUST_CAUCHY))


def matrix(clump):
    """Every cell of metric x weights x trim x gate x one-to-one at n = 193 (three full waves and a partial
    fourth: the last mask word and the last ballot are partial; "symm" and "gicp": the plane metric's symmetric
    and plane-to-plane forms on seeded unit normals for the scene) on one rank, and without one-to-one and
    without and with Tukey weights on two (the fold-only pass, the all-reduce at each row width, the step on
    all-reduced sums); the cow clump with Tukey weights and a trim to convergence; the stops through the weighted and trimmed paths."""
    m, nrm, p = P.gate_case(MATRIX_N)
    snrm = unit_rows(MATRIX_N, 7)
    for metric in ("point", "plane", "symm", "gicp"):
        for kname, kind in KINDS:
            for trim in (None, MATRIX_F):
                for dmax in (0.0, MATRIX_DMAX):
                    cell = f"{metric}_{kname}_trim{trim or 'off'}_gate{dmax or 'off'}"
                    args = dict(nrm=None if metric == "point" else nrm, robust=(kind, MATRIX_K) if kind else None, trim=trim,
                                snrm=snrm if metric in ("symm", "gicp") else None, gicp=metric == "gicp")
                    fresh(f"matrix/{cell}", m, p, dmax, MATRIX_ITERS, **args)
                    fresh(f"matrix/{cell}_one_to_one", m, p, dmax, MATRIX_ITERS, uniq=True, **args)
                    if kname in ("none", "tukey"):
                        sharded(f"matrix/world2/{cell}", m, p, dmax, 2, MATRIX_ITERS, **args)
    tukey = (amd.ROBUST_TUKEY, 0.25 * G.cow_ext(clump[0]))
    # (the clump is a quarter of the scene: its own fraction, not the matrix's)
    fresh("matrix/clump_tukey_trim", clump[0], clump[1], 0.0, 60, threshold=1e-5, robust=tukey, trim=0.75)
    # K+ below the least count with K above it
    sm, sn, sp, _src = P.synth(MATRIX_N, 100 + MATRIX_N, 0.01)
    for metric in ("point", "plane"):
        for trim in (None, MATRIX_F):
            fresh(f"matrix/stop/no_weight_{metric}_trim{trim or 'off'}", sm, sp, 0.0, 5, nrm=sn if metric == "plane" else None,
                  robust=(amd.ROBUST_TUKEY, 1e-9), trim=trim)
    # the trim's T below the least count
    fm, fp = G.synth(5, 105, 0.25)
    for kname, kind in KINDS[::2]:
        fresh(f"matrix/stop/trim_few_point_{kname}", fm, fp, 0.0, 5, robust=(kind, 1.0) if kind else None, trim=0.7)
        fresh(f"matrix/stop/trim_few_plane_{kname}", *P.five()[::2], 0.0, 5, nrm=P.five()[1], robust=(kind, 1.0) if kind else None,
              trim=MATRIX_F)
    # a degenerate weighted plane system
    dm, dn, dp = P.planar()
    for trim in (None, MATRIX_F):
        fresh(f"matrix/stop/degenerate_tukey_trim{trim or 'off'}", dm, dp, 0.0, 5, nrm=dn, robust=(amd.ROBUST_TUKEY, 1.0), trim=trim)


def dump():
    cow = [amd.load_matrix(datasets.path(k)) for k in ("cow_ref", "cow_tr2")]
    clump = (cow[0], G.cow_clump(*cow), 0.25 * G.cow_ext(cow[0]))
    matrix(clump)
    # the gated suite
    for n in G.SIZES:
        m, p = G.synth(n, 100 + n, 0.25)
        fresh(f"gated/size{n}", m, p, G.SIZES_DMAX, G.SIZES_ITERS)
    for n, dmax in G.BITES:
        m, p = G.synth(n, 100 + n, 0.25, sigma=0.05)
        fresh(f"gated/bite{n}_{dmax}", m, p, dmax, G.BITES_ITERS)
    fresh("gated/clump", *clump, 30, threshold=1e-5)
    for world in (2, 3):
        sharded(f"gated/world{world}", *clump, world, 30, threshold=1e-5)
    fresh("gated/rccl1", *clump, 30, threshold=1e-5, mode=amd.NN_CERTIFIED, rank=0, world_size=1,
          rccl_id=amd.rccl_unique_id())
    m, p = G.synth(300, 1, 0.0)
    fresh("gated/too_few", m, p + np.array([10.0, 0.0, 0.0]), 1.0, 5)
    # the plane suite
    for n in P.SIZES:
        m, nrm, p, _src = P.synth(n, 100 + n, 0.01)
        fresh(f"plane/size{n}", m, p, 0.0, P.SIZES_ITERS, nrm=nrm)
    for n, dmax in P.GATES:
        m, nrm, p = P.gate_case(n)
        fresh(f"plane/gate{n}_{dmax}", m, p, dmax, P.GATES_ITERS, nrm=nrm)
    gm, gn, gp = P.gate_case(4097)
    sm, sn, sp, _src = P.synth(4097, 100 + 4097, 0.01)
    for name, mode, variant in (("fp64", amd.NN_FP64, None), ("grid", amd.NN_CERTIFIED, amd.VARIANT_GRID)):
        fresh(f"plane/{name}_gate_on", gm, gp, 0.08, P.GATES_ITERS, nrm=gn, mode=mode, variant=variant)
        fresh(f"plane/{name}_gate_off", sm, sp, 0.0, P.SIZES_ITERS, nrm=sn, mode=mode, variant=variant)
    for world in (2, 3):
        sharded(f"plane/world{world}", gm, gp, 0.08, world, P.GATES_ITERS, nrm=gn)
    fresh("plane/rccl1", gm, gp, 0.08, P.GATES_ITERS, nrm=gn, rank=0, world_size=1, rccl_id=amd.rccl_unique_id())
    m, nrm, p = P.five()
    fresh("plane/too_few", m, p, 0.0, 5, nrm=nrm)
    m, nrm, p = P.planar()
    fresh("plane/degenerate", m, p, 0.0, 5, nrm=nrm)
    # the symmetric form's stops (the normals after a frozen iteration are in the dump: unmoved)
    m, nrm, p, snrm = S.five()
    fresh("symm/too_few", m, p, 0.0, 5, nrm=nrm, snrm=snrm)
    m, nrm, p, snrm = S.planar()
    fresh("symm/degenerate", m, p, 0.0, 5, nrm=nrm, snrm=snrm)
    # a scene in slot order, each metric
    m, p, nrm = slot_scene()
    for name in ("gated", "plane", "symm"):
        with amd.Context() as ctx:
            ctx.set_model(m)
            ctx.set_model_normals(nrm)
            ctx.set_scene(p)
            if name == "symm":
                ctx.set_scene_normals(unit_rows(p.shape[0], 6))
            record(f"{name}/slot/before", ctx, 2)
            if name != "gated":
                ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
            if name == "symm":
                ctx.set_plane_symmetric(True)
            ctx.set_max_distance(0.05)
            record(f"{name}/slot/run", ctx, 3)
    # one context: gated point-to-point, ungated plane, gated plane, a new scene
    with amd.Context() as ctx:
        ctx.set_model(gm)
        ctx.set_model_normals(gn)
        ctx.set_scene(gp)
        ctx.set_max_distance(0.08)
        record("sequence/1_gated_point", ctx, 4)
        ctx.set_max_distance(0.0)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        record("sequence/2_ungated_plane", ctx, 3)
        ctx.set_max_distance(0.08)
        record("sequence/3_gated_plane", ctx, 3)
        ctx.set_scene(gp)
        ctx.set_max_distance(0.0)
        ctx.set_metric(amd.METRIC_POINT_TO_POINT)
        record("sequence/4_new_scene_point", ctx, 3)
    # symmetric iterations, a pose from outside, more of them: the run's total composed onto the context's
    with amd.Context() as ctx:
        ctx.set_model(gm)
        ctx.set_model_normals(gn)
        ctx.set_scene(gp)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        symmetric(ctx, unit_rows(gp.shape[0], 8))
        ctx.set_max_distance(0.08)
        record("symm_sequence/1_run", ctx, 2)
        ctx.transform_scene(1.0, P.rot((3, -1, 2), 2.0).reshape(-1), [0.01, -0.02, 0.005])
        OUT["symm_sequence/posed/scene"] = ctx.get_scene()
        OUT["symm_sequence/posed/scene_normals"] = ctx.scene_normals()
        record("symm_sequence/2_run", ctx, 2)
    # a point-to-point run after a plane run
    with amd.Context() as ctx:
        ctx.set_model(cow[0])
        nrm = np.random.default_rng(11).standard_normal(cow[0].shape)
        ctx.set_model_normals(nrm / np.linalg.norm(nrm, axis=1)[:, None])
        ctx.set_scene(cow[1])
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        record("after_plane/plane", ctx, 3)
        ctx.set_metric(amd.METRIC_POINT_TO_POINT)
        record("after_plane/point", ctx, 5)


def normals():
    """What the estimators and the k-NN return at 257 points and on tests/test_gpu_normals.py's duplicates
    (k = 16): the model's normals, the same cloud's as a scene, the neighbours and their distances, and
    the counts of undetermined points."""
    for name, cloud in (("257", P.ellipsoid(257, 357)[0]), ("duplicates", NR.duplicates())):
        with amd.Context() as ctx:
            ctx.set_model(cloud)
            OUT[f"normals/{name}/model_degenerate"] = np.array(ctx.estimate_model_normals(16))
            OUT[f"normals/{name}/model_normals"] = ctx.model_normals()
            ctx.set_scene(cloud)
            OUT[f"normals/{name}/scene_degenerate"] = np.array(ctx.estimate_scene_normals(16))
            OUT[f"normals/{name}/scene_normals"] = ctx.scene_normals()
            idx, d2 = ctx.model_knn(16, distances=True)
            OUT[f"normals/{name}/knn_idx"] = idx
            OUT[f"normals/{name}/knn_d2"] = d2


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("only in one dump:", k)
    runs = set()
    for k in sorted(set(a.files) & set(b.files)):
        runs.add(k.rsplit("/", 1)[0])
        if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                (np.array_equal(a[k], b[k]) if a[k].dtype.kind in "US" else a[k].tobytes() == b[k].tobytes())):
            bad.append(k)
            print("DIFFERS:", k)
    stops = sorted(k for k in a.files if k.endswith("/rc") and int(a[k]) != 0)
    print(f"{len(a.files)} arrays of {len(runs)} runs compared bit for bit: {len(bad)} differ")
    for k in stops:
        print(f"  {k[:-3]}: rc {int(a[k])} in both: {str(a[k[:-3] + '/msg'])}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not a.out:
        ap.error("--out FILE.npz or --compare A.npz B.npz")
    dump()
    normals()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **OUT)
    print(f"{len(OUT)} arrays of {len({k.rsplit('/', 1)[0] for k in OUT})} runs -> {a.out} ({amd.LIB_PATH})")


if __name__ == "__main__":
    main()
