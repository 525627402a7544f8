"""The arithmetic of an iteration (moments, Horn's step, transform, error) on every path of the
engine against the extended-precision truth of tests/align_ref.py.

The other GPU tests compare the paths with each other bit for bit, and with the fp64 oracle at
well-conditioned shapes; a loss of accuracy common to all paths is invisible to both.  Here
iteration k in {1, 2, 6} of a run is checked on inputs that are ill-conditioned for the sums (far
from the origin, a small patch of a model whose centre is far away, rescaled, thin rods):

  run(k - 1) on a fresh context gives the input scene (the trajectory is deterministic; run(1)
  serves k = 1's output and k = 2's input); run(k) on another gives get_indices(), res.s / R / t,
  errs[k - 1], get_scene(), and inliers() under the gate.  Truth is
  truth_iteration(scene_{k-1}, m[idx_k], keep): the engine's own correspondences, the search is
  verified elsewhere.  The yardstick is the oracle's fp64 find_alignment + err_compute on the
  same pairs.

Acceptance, per metric (align_ref.acceptance): engine <= 8 x max(oracle, floor), floor = 16 eps64
(4 ulps for the stored cloud).  The engine sums in its own order and removes a shift: a small
constant number of extra roundings, and an order's luck is a factor of a few.  A defect that grows
like (D / sigma)^2 exceeds 8 from D / sigma ~ 10; the inputs reach 10^3 and 10^4.  On rods dR is
compared times the eigenvalue gap, dX and dP times gap / lever (the rotation about the axis is
determined to rounding / gap and moves a point by that times its distance from the axis), and
dOpt decides; dC, where the transform puts the pairs' centroid, does not depend on R and checks t
there at full strength.

Each path is confirmed from what stats() shows of it (confirm_path), so a policy change cannot
silently skip one.  Sizes are the smallest that reach the path.  The whole file takes 38 s on the
MI355X, 8 s of it the first RCCL communicator.

Measured on the MI355X (profiles/r08/align_accuracy.log): with the first
iterations' shifts near the data every figure is within the bound, most below a fifth of it.  With
both shifts at the model's centre (the parent of this test) the canonical and the gated first
iteration missed it on every patch: ds 9.9e-9 / 1.9e-8 at D / sigma = 1e4, 1.5e5 and 6.7e5 times
the bound.  Reading a miss: such a defect shows in ds, dX, dP and dE together and by orders of
magnitude.  dE alone on 'far' is mostly the rounding of the stored coordinates (|x| eps against
residuals of 1e-2), which the engine and the oracle meet on clouds that differ in their last bits:
two draws of the same noise, 0.73 of the bound apart at worst (far on two ranks, k = 6).  The
canonical schedule on ranks (ranks2_canon) sets its first shifts after an all-reduce of the sample:
with that branch taken out its three patch cases fail at k = 1 (ds 1.0e-8 at 1e4, 1.5e5 times the
bound) and nothing else does.
"""
import threading

import numpy as np
import pytest

import align_ref as A
import gated_ref as G
from test_gpu_sharded import HostAllReduce

pytestmark = pytest.mark.gpu

CHECKED = (1, 2, 6)
N_CANON, NM_CANON = (1 << 16) + 37, 1 << 16

N_RANKS_CANON = 2 * 49180  # two shards, each above the slot order's 49,152 points
BASE = ("plain", "far", "rod0.05", "rod1e-3", "patch1e3")
PATCHES = ("patch1e2", "patch1e3", "patch1e4")
EVERY = A.CASES
# path -> (n, nm, options, cases)
PATHS = {
    "one_launch_lds": (1000, 1000, dict(), BASE),
    "loop_small_1000": (1000, 1000, dict(run_mode="launches"), BASE),
    "loop_small_4096": (4096, 4096, dict(run_mode="launches"), BASE),
    "one_launch_mid": (4097, 4097, dict(), BASE),
    "loop_fused_tail": (4097, 4097, dict(variant="mfma16"), BASE),
    "loop_separate": (50000, 8000, dict(), BASE),
    "canon_default": (N_CANON, NM_CANON, dict(), EVERY),
    # (a model with all of A in a few grid cells would test only the brute-force fallback: no patch)
    "canon_grid": (N_CANON, NM_CANON, dict(variant="grid"), ("plain", "far", "scaled_small", "scaled_big", "noisy", "rod0.05")),
    "ranks2_4097": (4097, 4097, dict(world=2), BASE),
    "ranks3_4097": (4097, 4097, dict(world=3), BASE),
    # (shards of 32,787 and 21,858 points: below the slot order's 49,152, so these are the plain
    # multi-rank launch loop, first iteration two-pass, at a larger size -- not the canonical schedule)
    "ranks2_loop_65573": (N_CANON, NM_CANON, dict(world=2), BASE),
    "ranks3_loop_65573": (N_CANON, NM_CANON, dict(world=3), ("plain", "far", "rod1e-3", "patch1e4")),
    # the canonical schedule on ranks: every shard in slot order (49,180 points each), so the first
    # shifts go through the all-reduced sample (launch_first_shifts).  With that branch taken out
    # (shift_y left at c) the three patch cases fail at k = 1.
    "ranks2_canon": (N_RANKS_CANON, NM_CANON, dict(world=2), ("plain", "far", "rod0.05", "rod1e-3") + PATCHES),
    # (each context of this path builds a communicator, 0.5 s: the fewest cases that keep both solver
    # branches; a communicator differs from the host all-reduce inside allreduce() only, so the
    # canonical schedule on ranks is checked with the latter)
    "rccl1_4097": (4097, 4097, dict(rccl=True), ("plain", "far", "rod1e-3")),
    "gated_257": (257, 257, dict(gated=True), EVERY),
    "gated_4097": (4097, 4097, dict(gated=True), EVERY),
    "gated_9001": (9001, 9001, dict(gated=True), EVERY),
    "gated_canon": (N_CANON, NM_CANON, dict(gated=True), EVERY),
    "gated_ranks2_4097": (4097, 4097, dict(gated=True, world=2), ("plain", "far", "rod0.05", "patch1e4")),
}
PARAMS = [(path, name) for path, (_n, _nm, _o, cases) in PATHS.items() for name in cases]


@pytest.fixture(scope="module")
def amd(icp_lib):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return icp_lib


def one_context(amd, m, p, iters, opts, dmax, rank=0, world=1, red=None, np_total=None):
    kw = {}
    if world > 1:
        kw = dict(rank=rank, world_size=world, host_allreduce=red.for_rank(rank))
    elif opts.get("rccl"):
        kw = dict(rank=0, world_size=1, rccl_id=amd.rccl_unique_id())
    with amd.Context(0, amd.NN_CERTIFIED, **kw) as ctx:
        if opts.get("variant"):
            ctx.set_nn_variant({"mfma16": amd.VARIANT_MFMA16, "grid": amd.VARIANT_GRID}[opts["variant"]])
        if opts.get("run_mode") == "launches":
            ctx.set_run_mode(amd.RUN_LAUNCHES)
        ctx.set_allow_unequal((np_total or p.shape[0]) != m.shape[0])
        ctx.set_model(m)
        ctx.set_scene(p, np_total=np_total)
        if dmax is not None:
            ctx.set_max_distance(dmax)
        res, errs = ctx.run(iters, -1.0)
        out = dict(s=res.s, R=np.array(res.R).reshape(3, 3), t=np.array(res.t), iterations=res.iterations, errs=errs,
                   scene=ctx.get_scene(), idx=ctx.get_indices() if iters > 0 else None, stats=ctx.stats())
        if dmax is not None and iters > 0:
            out["mask"], out["K"] = ctx.inliers()
            out["ktrace"] = ctx.inlier_trace()
        return out


def run_engine(amd, m, p, iters, opts, dmax):
    world = opts.get("world", 1)
    if world == 1:
        return one_context(amd, m, p, iters, opts, dmax)
    red = HostAllReduce(world)
    results, errors = [None] * world, []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            results[r] = one_context(amd, m, p[b:b + c], iters, opts, dmax, r, world, red, p.shape[0])
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errors, errors
    out = dict(results[0])
    for r in results[1:]:  # identical solves on every rank
        assert r["s"] == out["s"] and np.array_equal(r["R"], out["R"]) and np.array_equal(r["errs"], out["errs"])
    for key in ("scene", "idx", "mask"):
        if out.get(key) is not None:
            out[key] = np.concatenate([r[key] for r in results])
    return out


FILTER = {"valu": 0, "mfma16": 2, "bundle": 3, "grid": 4, "one_launch": 6}  # icp_stats.last_filter


def confirm_path(amd, path, opts, k, out, n_local):
    """What stats() shows of the path the case is named after: whether the run was one launch,
    the search level of the last iteration, the searches the slot-order schedules count.  The
    launch loop's three tails (one workgroup up to 4,096 points, the fused tail up to 49,152 under
    AUTO, separate launches) have no statistic of their own: they follow from n and the run mode,
    restated here, and tests/test_gpu_persistent.py ties them to each other bit for bit."""
    st = out["stats"]
    assert out["iterations"] == k and out["errs"].size == k
    searches = st["run_bundle_searches"] + st["run_grid_searches"]
    slot_order = n_local > 49152
    if path.startswith("one_launch"):
        assert st["persistent_runs"] == 1 and st["last_filter"] == FILTER["one_launch"], st
    else:
        assert st["persistent_runs"] == 0 and st["last_filter"] != FILTER["one_launch"], st
    if path.startswith("loop_small"):
        assert n_local <= 4096 and st["last_filter"] == FILTER["valu"], st
    if path == "loop_fused_tail":
        assert 4096 < n_local <= 49152 and st["last_filter"] == FILTER["mfma16"], st
    if path == "loop_separate":
        assert n_local > 49152 and searches == 0, st  # (below 2^31 pairs: no slot order, no bundle, no grid)
    if path in ("ranks2_4097", "ranks3_4097", "rccl1_4097", "ranks2_loop_65573", "ranks3_loop_65573"):
        assert not slot_order
    if path in ("canon_default", "ranks2_canon"):
        assert slot_order and searches == k, st  # (the slot order's sizes: the bundle cascade or the grid)
    if path == "canon_grid":
        assert slot_order and st["run_grid_searches"] == k and st["last_filter"] == FILTER["grid"], st
        if k > 1:  # (iterations >= 2: the fused grid iteration)
            assert st["run_walked"] + st["run_certified"] > 0, st
    if opts.get("gated"):
        assert out["ktrace"].size == k and out["K"] == out["ktrace"][-1]


def check_iteration(amd, oracle, path, name, case, opts, k, before, out, report):
    m = case["m"]
    scene_in = before["scene"] if before is not None else case["p"]
    y = m[out["idx"]]
    keep = None
    if opts.get("gated"):
        D = np.float64(case["dmax"]) * np.float64(case["dmax"])
        keep = G.d2_of(scene_in, y) <= D
        np.testing.assert_array_equal(out["mask"], keep)  # the gate, in fp64 as written
        assert out["K"] == int(keep.sum()) == case["p"].shape[0] - max(1, case["p"].shape[0] // 20)
    tr = A.truth_iteration(scene_in, y, keep)
    eng = A.deviation(dict(s=out["s"], R=out["R"], t=out["t"], scene_out=out["scene"], err=out["errs"][k - 1]), tr)
    yard = A.oracle_deviation(oracle, tr)
    fails, ratios = A.acceptance(eng, yard, rod=case["rod"] is not None, gap=tr["gap"], lever=tr["lever"])
    line = (f"{path} {name} k={k} gap {float(tr['gap']):.3g} P'/|N|^3 {float(tr['dpoly']):.3g} "
            f"D/sigma {A.d_over_sigma(A.model_centre(m), np.asarray(tr['y'], dtype=np.float64)[tr['keep']]):.3g} | "
            + " ".join(f"{q} {eng[q]:.2g}/{yard[q]:.2g} ({ratios[q]:.2g})" for q in A.METRICS))
    print(line)
    report.append(line)
    if name == "rod0.05":  # the suite's handle on the polynomial branch, rod1e-3 on Jacobi's
        assert tr["dpoly"] > A.HANDOVER, line
    if name == "rod1e-3":
        assert tr["dpoly"] < 1e-4, line
    return [f"k={k} {f}" for f in fails]


_hip_failed = False  # a HIP error is sticky: once one is seen, no later test touches the device


@pytest.mark.parametrize("path,name", PARAMS)
def test_iteration_against_extended_precision(amd, oracle, path, name):
    global _hip_failed
    if _hip_failed:
        pytest.fail("an earlier test of this module met a HIP error")
    n, nm, opts, _cases = PATHS[path]
    case = A.case(name, n, nm, gated=bool(opts.get("gated")))
    runs = {0: None}
    try:
        for it in sorted({k for k in CHECKED} | {k - 1 for k in CHECKED if k > 1}):
            runs[it] = run_engine(amd, case["m"], case["p"], it, opts, case["dmax"])
    except amd.ICPError as e:
        _hip_failed = _hip_failed or e.code == amd.ICP_E_HIP
        raise
    fails, report = [], []
    for k in CHECKED:
        confirm_path(amd, path, opts, k, runs[k], amd.shard_range(n, 0, opts.get("world", 1))[1])
        fails += check_iteration(amd, oracle, path, name, case, opts, k, runs[k - 1], runs[k], report)
    assert not fails, "\n".join(fails + report)


# ---- the per-operation surface: find_alignment / err_compute fed the pairs directly ------------

@pytest.mark.parametrize("n", [4097, N_CANON])
@pytest.mark.parametrize("name", ["plain", "far", "scaled_small", "scaled_big", "rod0.05", "rod1e-3", "noisy"])
def test_surface_ops_against_extended_precision(amd, oracle, name, n):
    p, y, rod = A.pairs_case(name, n)
    tr = A.truth_iteration(p, y)
    with amd.Context(0, amd.NN_CERTIFIED) as ctx:
        s, R, t, e_al = ctx.find_alignment(p, y)
        e_tr, new_p = ctx.err_compute(y, p, True, (s * R).reshape(9), t)
    eng = A.deviation(dict(s=s, R=R, t=t, scene_out=new_p, err=(e_al + e_tr) / n), tr)
    yard = A.oracle_deviation(oracle, tr)
    fails, ratios = A.acceptance(eng, yard, rod=rod is not None, gap=tr["gap"], lever=tr["lever"])
    print(f"surface {name} n={n} gap {float(tr['gap']):.3g} | "
          + " ".join(f"{q} {eng[q]:.2g}/{yard[q]:.2g} ({ratios[q]:.2g})" for q in A.METRICS))
    assert not fails, fails
    # find_alignment's own residual and err_compute's are the same sum of the truth
    assert abs(e_al - float(tr["e"])) <= 8 * max(yard["dE"], A.FLOOR["dE"]) * float(tr["e"])
