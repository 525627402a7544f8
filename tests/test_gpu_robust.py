"""icp_run with robust weights (icp_set_robust; the robust kernels of icp_gated.hip and icp_plane.hip)
against tests/robust_ref.py, the loop restated with the oracle's search, its Horn eigen-solve and numpy.

Tolerances are test_gpu_plane.py's: err rel 1e-9, R abs 1e-9, t and new_p abs 1e-9 x
extent; W rel 1e-9; K+ and K exact (tests/test_robust_ref.py checks on the CPU that no kept pair of
these inputs lies within 1e-9 of k, none within 1e-6 of the gate, and that the fp64 reference sits
within 1e-11 of extended precision).
"""
import os
import subprocess
import threading

import numpy as np
import pytest
import torch  # (before the first HIP call of the session: torch then sees the device)

import plane_ref as P
import robust_ref as R
from test_gpu_gated import HostAllReduce

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


def setup(amd, ctx, metric, m, nrm, p, dmax, kind, k, np_total=None):
    ctx.set_model(m)
    if metric == "plane":
        ctx.set_model_normals(nrm)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
    ctx.set_scene(p, np_total=np_total)
    if dmax:
        ctx.set_max_distance(dmax)
    if kind is not None:
        ctx.set_robust(kind, k)


def collect(ctx, res, errs, dmax, kind):
    out = dict(res=res, errs=errs, scene=ctx.get_scene(), R=np.array(res.R).reshape(3, 3), t=np.array(res.t), s=res.s)
    if dmax:
        mask, k = ctx.inliers()
        out.update(K=ctx.inlier_trace(), mask=mask, k=k)
    if kind:
        out["W"], out["Kpos"] = ctx.robust_trace()
    return out


def run(amd, metric, m, nrm, p, dmax, kind, k, iters, threshold=-1.0, **ctx_args):
    """-> dict(res, errs, scene, R, t, s; with a gate K (trace), mask, k; with weights W, Kpos) of a
    fresh context.  kind None: icp_set_robust is never called."""
    with amd.Context(0, 0, **ctx_args) as ctx:
        setup(amd, ctx, metric, m, nrm, p, dmax, kind, k)
        res, errs = ctx.run(iters, threshold)
        return collect(ctx, res, errs, dmax, kind)


def check_against_ref(m, out, r, metric):
    print("err", out["errs"], "ref err", np.asarray(r["err"]), "W", list(out["W"]), "K+", list(out["Kpos"]))
    assert out["res"].iterations == r["iterations"]
    np.testing.assert_allclose(out["errs"], r["err"], rtol=1e-9)
    np.testing.assert_allclose(out["R"], r["R"], atol=1e-9)
    extent = float(np.abs(m).max())
    np.testing.assert_allclose(out["t"], r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(out["scene"], r["new_p"], atol=1e-9 * extent)
    if metric == "plane":
        assert out["s"] == 1.0
    else:
        np.testing.assert_allclose(out["s"], r["s"], rtol=1e-9)
    np.testing.assert_allclose(out["W"], np.array(r["W"], dtype=np.float64), rtol=1e-9)
    assert list(out["Kpos"]) == r["Kpos"]
    if "K" in out:
        assert list(out["K"]) == r["K"] and out["k"] == r["K"][-1]
        np.testing.assert_array_equal(out["mask"], r["mask"])


def bitwise(a, b, keys=("errs", "scene", "R", "t", "s")):
    for key in keys + (("K", "mask") if "K" in a and "K" in b else ()):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# 1. against the reference: the least K, the whole-wave loop with its ballot across a wave and a
# workgroup boundary, more than one partial row (4097 > kRedSingle); no gate (D = +inf).  The
# point-to-point cases pin the pre-pass too: the scene is centred 0.037 from the model's centre.
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("kname", list(R.KINDS))
@pytest.mark.parametrize("metric", R.METRICS)
def test_sizes(icp_lib, oracle, metric, kname, n):
    m, nrm, p, dmax, kind, k, r = R.reference(oracle, ("size", metric, R.KINDS[kname], n))
    check_against_ref(m, run(icp_lib, metric, m, nrm, p, dmax, kind, k, R.SIZES_ITERS), r, metric)


def test_far_scene_pins_the_first_shifts(icp_lib, oracle):
    """The scene 10 x the model's extent away under a gate that keeps every pair (robust_ref.far_case:
    why not 100 x)."""
    m, nrm, p, dmax, kind, k, r = R.reference(oracle, ("far",))
    out = run(icp_lib, "point", m, nrm, p, dmax, kind, k, R.SIZES_ITERS)
    check_against_ref(m, out, r, "point")
    assert list(out["K"]) == [R.FAR_N] * R.SIZES_ITERS


# 2. a weight of exactly 1.0 adds the unweighted kernel's bits: Huber with k = 1e150 and the gate on
# against the same run without icp_set_robust
@pytest.mark.parametrize("metric", R.METRICS)
def test_unit_weights_are_bit_identical_at_4097(icp_lib, metric):
    m, nrm, p = P.gate_case(4097)
    a = run(icp_lib, metric, m, nrm, p, 0.08, R.HUBER, 1e150, 8)
    b = run(icp_lib, metric, m, nrm, p, 0.08, None, 0.0, 8)
    print("K", list(a["K"]), "W", list(a["W"]))
    assert a["res"].iterations == b["res"].iterations == 8
    bitwise(a, b)
    np.testing.assert_array_equal(a["W"], a["K"].astype(np.float64))
    np.testing.assert_array_equal(a["Kpos"], a["K"])


@pytest.mark.parametrize("metric", R.METRICS)
def test_unit_weights_are_bit_identical_past_the_grid_cap(icp_lib, metric):
    """One point more than the reductions' 256 workgroups x 256 threads: a thread takes two points."""
    amd = icp_lib
    n = 256 * 256 + 1
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    nrm = r.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    a = run(amd, metric, m, nrm, p, 0.05, R.HUBER, 1e150, 3)
    b = run(amd, metric, m, nrm, p, 0.05, None, 0.0, 3)
    print("K", list(a["K"]), "W", list(a["W"]))
    assert a["res"].iterations == b["res"].iterations == 3 and 6 <= a["k"] < n
    bitwise(a, b)
    np.testing.assert_array_equal(a["W"], a["K"].astype(np.float64))
    np.testing.assert_array_equal(a["Kpos"], a["K"])


# 3. the purpose: clutter near the surface, inside the gate
@pytest.fixture(scope="module")
def shell_runs(icp_lib, oracle):
    out = {}
    for metric in R.METRICS:
        m, nrm, p, dmax, kind, k, _r = R.reference(oracle, ("shell", metric, R.TUKEY))
        out[metric] = run(icp_lib, metric, m, nrm, p, dmax, kind, k, R.SHELL_ITERS[metric])
    return out


@pytest.mark.parametrize("metric", R.METRICS)
def test_outlier_shell(icp_lib, oracle, shell_runs, metric):
    m, nrm, p, dmax, kind, k, r = R.reference(oracle, ("shell", metric, R.TUKEY))
    _m, _nrm, _p, inlier = R.outlier_shell()
    out = shell_runs[metric]
    check_against_ref(m, out, r, metric)
    plain = run(icp_lib, metric, m, nrm, p, dmax, None, 0.0, R.SHELL_ITERS[metric])
    d0, d1 = R.inlier_displacement(plain["scene"], m, inlier), R.inlier_displacement(out["scene"], m, inlier)
    print(metric, "largest inlier displacement: unweighted %.3e Tukey %.3e" % (d0, d1))
    assert list(plain["K"]) == list(out["K"]) == [R.SHELL_N] * R.SHELL_ITERS[metric]
    assert d1 <= 0.5 * d0


# 4. too few positive weights: the run stops before the iteration changes anything
def test_no_positive_weight_stops_at_iteration_0(icp_lib):
    amd = icp_lib
    m, nrm, p, _src = P.synth(257, 357, 0.01)
    for metric in R.METRICS:
        with amd.Context() as ctx:
            setup(amd, ctx, metric, m, nrm, p, 0.0, R.TUKEY, 1e-9)
            with pytest.raises(amd.ICPError) as ei:
                ctx.run(5, -1.0)
            print(str(ei.value))
            assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS
            assert "iteration 0" in str(ei.value) and "K = 257" in str(ei.value) and "K+ = 0" in str(ei.value)
            np.testing.assert_array_equal(ctx.get_scene(), p)
            w, kpos = ctx.robust_trace()
            assert w.size == 0 and kpos.size == 0


def test_five_positive_weights_stop_the_plane_metric(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, _src = P.synth(257, 357, 0.01)
    Y, idx = oracle.closest(p, m)
    d = p - Y
    n_ = nrm[idx]
    r = (d[:, 0] * n_[:, 0] + d[:, 1] * n_[:, 1]) + d[:, 2] * n_[:, 2]
    r2 = np.sort(r * r)
    k = float(np.sqrt(0.5 * (r2[4] + r2[5])))  # between the 5th and the 6th smallest residual
    assert (r2[5] - r2[4]) / r2[5] > 1e-6 and int((r * r < k * k).sum()) == 5
    with amd.Context() as ctx:
        setup(amd, ctx, "plane", m, nrm, p, 0.0, R.TUKEY, k)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(5, -1.0)
        print(str(ei.value))
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS
        assert "iteration 0" in str(ei.value) and "K = 257" in str(ei.value) and "K+ = 5" in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)
        assert ctx.robust_trace()[0].size == 0
    with amd.Context() as ctx:  # (five are enough for the point-to-point metric's 4)
        m6, nrm6, p6, dmax, kind, k6, ref = R.reference(oracle, ("size", "point", R.TUKEY, 6))
        setup(amd, ctx, "point", m6, nrm6, p6, dmax, kind, k6)
        res, _errs = ctx.run(2, -1.0)
        assert res.iterations == 2


# 5. ranks
def run_sharded(amd, metric, m, nrm, p, dmax, kind, k, world, iters):
    red = HostAllReduce(world)
    results = [None] * world
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                setup(amd, ctx, metric, m, nrm, p[b:b + c], dmax, kind, k, np_total=p.shape[0])
                res, errs = ctx.run(iters, -1.0)
                results[r] = collect(ctx, res, errs, dmax, kind)
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errors, errors
    return results


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("metric", R.METRICS)
def test_ranks_match_single(icp_lib, oracle, shell_runs, metric, world):
    m, nrm, p, dmax, kind, k, _r = R.reference(oracle, ("shell", metric, R.TUKEY))
    ref = shell_runs[metric]
    out = run_sharded(icp_lib, metric, m, nrm, p, dmax, kind, k, world, R.SHELL_ITERS[metric])
    print("single", ref["errs"][-3:], "ranks", out[0]["errs"][-3:], "W", out[0]["W"][-3:], ref["W"][-3:])
    for o in out:  # identical decisions and solves on every rank
        for key in ("errs", "K", "R", "W", "Kpos"):
            np.testing.assert_array_equal(o[key], out[0][key], err_msg=key)
    assert out[0]["res"].iterations == ref["res"].iterations
    np.testing.assert_array_equal(out[0]["K"], ref["K"])
    np.testing.assert_array_equal(out[0]["Kpos"], ref["Kpos"])
    np.testing.assert_allclose(out[0]["W"], ref["W"], rtol=1e-11)
    np.testing.assert_allclose(out[0]["errs"], ref["errs"], rtol=1e-11)
    np.testing.assert_array_equal(np.concatenate([o["mask"] for o in out]), ref["mask"])
    np.testing.assert_allclose(np.concatenate([o["scene"] for o in out]), ref["scene"], atol=1e-12)


def test_rccl_single_rank_communicator(icp_lib, oracle, shell_runs):
    """The 30 sums and the residual all-reduce through ncclAllReduce on a 1-rank communicator: the
    identity, so the run is the plain context's bit for bit."""
    amd = icp_lib
    m, nrm, p, dmax, kind, k, _r = R.reference(oracle, ("shell", "plane", R.TUKEY))
    out = run(amd, "plane", m, nrm, p, dmax, kind, k, R.SHELL_ITERS["plane"], rank=0, world_size=1,
              rccl_id=amd.rccl_unique_id())
    bitwise(out, shell_runs["plane"], keys=("errs", "scene", "R", "t", "s", "W", "Kpos"))


# 6. a scene in slot order, correspondences with kd positions
@pytest.mark.parametrize("metric", R.METRICS)
def test_robust_run_on_a_scene_in_slot_order(icp_lib, metric):
    """test_gpu_plane.py::test_plane_run_on_a_scene_in_slot_order with Tukey weights: two unweighted
    point-to-point iterations at 65,536 points leave the scene in slot order; three gated robust
    iterations on that context against three on a fresh context given the same scene (file order)."""
    amd = icp_lib
    n = 65536
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    nrm = r.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    dmax, scale = 0.05, 0.02
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.run(2, -1.0)
        mid = ctx.get_scene()
        if metric == "plane":
            ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_max_distance(dmax)
        ctx.set_robust(R.TUKEY, scale)
        res, errs = ctx.run(3, -1.0)
        a = collect(ctx, res, errs, dmax, R.TUKEY)
    b = run(amd, metric, m, nrm, mid, dmax, R.TUKEY, scale, 3)
    print("K", list(a["K"]), "K+", list(a["Kpos"]), list(b["Kpos"]), "W", list(a["W"]), "err", a["errs"], b["errs"])
    assert a["res"].iterations == b["res"].iterations == 3
    np.testing.assert_array_equal(a["K"], b["K"])
    np.testing.assert_array_equal(a["Kpos"], b["Kpos"])
    assert a["k"] == b["k"] and 6 <= a["Kpos"][-1] < a["k"] < n
    np.testing.assert_array_equal(a["mask"], b["mask"])
    np.testing.assert_allclose(a["W"], b["W"], rtol=1e-11)
    np.testing.assert_allclose(a["errs"], b["errs"], rtol=1e-11)
    np.testing.assert_allclose(a["scene"], b["scene"], atol=1e-12)


# 7. off is off
def test_off_is_off(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p = P.gate_case(4097)
    fresh = {"gated": run(amd, "point", m, nrm, p, 0.08, None, 0.0, 6),
             "plane": run(amd, "plane", m, nrm, p, 0.0, None, 0.0, 6)}
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        res, errs = ctx.run(6, -1.0)
        fresh["plain"] = collect(ctx, res, errs, 0.0, None)
        fresh["plain_stats"] = ctx.stats()["persistent_runs"]
    with amd.Context() as ctx:
        setup(amd, ctx, "point", m, nrm, p, 0.08, R.TUKEY, 0.05)
        res, errs = ctx.run(4, -1.0)  # a robust gated run: the inliers are the gate's, not the weights'
        mask, k = ctx.inliers()
        w, kpos = ctx.robust_trace()
        ktrace = ctx.inlier_trace()
        print("K", list(ktrace), "K+", list(kpos))
        assert res.iterations == 4 and mask.sum() == k == ktrace[-1] and kpos[-1] < k
        ctx.set_max_distance(0.0)
        res, errs = ctx.run(2, -1.0)  # robust, ungated: the last gated run's report stays
        mask2, k2 = ctx.inliers()
        np.testing.assert_array_equal(mask2, mask)
        assert k2 == k and ctx.robust_trace()[0].size == 2
        np.testing.assert_array_equal(ctx.inlier_trace(), ktrace)
        ctx.set_robust(R.NONE, 0.0)
        ctx.set_model_normals(nrm)
        for form in ("gated", "plane", "plain"):
            ctx.set_scene(p)
            ctx.set_max_distance(0.08 if form == "gated" else 0.0)
            ctx.set_metric(amd.METRIC_POINT_TO_PLANE if form == "plane" else amd.METRIC_POINT_TO_POINT)
            before = ctx.stats()["persistent_runs"]
            res, errs = ctx.run(6, -1.0)
            out = collect(ctx, res, errs, 0.08 if form == "gated" else 0.0, None)
            bitwise(out, fresh[form])
            if form == "plain":
                assert ctx.stats()["persistent_runs"] - before == fresh["plain_stats"]
            with pytest.raises(amd.ICPError) as ei:  # (no robust run since set_scene)
                ctx.robust_trace()
            assert ei.value.code == amd.ICP_E_NO_MODEL


# 8. arguments
def test_arguments(icp_lib, oracle):
    amd = icp_lib
    import ctypes as C
    m, nrm, p, dmax, kind, k, _r = R.reference(oracle, ("size", "point", R.TUKEY, 257))
    ref = run(amd, "point", m, nrm, p, dmax, kind, k, R.SIZES_ITERS)
    with amd.Context() as ctx:
        setup(amd, ctx, "point", m, nrm, p, dmax, kind, k)
        for bad_kind, bad_k in ((4, 0.1), (-1, 0.1), (R.HUBER, 0.0), (R.HUBER, -1.0), (R.TUKEY, float("nan")),
                                (R.CAUCHY, float("inf")), (R.TUKEY, 1e200), (R.TUKEY, 1e-200)):
            with pytest.raises(amd.ICPError) as ei:
                ctx.set_robust(bad_kind, bad_k)
            assert ei.value.code == amd.ICP_E_ARG, (bad_kind, bad_k)
        with pytest.raises(amd.ICPError) as ei:  # no robust run yet
            ctx.robust_trace()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        res, errs = ctx.run(R.SIZES_ITERS, -1.0)  # (every refused call left Tukey, k)
        out = collect(ctx, res, errs, dmax, kind)
        bitwise(out, ref, keys=("errs", "scene", "R", "t", "s", "W", "Kpos"))
        L = amd.lib()
        w = np.full(8, -1.0)
        kp = np.full(8, -1, dtype=np.int64)
        wp, kpp = w.ctypes.data_as(C.POINTER(C.c_double)), kp.ctypes.data_as(C.POINTER(C.c_longlong))
        assert L.icp_get_robust_trace(ctx._h, wp, kpp, 2) == R.SIZES_ITERS  # cap < iterations: two entries
        np.testing.assert_array_equal(w[:2], out["W"][:2])
        np.testing.assert_array_equal(kp[:2], out["Kpos"][:2])
        assert np.all(w[2:] == -1.0) and np.all(kp[2:] == -1)
        assert L.icp_get_robust_trace(ctx._h, None, kpp, 8) == R.SIZES_ITERS  # cap > iterations, one array NULL
        np.testing.assert_array_equal(kp[:R.SIZES_ITERS], out["Kpos"])
        assert np.all(kp[R.SIZES_ITERS:] == -1) and np.all(w[2:] == -1.0)
        assert L.icp_get_robust_trace(ctx._h, None, None, 0) == R.SIZES_ITERS
        ctx.set_robust(R.NONE, float("nan"))  # (with NONE k is ignored)
        ctx.set_scene(p)  # the setting survives a new scene; the trace does not
        with pytest.raises(amd.ICPError) as ei:
            ctx.robust_trace()
        assert ei.value.code == amd.ICP_E_NO_MODEL


def test_reference_shaped_class_takes_robust(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, dmax, kind, k, _r = R.reference(oracle, ("size", "plane", R.CAUCHY, 257))
    ref = run(amd, "plane", m, nrm, p, dmax, kind, k, 3)
    icp = amd.ICP(m, p, 3, threshold=-1.0, normals=nrm, robust=(amd.ROBUST_CAUCHY, k))
    res = icp.find_corresponding_opti()
    assert res.iterations == 3
    np.testing.assert_array_equal(icp.errors, ref["errs"])
    np.testing.assert_array_equal(icp.new_p, ref["scene"])
    assert (amd.ROBUST_NONE, amd.ROBUST_HUBER, amd.ROBUST_TUKEY, amd.ROBUST_CAUCHY) == (0, 1, 2, 3)


# 9. CLI
def test_cli_robust(icp_lib, tmp_path):
    amd = icp_lib
    m, nrm, p, _inl = R.outlier_shell()
    paths = {k: str(tmp_path / (k + ".txt")) for k in ("model", "scene", "normals")}
    amd.write_matrix(paths["model"], m)
    amd.write_matrix(paths["scene"], p)
    amd.write_matrix(paths["normals"], nrm)
    exe = os.path.join(BUILD, "icp-gpu")
    base = [exe, paths["model"], paths["scene"], "12"]
    for metric, extra in (("point", []), ("plane", ["--normals", paths["normals"]])):
        f = str(tmp_path / (metric + "_f.txt"))
        r = subprocess.run(base + extra + ["--max-dist", str(R.SHELL_DMAX), "--robust", "tukey", "--robust-k",
                                           str(R.SHELL_K), "--out", f], cwd=tmp_path, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with amd.Context() as ctx:  # the rounded clouds: the input of both sides
            setup(amd, ctx, metric, amd.load_matrix(paths["model"]), amd.load_matrix(paths["normals"]),
                  amd.load_matrix(paths["scene"]), R.SHELL_DMAX, R.TUKEY, R.SHELL_K)
            res, _errs = ctx.run(12, 1e-5)
            g = str(tmp_path / (metric + "_g.txt"))
            amd.write_matrix(g, ctx.get_scene())
        assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
        assert open(f, "rb").read() == open(g, "rb").read()
    for bad in (["--robust", "tukey"], ["--robust-k", "0.06"], ["--robust", "welsch", "--robust-k", "0.06"],
                ["--robust", "tukey", "--robust-k", "abc"]):
        r = subprocess.run(base + bad, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 255 and "[error]" in r.stderr, (bad, r.returncode, r.stderr[-500:])
        assert "[load]" not in r.stderr  # (refused before any file is opened)
