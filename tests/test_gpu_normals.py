"""The model's k nearest neighbours over its grid and the normals estimated from them
(icp_model_knn, icp_estimate_model_normals, icp_get_model_normals; icp_normals.hip) against
tests/normals_ref.py, the same steps restated in numpy.

The neighbour lists and their distances are compared exactly.  The normals are compared where the
reference's eigenvalue gap ratio (l1 - l0) / l2 is at least 1e-3: |n . n_ref| >= 1 - 1e-9 (the
project's GPU-against-reference tolerance; the fp64 bound at that gap and k = 64 is about
64 x 1.1e-16 / 1e-3 = 7e-12), | |n| - 1 | <= 1e-12, and the sign where the sign rule's margin is at
least 1e-6.  tests/test_normals_ref.py checks on the CPU that these filters leave out at most 1 %
of the points, and that the fp64 reference sits within 1e-11 of extended precision.
"""
import os
import subprocess
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import datasets
import normals_ref as NR
import plane_ref as P
from test_gpu_gated import HostAllReduce
from test_gpu_plane import bitwise, check_against_ref, run_plane

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


def estimate(amd, m, k, view=None, **ctx_args):
    """-> (normals, degenerate count) of a fresh context"""
    with amd.Context(0, 0, **ctx_args) as ctx:
        ctx.set_model(m)
        deg = ctx.estimate_model_normals(k, view)
        return ctx.model_normals(), deg


# 1. the neighbour lists, element for element, and their distances, bit for bit
@pytest.mark.parametrize("name", NR.KNN_CASES)
def test_knn_exact(icp_lib, oracle, name):
    m, k, r = NR.reference(name, oracle.load_matrix)
    with icp_lib.Context() as ctx:
        ctx.set_model(m)
        idx, d2 = ctx.model_knn(k, distances=True)
        only_idx = ctx.model_knn(k)
    wrong = int((idx != r["idx"]).any(axis=1).sum())
    print(name, "n", m.shape[0], "k", k, "rows that differ", wrong, "ties at the k-th place", int(r["tie"].sum()))
    assert idx.shape == (m.shape[0], k) and idx.dtype == np.int32
    np.testing.assert_array_equal(idx, r["idx"])
    np.testing.assert_array_equal(d2, r["d2"])
    np.testing.assert_array_equal(only_idx, idx)


# 2. the normals
@pytest.mark.parametrize("view", [None, NR.VIEW])
@pytest.mark.parametrize("name", NR.CLEAR_CASES + tuple("ell257k%d" % k for k in NR.KS_AT_257) + ("ell64k64", "duplicates"))
def test_normals(icp_lib, oracle, name, view):
    m, k, r = NR.reference(name, oracle.load_matrix, view)
    n, deg = estimate(icp_lib, m, k, view)
    clear = r["gap"] >= NR.GAP_CLEAR
    dot = (n * r["normals"]).sum(axis=1)
    length = np.sqrt((n * n).sum(axis=1))
    signs = clear & (r["sign_margin"] >= NR.SIGN_CLEAR)
    print(name, view, "compared", int(clear.sum()), "of", clear.size, "least |n . n_ref|", np.abs(dot[clear]).min(),
          "largest | |n| - 1 |", np.abs(length[clear] - 1).max(), "signs compared", int(signs.sum()), "degenerate", deg)
    assert n.shape == m.shape
    assert np.all(np.abs(dot[clear]) >= 1 - 1e-9)
    assert np.all(np.abs(length[clear] - 1) <= 1e-12)
    assert np.all(dot[signs] > 0)
    if name in NR.CLEAR_CASES:
        assert deg == 0
    assert deg == int((~n.any(axis=1)).sum())
    if name == "planar":
        np.testing.assert_allclose(np.abs(n), np.tile([0.0, 0.0, 1.0], (m.shape[0], 1)), atol=1e-12)
        assert np.all(n[:, 2] > 0)  # (both rules: the largest component, and the viewpoint above the plane)


@pytest.mark.parametrize("name", ["line", "equal"])
def test_no_direction_gives_the_zero_normal(icp_lib, name):
    m, k, r = NR.reference(name)
    assert r["degenerate"] == m.shape[0]
    for view in (None, NR.VIEW):
        n, deg = estimate(icp_lib, m, k, view)
        assert deg == m.shape[0]
        np.testing.assert_array_equal(n, np.zeros_like(m))


# 3. determinism
def test_two_calls_and_two_contexts_give_the_same_bits(icp_lib):
    m, k, _r = NR.reference("ell4097")
    with icp_lib.Context() as ctx:
        ctx.set_model(m)
        ctx.estimate_model_normals(k)
        a = ctx.model_normals()
        ctx.estimate_model_normals(k)
        b = ctx.model_normals()
    c, _deg = estimate(icp_lib, m, k)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


# 4. the normals are the context's
def run_estimated(amd, m, p, k, dmax, iters, threshold=-1.0, variant=None):
    with amd.Context() as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        ctx.set_model(m)
        deg = ctx.estimate_model_normals(k)
        ctx.set_scene(p)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        if dmax:
            ctx.set_max_distance(dmax)
        nrm = ctx.model_normals()
        res, errs = ctx.run(iters, threshold)
        out = dict(res=res, errs=errs, scene=ctx.get_scene(), R=np.array(res.R).reshape(3, 3), t=np.array(res.t),
                   normals=nrm, degenerate=deg)
        if dmax:
            mask, kk = ctx.inliers()
            out.update(K=ctx.inlier_trace(), mask=mask, k=kk)
        return out


@pytest.mark.parametrize("n", [257, 4097])
def test_a_plane_run_on_estimated_normals(icp_lib, oracle, n):
    amd = icp_lib
    m, _nrm, p, _src = P.synth(n, 100 + n, 0.01)
    out = run_estimated(amd, m, p, 16, 0.0, 5)
    given = run_plane(amd, m, out["normals"], p, 0.0, 5)
    bitwise(out, given)
    r = P.plane_ref(oracle, m, out["normals"], p, 0.0, 5, -1.0)
    check_against_ref(m, out, r)
    icp = amd.ICP(m, p, 5, threshold=-1.0, estimate_normals=16)
    res = icp.find_corresponding_opti()
    assert res.iterations == 5 and icp.s == 1.0
    np.testing.assert_array_equal(icp.errors, out["errs"])
    np.testing.assert_array_equal(icp.new_p, out["scene"])
    np.testing.assert_array_equal(icp.r, out["R"])


# 5. the purpose: a different sample of the same surface, and no normals at hand
def test_estimated_normals_register_where_point_to_point_slides(icp_lib):
    amd = icp_lib
    m, _nrm, p, src = P.synth(4097, 4197, 0.0, other=True)
    out = run_estimated(amd, m, p, 16, 0.0, 5)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(10, -1.0)
        point = ctx.get_scene()
    dplane, dpoint = float(np.abs(out["scene"] - src).max()), float(np.abs(point - src).max())
    print("max |new_p - src|: plane on estimated normals, 5 iterations", dplane, "point-to-point, 10 iterations", dpoint)
    assert dplane < 0.1 * dpoint


# 6. life and errors
def test_life_and_errors(icp_lib):
    amd = icp_lib
    m, _nrm, p, _src = P.synth(257, 357, 0.01)
    with amd.Context() as ctx:
        for call in (lambda: ctx.estimate_model_normals(16), lambda: ctx.model_knn(16), ctx.model_normals):
            with pytest.raises(amd.ICPError) as ei:  # no model yet
                call()
            assert ei.value.code == amd.ICP_E_NO_MODEL
        ctx.set_model(m)
        ctx.set_scene(p)
        with pytest.raises(amd.ICPError) as ei:  # a model, no normals
            ctx.model_normals()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        assert ctx.estimate_model_normals(16) == 0
        before = ctx.model_normals()
        for k, view, word in ((2, None, "k = 2"), (65, None, "k = 65"), (258, None, "k = 258"),
                              (16, (0.0, np.nan, 1.0), "viewpoint[1]")):
            with pytest.raises(amd.ICPError) as ei:
                ctx.estimate_model_normals(k, view)
            print(str(ei.value))
            assert ei.value.code == amd.ICP_E_ARG and word in str(ei.value)
            if view is None:
                with pytest.raises(amd.ICPError) as ei:
                    ctx.model_knn(k)
                assert ei.value.code == amd.ICP_E_ARG and word in str(ei.value)
        assert amd.lib().icp_get_model_normals(ctx._h, None) == amd.ICP_E_ARG  # a null required pointer
        assert amd.lib().icp_model_knn(ctx._h, 16, None, None) == amd.ICP_E_ARG
        np.testing.assert_array_equal(ctx.get_scene(), p)  # (none of the refused calls ran anything)
        np.testing.assert_array_equal(ctx.model_normals(), before)
        assert not ctx.ensure_model(m)  # the same model: the normals stay
        np.testing.assert_array_equal(ctx.model_normals(), before)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        res, _errs = ctx.run(2, -1.0)
        assert res.iterations == 2
        ctx.set_model(m)  # a model upload drops them
        ctx.set_scene(p)
        with pytest.raises(amd.ICPError) as ei:
            ctx.model_normals()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(2, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL


def test_planar_model_stops_a_plane_run(icp_lib):
    amd = icp_lib
    m, _nrm, p = P.planar()
    with amd.Context() as ctx:
        ctx.set_model(m)
        assert ctx.estimate_model_normals(16) == 0
        ctx.set_scene(p)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(5, -1.0)
        print(str(ei.value))
        assert ei.value.code == amd.ICP_E_DEGENERATE
        assert "iteration 0" in str(ei.value) and "pivot" in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)


# 7. off is off: an estimate leaves everything a run reads as it found it
@pytest.mark.parametrize("case", ["cow", "grid4097"])
def test_off_is_off(icp_lib, oracle, case):
    amd = icp_lib
    if case == "cow":
        m = oracle.load_matrix(datasets.path("cow_ref"))
        p = oracle.load_matrix(datasets.path("cow_tr1"))
    else:
        m, _nrm, p, _src = P.synth(4097, 4197, 0.01)
    runs = []
    for form in ("fresh", "estimated"):
        with amd.Context() as ctx:
            if case != "cow":
                ctx.set_nn_variant(amd.VARIANT_GRID)
            ctx.set_model(m)
            ctx.set_scene(p)
            if form == "estimated":
                ctx.estimate_model_normals(16)
                ctx.model_knn(16)
            res, errs = ctx.run(10)
            st = ctx.stats()
            if case == "cow":
                assert st["persistent_runs"] == 1
            runs.append((errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t), ctx.get_indices(),
                         [st[key] for key in ("persistent_runs", "iterations", "ambiguous", "grid_fallback",
                                              "run_grid_searches", "run_certified", "run_walked")]))
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)


# 8. ranks: the model is replicated, so every rank estimates the same normals
def run_estimated_sharded(amd, m, p, k, dmax, world, iters):
    red = HostAllReduce(world)
    results = [None] * world
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                ctx.set_model(m)
                ctx.estimate_model_normals(k)
                ctx.set_scene(p[b:b + c], np_total=p.shape[0])
                ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
                ctx.set_max_distance(dmax)
                nrm = ctx.model_normals()
                res, errs = ctx.run(iters, -1.0)
                mask, kk = ctx.inliers()
                results[r] = dict(res=res, errs=errs, scene=ctx.get_scene(), R=np.array(res.R), K=ctx.inlier_trace(),
                                  mask=mask, k=kk, normals=nrm)
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


@pytest.fixture(scope="module")
def gate_single(icp_lib, oracle):
    m, _nrm, p, dmax, _r = P.reference(oracle, ("gate", 4097, 0.08))
    return run_estimated(icp_lib, m, p, 16, dmax, P.GATES_ITERS)


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_match_single(icp_lib, oracle, gate_single, world):
    m, _nrm, p, dmax, _r = P.reference(oracle, ("gate", 4097, 0.08))
    ref = gate_single
    out = run_estimated_sharded(icp_lib, m, p, 16, dmax, world, P.GATES_ITERS)
    print("single", ref["errs"], "ranks", out[0]["errs"], "K", list(ref["K"]))
    for o in out:
        np.testing.assert_array_equal(o["normals"], ref["normals"])
        np.testing.assert_array_equal(o["errs"], out[0]["errs"])
        np.testing.assert_array_equal(o["K"], out[0]["K"])
        np.testing.assert_array_equal(o["R"], out[0]["R"])
        assert o["k"] == out[0]["k"]
    assert out[0]["res"].iterations == ref["res"].iterations
    np.testing.assert_array_equal(out[0]["K"], ref["K"])
    assert out[0]["k"] == ref["k"]
    np.testing.assert_allclose(out[0]["errs"], ref["errs"], rtol=1e-11)
    np.testing.assert_array_equal(np.concatenate([o["mask"] for o in out]), ref["mask"])
    np.testing.assert_allclose(np.concatenate([o["scene"] for o in out]), ref["scene"], atol=1e-12)


# 9. CLI
def test_cli_estimates_and_writes_normals(icp_lib, tmp_path):
    amd = icp_lib
    cow, tr = datasets.path("cow_ref"), datasets.path("cow_tr1")
    f, g, nf, ng = (str(tmp_path / name) for name in ("f.txt", "g.txt", "n.txt", "ng.txt"))
    exe = os.path.join(BUILD, "icp-gpu")
    r = subprocess.run([exe, cow, tr, "20", "--estimate-normals", "16", "--write-normals", nf, "--out", f], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:
        ctx.set_model(amd.load_matrix(cow))
        ctx.set_scene(amd.load_matrix(tr))
        ctx.estimate_model_normals(16)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        res, _errs = ctx.run(20, 1e-5)
        amd.write_matrix(g, ctx.get_scene())
        amd.write_matrix(ng, ctx.model_normals())
    assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
    assert open(f, "rb").read() == open(g, "rb").read()
    np.testing.assert_array_equal(amd.load_matrix(nf), amd.load_matrix(ng))
    for extra in (["--estimate-normals", "2"], ["--estimate-normals", "16", "--normals", nf]):
        r = subprocess.run([exe, cow, tr, "20"] + extra + ["--out", f], cwd=tmp_path, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0 and "[error]" in r.stderr, (extra, r.stderr[-500:])
