"""icp_run with the point-to-plane metric (icp_set_metric, icp_plane.hip) against
tests/plane_ref.py, the loop restated with the oracle's search and numpy.

Tolerances are test_gpu_gated.py's: K per iteration and the masks exact
(tests/test_plane_ref.py checks on the CPU that no pair of these inputs lies within 1e-6 of the
gate, and that the fp64 reference sits within 1e-11 of extended precision), err rel 1e-9, R abs
1e-9, t and new_p abs 1e-9 x extent.
"""
import os
import subprocess
import threading

import numpy as np
import pytest
import torch  # (before the first HIP call of the session: torch then sees the device)

import datasets
import plane_ref as P
from test_gpu_gated import HostAllReduce

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


def setup_plane(amd, ctx, m, nrm, p, dmax, np_total=None):
    ctx.set_model(m)
    ctx.set_model_normals(nrm)
    ctx.set_scene(p, np_total=np_total)
    ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
    if dmax:
        ctx.set_max_distance(dmax)


def run_plane(amd, m, nrm, p, dmax, iters, threshold=-1.0, mode=0, variant=None, **ctx_args):
    """-> dict(res, errs, scene, R, t, and with a gate K (trace), mask, k) of a fresh context."""
    with amd.Context(0, mode, **ctx_args) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        setup_plane(amd, ctx, m, nrm, p, dmax)
        res, errs = ctx.run(iters, threshold)
        out = dict(res=res, errs=errs, scene=ctx.get_scene(), R=np.array(res.R).reshape(3, 3), t=np.array(res.t))
        if dmax:
            mask, k = ctx.inliers()
            out.update(K=ctx.inlier_trace(), mask=mask, k=k)
        return out


def check_against_ref(m, out, r):
    print("err", out["errs"], "ref err", r["err"], "K", list(out.get("K", [])))
    assert out["res"].iterations == r["iterations"]
    assert out["res"].s == 1.0
    np.testing.assert_allclose(out["errs"], r["err"], rtol=1e-9)
    np.testing.assert_allclose(out["R"], r["R"], atol=1e-9)
    np.testing.assert_allclose(out["R"] @ out["R"].T, np.eye(3), atol=1e-14)
    extent = float(np.abs(m).max())
    np.testing.assert_allclose(out["t"], r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(out["scene"], r["new_p"], atol=1e-9 * extent)
    if "K" in out:
        assert list(out["K"]) == r["K"] and out["k"] == r["K"][-1]
        np.testing.assert_array_equal(out["mask"], r["mask"])
        assert out["mask"].sum() == out["k"]


def bitwise(a, b):
    for key in ("errs", "scene", "R", "t") + (("K", "mask") if "K" in a else ()):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# 1. sizes: the wave tail, one workgroup, kRedSingle, the first multi-workgroup fold, an odd
# multi-block size; n = 6 sits on the minimum K
@pytest.mark.parametrize("n", P.SIZES)
def test_sizes(icp_lib, oracle, n):
    m, nrm, p, dmax, r = P.reference(oracle, ("size", n))
    out = run_plane(icp_lib, m, nrm, p, dmax, P.SIZES_ITERS)
    check_against_ref(m, out, r)


# 2. the kernels do not depend on which search ran, and a run is deterministic
def test_variants_bitwise_at_4097(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, dmax, _r = P.reference(oracle, ("size", 4097))
    a = run_plane(amd, m, nrm, p, dmax, P.SIZES_ITERS)
    bitwise(run_plane(amd, m, nrm, p, dmax, P.SIZES_ITERS), a)
    for mode, variant in ((amd.NN_FP64, None), (amd.NN_CERTIFIED, amd.VARIANT_GRID)):
        bitwise(run_plane(amd, m, nrm, p, dmax, P.SIZES_ITERS, mode=mode, variant=variant), a)


# 3. with the gate
@pytest.fixture(scope="module")
def gate_single(icp_lib, oracle):
    m, nrm, p, dmax, _r = P.reference(oracle, ("gate", 4097, 0.08))
    return run_plane(icp_lib, m, nrm, p, dmax, P.GATES_ITERS)


@pytest.mark.parametrize("n,dmax", list(P.GATES))
def test_gate(icp_lib, oracle, gate_single, n, dmax):
    m, nrm, p, d, r = P.reference(oracle, ("gate", n, dmax))
    out = gate_single if n == 4097 else run_plane(icp_lib, m, nrm, p, d, P.GATES_ITERS)
    check_against_ref(m, out, r)
    assert list(out["K"]) == P.GATES[(n, dmax)]


# 4. the purpose: a different sample of the same surface
def test_plane_registers_where_point_to_point_slides(icp_lib):
    amd = icp_lib
    m, nrm, p, src = P.synth(4097, 4197, 0.0, other=True)
    out = run_plane(amd, m, nrm, p, 0.0, 5)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(10, -1.0)
        point = ctx.get_scene()
    dplane, dpoint = float(np.abs(out["scene"] - src).max()), float(np.abs(point - src).max())
    print("max |new_p - src|: plane, 5 iterations", dplane, "point-to-point, 10 iterations", dpoint)
    assert dplane < 1e-3
    assert dpoint > 1e-2


# 5. too few, degenerate: the run stops before the iteration changes anything
@pytest.mark.parametrize("case", ["few", "degenerate"])
def test_stops_before_the_iteration(icp_lib, case):
    amd = icp_lib
    m, nrm, p = P.five() if case == "few" else P.planar()
    with amd.Context() as ctx:
        setup_plane(amd, ctx, m, nrm, p, 0.0)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(5, -1.0)
        print(str(ei.value))
        assert ei.value.code == (amd.ICP_E_TOO_FEW_POINTS if case == "few" else amd.ICP_E_DEGENERATE)
        assert "iteration 0" in str(ei.value)
        assert ("K = 5" if case == "few" else "pivot") in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)


# 6. the normals' life
def test_normals_hygiene(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, dmax, _r = P.reference(oracle, ("size", 257))
    ref = run_plane(amd, m, nrm, p, dmax, 3)
    with amd.Context() as ctx:
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        with pytest.raises(amd.ICPError) as ei:  # no model yet
            ctx.set_model_normals(nrm)
        assert ei.value.code == amd.ICP_E_NO_MODEL
        ctx.set_model(m)
        ctx.set_scene(p)
        with pytest.raises(amd.ICPError) as ei:  # no normals
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL and "icp_set_model_normals" in str(ei.value)
        with pytest.raises(amd.ICPError) as ei:
            ctx.set_model_normals(nrm[:-1])
        assert ei.value.code == amd.ICP_E_SIZE_MISMATCH
        bad = nrm.copy()
        bad[100, 1] = np.nan
        with pytest.raises(amd.ICPError) as ei:
            ctx.set_model_normals(bad)
        assert ei.value.code == amd.ICP_E_ARG
        with pytest.raises(amd.ICPError) as ei:
            ctx.set_metric(2)
        assert ei.value.code == amd.ICP_E_ARG
        np.testing.assert_array_equal(ctx.get_scene(), p)  # (none of the refused calls ran anything)
        ctx.set_model_normals(nrm)
        assert not ctx.ensure_model(m)  # the same model: the normals stay
        res, errs = ctx.run(3, -1.0)
        np.testing.assert_array_equal(errs, ref["errs"])
        np.testing.assert_array_equal(ctx.get_scene(), ref["scene"])
        ctx.set_model(m)  # a model upload drops them
        ctx.set_scene(p)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL
        dn = torch.from_numpy(nrm).to("cuda:0")  # the device setter: the host setter's run bit for bit
        torch.cuda.synchronize()
        ctx.set_model_normals_device(dn.data_ptr(), nrm.shape[0])
        res, errs = ctx.run(3, -1.0)
        np.testing.assert_array_equal(errs, ref["errs"])
        np.testing.assert_array_equal(ctx.get_scene(), ref["scene"])
        np.testing.assert_array_equal(np.array(res.R).reshape(3, 3), ref["R"])


def test_reference_shaped_class_takes_normals(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, dmax, _r = P.reference(oracle, ("size", 257))
    ref = run_plane(amd, m, nrm, p, dmax, 3)
    icp = amd.ICP(m, p, 3, threshold=-1.0, normals=nrm)
    res = icp.find_corresponding_opti()
    assert res.iterations == 3 and icp.s == 1.0
    np.testing.assert_array_equal(icp.errors, ref["errs"])
    np.testing.assert_array_equal(icp.new_p, ref["scene"])
    np.testing.assert_array_equal(icp.r, ref["R"])


# 7. off is off
def cow_normals(n):
    v = np.random.default_rng(11).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_off_is_off(icp_lib, oracle):
    amd = icp_lib
    m = oracle.load_matrix(datasets.path("cow_ref"))
    p = oracle.load_matrix(datasets.path("cow_tr1"))
    runs = []
    for form in ("fresh", "set", "after_plane"):
        with amd.Context() as ctx:
            ctx.set_model(m)
            ctx.set_scene(p)
            if form == "set":
                ctx.set_metric(amd.METRIC_POINT_TO_POINT)
            if form == "after_plane":
                ctx.set_model_normals(cow_normals(m.shape[0]))
                ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
                res, _errs = ctx.run(3, -1.0)
                assert res.iterations == 3 and res.s == 1.0 and ctx.stats()["persistent_runs"] == 0
                ctx.set_metric(amd.METRIC_POINT_TO_POINT)
                ctx.set_scene(p)
            res, errs = ctx.run(10)
            assert ctx.stats()["persistent_runs"] == 1
            with pytest.raises(amd.ICPError) as ei:  # (an ungated plane run is not a gated run)
                ctx.inliers()
            assert ei.value.code == amd.ICP_E_NO_MODEL
            runs.append((errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)


def test_point_to_point_run_after_a_plane_one(icp_lib, oracle):
    """Plane 3, metric off, point-to-point 5 on one context == point-to-point 5 on a fresh context
    loaded with the scene the 3 plane iterations left, bit for bit."""
    amd = icp_lib
    m = oracle.load_matrix(datasets.path("cow_ref"))
    p = oracle.load_matrix(datasets.path("cow_tr2"))
    with amd.Context() as ctx:
        setup_plane(amd, ctx, m, cow_normals(m.shape[0]), p, 0.0)
        ctx.run(3, -1.0)
        mid = ctx.get_scene()
        ctx.set_metric(amd.METRIC_POINT_TO_POINT)
        res_a, errs_a = ctx.run(5, -1.0)
        scene_a = ctx.get_scene()
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(mid)
        res_b, errs_b = ctx.run(5, -1.0)
        scene_b = ctx.get_scene()
    np.testing.assert_array_equal(errs_a, errs_b)
    np.testing.assert_array_equal(scene_a, scene_b)
    np.testing.assert_array_equal(np.array(res_a.R), np.array(res_b.R))


def test_last_gate_survives_an_ungated_plane_run(icp_lib, oracle):
    """The gated and the plane loop share their run-scoped buffers (mask, state, K trace); what
    inliers() and inlier_trace() report is the last gated run's all the same: unchanged by an
    ungated plane run on the same scene, replaced by the next gated run, dropped by set_scene.

    The ungated plane run pairs the quarter of this scene that lies 4 away as well, and its three
    iterations throw the scene off the model: every point ends more than 5.5 from it (plane_ref on
    the CPU: err 1.5, 5.4, 2.7), so the gated plane run that follows on that scene keeps K = 0 pairs
    at iteration 0 and stops -- that stop is what the getters then report.  A gated plane run that
    records its iterations comes after a set_scene: its K are the reference's."""
    amd = icp_lib
    m, nrm, p, dmax, r = P.reference(oracle, ("gate", 4097, 0.08))
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.set_max_distance(dmax)
        res, _errs = ctx.run(4, -1.0)  # 1. gated, point-to-point
        mask1, k1 = ctx.inliers()
        trace1 = ctx.inlier_trace()
        print("K", list(trace1))
        assert res.iterations == 4 and trace1.size == 4 and mask1.sum() == k1 == trace1[-1] and 4 <= k1 < p.shape[0]
        ctx.set_max_distance(0.0)  # 2. ungated, point-to-plane, no set_scene: every pair kept, nothing reported
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        res, _errs = ctx.run(3, -1.0)
        assert res.iterations == 3
        mask2, k2 = ctx.inliers()
        np.testing.assert_array_equal(mask2, mask1)
        assert k2 == k1
        np.testing.assert_array_equal(ctx.inlier_trace(), trace1)
        ctx.set_max_distance(dmax)  # 3. gated, point-to-plane, the scene where it is: this run's stop
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS and "iteration 0" in str(ei.value) and "K = 0" in str(ei.value)
        mask3, k3 = ctx.inliers()
        assert k3 == 0 and not mask3.any() and ctx.inlier_trace().size == 0
        ctx.set_scene(p)  # ... and from the scene as given: this run's three iterations
        res, _errs = ctx.run(3, -1.0)
        mask3, k3 = ctx.inliers()
        trace3 = ctx.inlier_trace()
        print("K", list(trace3))
        assert res.iterations == 3 and list(trace3) == r["K"][:3]
        assert mask3.sum() == k3 == trace3[-1] and 6 <= k3 < p.shape[0]
        ctx.set_scene(p)  # 4. a new scene: no gated run since
        for getter in (ctx.inliers, ctx.inlier_trace):
            with pytest.raises(amd.ICPError) as ei:
                getter()
            assert ei.value.code == amd.ICP_E_NO_MODEL


# 8. a scene in slot order, correspondences with kd positions
def test_plane_run_on_a_scene_in_slot_order(icp_lib):
    """Two point-to-point iterations at 65,536 points leave the scene in slot order and the bundle
    search's kd positions; three gated plane iterations on that context against three on a fresh
    context given the same scene (file order).  The normals are fixed unit vectors: the metric's
    arithmetic does not care that they are not a surface's.  The two runs sum in different orders,
    so K and the mask (the caller's order) are compared exactly and the rest to rounding, as in
    test_gpu_gated.py (b)."""
    amd = icp_lib
    n = 65536
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    nrm = r.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    dmax = 0.05
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.run(2, -1.0)
        mid = ctx.get_scene()
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_max_distance(dmax)
        res_a, errs_a = ctx.run(3, -1.0)
        ka, (mask_a, cnt_a), scene_a = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene()
    b = run_plane(amd, m, nrm, mid, dmax, 3)
    print("K", list(ka), list(b["K"]), "err", errs_a, b["errs"])
    assert res_a.iterations == b["res"].iterations == 3
    np.testing.assert_array_equal(ka, b["K"])
    assert cnt_a == b["k"] == ka[-1] and 6 <= cnt_a < n
    np.testing.assert_array_equal(mask_a, b["mask"])
    assert mask_a.sum() == cnt_a
    np.testing.assert_allclose(errs_a, b["errs"], rtol=1e-11)
    np.testing.assert_allclose(scene_a, b["scene"], atol=1e-12)


# 9. ranks
def run_plane_sharded(amd, m, nrm, p, dmax, world, iters):
    red = HostAllReduce(world)
    results = [None] * world
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                setup_plane(amd, ctx, m, nrm, p[b:b + c], dmax, np_total=p.shape[0])
                res, errs = ctx.run(iters, -1.0)
                mask, k = ctx.inliers()
                results[r] = dict(res=res, errs=errs, scene=ctx.get_scene(), R=np.array(res.R), K=ctx.inlier_trace(),
                                  mask=mask, k=k)
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
def test_ranks_match_single(icp_lib, oracle, gate_single, world):
    m, nrm, p, dmax, _r = P.reference(oracle, ("gate", 4097, 0.08))
    ref = gate_single
    out = run_plane_sharded(icp_lib, m, nrm, p, dmax, world, P.GATES_ITERS)
    print("single", ref["errs"], "ranks", out[0]["errs"])
    for o in out:  # identical decisions and solves on every rank
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


def test_rccl_single_rank_communicator(icp_lib, oracle, gate_single):
    """The 28 sums and the residual all-reduce through ncclAllReduce on a 1-rank communicator: the
    identity, so the run is the plain context's bit for bit."""
    amd = icp_lib
    m, nrm, p, dmax, _r = P.reference(oracle, ("gate", 4097, 0.08))
    out = run_plane(amd, m, nrm, p, dmax, P.GATES_ITERS, rank=0, world_size=1, rccl_id=amd.rccl_unique_id())
    bitwise(out, gate_single)
    assert out["k"] == gate_single["k"]


# 10. CLI
def test_cli_normals(icp_lib, tmp_path):
    amd = icp_lib
    m, nrm, p, _src = P.synth(257, 357, 0.01)
    paths = {k: str(tmp_path / (k + ".txt")) for k in ("model", "scene", "normals", "short")}
    amd.write_matrix(paths["model"], m)
    amd.write_matrix(paths["scene"], p)
    amd.write_matrix(paths["normals"], nrm)
    amd.write_matrix(paths["short"], nrm[:-1])
    f = str(tmp_path / "f.txt")
    r = subprocess.run([os.path.join(BUILD, "icp-gpu"), paths["model"], paths["scene"], "20", "--normals",
                        paths["normals"], "--out", f], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:  # the rounded clouds: the input of both sides
        setup_plane(amd, ctx, amd.load_matrix(paths["model"]), amd.load_matrix(paths["normals"]),
                    amd.load_matrix(paths["scene"]), 0.0)
        res, _errs = ctx.run(20, 1e-5)
        g = str(tmp_path / "g.txt")
        amd.write_matrix(g, ctx.get_scene())
    assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
    assert open(f, "rb").read() == open(g, "rb").read()
    r = subprocess.run([os.path.join(BUILD, "icp-gpu"), paths["model"], paths["scene"], "20", "--normals",
                        paths["short"], "--out", f], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "[error]" in r.stderr


# 11. instrumentation
def test_index_digest_and_progress_under_the_plane_loop(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, d, _r = P.reference(oracle, ("gate", 257, 0.08))
    plain = run_plane(amd, m, nrm, p, d, P.GATES_ITERS)
    seen = []
    with amd.Context() as ctx:
        setup_plane(amd, ctx, m, nrm, p, d)
        ctx.set_index_digest(P.GATES_ITERS)
        ctx.set_progress(lambda i, e: seen.append((i, e)))
        res, errs = ctx.run(P.GATES_ITERS, -1.0)
        dig = ctx.index_digest()
        idx = ctx.get_indices().astype(np.uint64)
        scene = ctx.get_scene()
    np.testing.assert_array_equal(errs, plain["errs"])
    np.testing.assert_array_equal(scene, plain["scene"])
    assert [i for i, _ in seen] == list(range(P.GATES_ITERS))
    np.testing.assert_array_equal([e for _, e in seen], errs)
    j = np.arange(idx.size, dtype=np.uint64)
    want = np.array([idx.sum(), ((j + np.uint64(1)) * idx).sum(), (idx == j).sum()], dtype=np.uint64)
    np.testing.assert_array_equal(dig[-1], want)  # (the last search's correspondences)
    assert np.all(dig[:, 0] > 0)
