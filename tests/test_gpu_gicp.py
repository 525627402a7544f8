"""icp_run with the plane-to-plane iteration (icp_set_plane_to_plane, icp_gicp.hip: generalised ICP from
both clouds' normals) against tests/gicp_ref.py, the loop restated with the oracle's search and numpy.

Tolerances are test_gpu_symm.py's: K per iteration and the masks exact
(tests/test_gicp_ref.py checks on the CPU that no pair of these inputs lies within 1e-6 of the gate, of
the trim's cut or of Tukey's k), err rel 1e-9 or within (1e-9 x extent)^2 absolutely, R abs 1e-9, t and
new_p abs 1e-9 x extent; the reference agrees with its extended-precision twin to under 1 % of them.
"""
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import datasets
import gicp_ref as G
import plane_ref as P
import symm_ref as S
import test_gpu_symm as TS
from test_gpu_gated import HostAllReduce

pytestmark = pytest.mark.gpu


def setup_gicp(amd, ctx, m, nrm, p, U0, dmax, eps=G.EPS, np_total=None, trim=None, robust=None):
    ctx.set_model(m)
    ctx.set_model_normals(nrm)
    ctx.set_scene(p, np_total=np_total)
    if U0 is not None:
        ctx.set_scene_normals(U0)
    ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
    ctx.set_plane_to_plane(eps)
    if dmax:
        ctx.set_max_distance(dmax)
    if trim is not None:
        ctx.set_trim(trim)
    if robust is not None:
        ctx.set_robust(*robust)


def run_gicp(amd, m, nrm, p, U0, dmax, iters, threshold=-1.0, mode=0, variant=None, eps=G.EPS, trim=None, robust=None,
             **ctx_args):
    """-> dict(res, errs, scene, R, t, and with a gate or a trim K (trace), mask, k) of a fresh context."""
    with amd.Context(0, mode, **ctx_args) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        setup_gicp(amd, ctx, m, nrm, p, U0, dmax, eps, trim=trim, robust=robust)
        res, errs = ctx.run(iters, threshold)
        return TS.collect(ctx, res, errs, bool(dmax) or trim is not None)


# 1. sizes: below a wave, the wave's tail, one workgroup, the first multi-workgroup fold, an odd multi-block size
@pytest.mark.parametrize("n", G.SIZES)
def test_sizes(icp_lib, oracle, n):
    m, nrm, p, U0, dmax, r = G.reference(oracle, ("size", n))
    out = run_gicp(icp_lib, m, nrm, p, U0, dmax, G.SIZES_ITERS)
    TS.check_against_ref(m, out, r)


# 2. the kernels do not depend on which search ran, and a run is deterministic
def test_variants_bitwise_at_2049(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = G.reference(oracle, ("size", 2049))
    a = run_gicp(amd, m, nrm, p, U0, dmax, G.SIZES_ITERS)
    TS.bitwise(run_gicp(amd, m, nrm, p, U0, dmax, G.SIZES_ITERS), a)
    for mode, variant in ((amd.NN_FP64, None), (amd.NN_CERTIFIED, amd.VARIANT_GRID)):
        TS.bitwise(run_gicp(amd, m, nrm, p, U0, dmax, G.SIZES_ITERS, mode=mode, variant=variant), a)


# 3. the gate with the trim, and with robust weights of the Mahalanobis residual
@pytest.fixture(scope="module")
def tukey_single(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, d, _r = G.reference(oracle, ("tukey",))
    with amd.Context() as ctx:
        setup_gicp(amd, ctx, m, nrm, p, U0, d, robust=(amd.ROBUST_TUKEY, G.TUKEY_K))
        res, errs = ctx.run(G.GATE_ITERS, -1.0)
        out = TS.collect(ctx, res, errs, True)
        out["W"], out["Kpos"] = ctx.robust_trace()
    return out


def test_gate_with_a_trim(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, d, r = G.reference(oracle, ("trim",))
    with amd.Context() as ctx:
        setup_gicp(amd, ctx, m, nrm, p, U0, d, trim=G.TRIM)
        res, errs = ctx.run(G.GATE_ITERS, -1.0)
        out = TS.collect(ctx, res, errs, True)
        C = ctx.trim_trace()
    TS.check_against_ref(m, out, r)
    print("C", list(C), r["C"])
    np.testing.assert_allclose(C, r["C"], rtol=1e-9)


def test_gate_with_tukey_weights(oracle, tukey_single):
    m, _nrm, _p, _U0, _d, r = G.reference(oracle, ("tukey",))
    TS.check_against_ref(m, tukey_single, r)
    print("K+", list(tukey_single["Kpos"]), "W", list(tukey_single["W"]))
    assert list(tukey_single["Kpos"]) == r["Kpos"]
    np.testing.assert_allclose(tukey_single["W"], r["W"], rtol=1e-9)


# 4. the purpose inputs, with the reference's thresholds
def test_lands_nearer_than_point_to_plane_on_a_curved_surface(icp_lib):
    amd = icp_lib
    m, nrm, p, U0, src = S.purpose()
    out = run_gicp(amd, m, nrm, p, U0, 0.0, 5)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.run(8, -1.0)
        plane = ctx.get_scene()
    dg, dplane = float(np.abs(out["scene"] - src).max()), float(np.abs(plane - src).max())
    print("max |new_p - src|: plane-to-plane, 5 iterations", dg, "point-to-plane, 8 iterations", dplane, "err", out["errs"])
    assert dg * G.PURPOSE_FACTOR < dplane
    assert 5e-4 < out["errs"][-1] < 2e-3  # (the tangential distance between two samplings, at weight 1/2)


def test_planar_model_registers_here_and_is_degenerate_with_the_switch_off(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, _R, _t = G.planar_L()
    r = G.gicp_ref(oracle, m, nrm, p, U0, G.EPS, 0.0, 5, -1.0)
    out = run_gicp(amd, m, nrm, p, U0, 0.0, 5)
    TS.check_against_ref(m, out, r)
    back = float(np.abs(out["scene"] - m).max())
    print("max |new_p - model|", back)
    assert back <= 1e-12 * float(np.abs(m).max())
    for symmetric in (False, True):
        with amd.Context() as ctx:
            setup_gicp(amd, ctx, m, nrm, p, U0, 0.0, eps=0.0)
            ctx.set_plane_symmetric(symmetric)
            with pytest.raises(amd.ICPError) as ei:
                ctx.run(5, -1.0)
            assert ei.value.code == amd.ICP_E_DEGENERATE


# 5. signs, zeros and a normal that is not a unit vector
def test_the_sign_of_a_normal_changes_no_bit(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = G.reference(oracle, ("size", 2049))
    a = run_gicp(amd, m, nrm, p, U0, dmax, G.SIZES_ITERS)
    flip = np.where(np.random.default_rng(2).random(2049) < 0.5, -1.0, 1.0)[:, None]
    TS.bitwise(run_gicp(amd, m, nrm, p, U0 * flip, dmax, G.SIZES_ITERS), a)
    TS.bitwise(run_gicp(amd, m, nrm * flip, p, U0, dmax, G.SIZES_ITERS), a)


def test_zero_normals_leave_the_identity(icp_lib, oracle):
    m, nrm, p, U0, _dmax, _r = G.reference(oracle, ("size", 257))
    idx = oracle.closest(p, m)[1]
    N0, U00 = nrm.copy(), U0.copy()
    N0[idx[7]] = 0.0  # the model's normal of scene point 7's first pair ...
    U00[7] = 0.0  # ... whose own is zero too: both zero, S = 2 I
    assert idx[11] != idx[7] and idx[13] != idx[7]
    U00[11] = 0.0  # one cloud only: the scene's
    N0[idx[13]] = 0.0  # one cloud only: the model's
    r = G.gicp_ref(oracle, m, N0, p, U00, G.EPS, 0.0, G.SIZES_ITERS, -1.0)
    out = run_gicp(icp_lib, m, N0, p, U00, 0.0, G.SIZES_ITERS)
    TS.check_against_ref(m, out, r)
    assert not np.array_equal(out["errs"], run_gicp(icp_lib, m, nrm, p, U0, 0.0, G.SIZES_ITERS)["errs"])


def test_a_normal_of_length_40_counts_in_K_only(icp_lib, oracle):
    """S = 2 I - k1 (N N^T + u u^T) is indefinite for |N| = 40: the pair counts in K and adds nothing else,
    as the reference restates; the wide gate is there for the K trace."""
    m, nrm, p, U0, _dmax, _r = G.reference(oracle, ("size", 257))
    idx = oracle.closest(p, m)[1]
    N40 = nrm.copy()
    N40[idx[7]] *= 40.0
    r = G.gicp_ref(oracle, m, N40, p, U0, G.EPS, 10.0, G.SIZES_ITERS, -1.0)
    out = run_gicp(icp_lib, m, N40, p, U0, 10.0, G.SIZES_ITERS)
    TS.check_against_ref(m, out, r)
    assert list(out["K"]) == [257] * G.SIZES_ITERS
    assert not np.array_equal(out["errs"], run_gicp(icp_lib, m, nrm, p, U0, 10.0, G.SIZES_ITERS)["errs"])


# 6. too few: the run stops before the iteration changes anything
def test_too_few_under_a_tight_gate(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, _dmax, _r = G.reference(oracle, ("size", 257))
    d2 = np.sort(((p - m[oracle.closest(p, m)[1]]) ** 2).sum(axis=1))
    dmax = float(np.sqrt(0.5 * (d2[4] + d2[5])))  # five pairs within it
    with amd.Context() as ctx:
        setup_gicp(amd, ctx, m, nrm, p, U0, dmax)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(5, -1.0)
        print(str(ei.value))
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS
        assert "iteration 0" in str(ei.value) and "K = 5" in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)
        np.testing.assert_array_equal(ctx.scene_normals(), U0)
        _s, Rt, tt = ctx.transform()
        np.testing.assert_array_equal(Rt, np.eye(3))
        np.testing.assert_array_equal(tt, np.zeros(3))


# 7. the switch's life
def plain_run(amd, m, nrm, p, U0, metric, symmetric, eps, iters=3):
    with amd.Context() as ctx:
        if eps is not None:
            ctx.set_plane_to_plane(eps)  # (before the clouds: the setting survives icp_set_model / icp_set_scene)
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.set_scene_normals(U0)
        ctx.set_metric(metric)
        ctx.set_plane_symmetric(symmetric)
        res, errs = ctx.run(iters, -1.0)
        return dict(errs=errs, scene=ctx.get_scene(), R=np.array(res.R).reshape(3, 3), t=np.array(res.t))


def test_off_is_off_and_point_to_point_ignores_the_switch(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, _d, _r = G.reference(oracle, ("size", 2049))
    for symmetric in (False, True):  # epsilon = 0: a plane run and a symmetric run are what they are without the call
        TS.bitwise(plain_run(amd, m, nrm, p, U0, amd.METRIC_POINT_TO_PLANE, symmetric, 0.0),
                   plain_run(amd, m, nrm, p, U0, amd.METRIC_POINT_TO_PLANE, symmetric, None))
    TS.bitwise(plain_run(amd, m, nrm, p, U0, amd.METRIC_POINT_TO_POINT, False, G.EPS),
               plain_run(amd, m, nrm, p, U0, amd.METRIC_POINT_TO_POINT, False, None))
    on = plain_run(amd, m, nrm, p, U0, amd.METRIC_POINT_TO_PLANE, False, G.EPS)  # set before the clouds: it survived
    TS.bitwise(on, run_gicp(amd, m, nrm, p, U0, 0.0, 3))
    assert not np.array_equal(on["errs"], plain_run(amd, m, nrm, p, U0, amd.METRIC_POINT_TO_PLANE, False, None)["errs"])


def test_point_to_point_run_after_a_plane_to_plane_one(icp_lib, oracle):
    """test_gpu_plane.py's recipe: plane-to-plane 3, the metric set to point-to-point with the switch still on,
    point-to-point 5 on one context == point-to-point 5 on a fresh context loaded with the scene the 3
    plane-to-plane iterations left, bit for bit: the new moments and transform leave the ring, the stored y,
    the seeds and idx as the next loop expects them."""
    amd = icp_lib
    m = oracle.load_matrix(datasets.path("cow_ref"))
    p = oracle.load_matrix(datasets.path("cow_tr2"))
    with amd.Context() as ctx:
        setup_gicp(amd, ctx, m, TS.cow_normals(m.shape[0], 11), p, TS.cow_normals(p.shape[0], 12), 0.0)
        ctx.run(3, -1.0)
        mid = ctx.get_scene()
        assert not np.array_equal(mid, p)
        ctx.set_metric(amd.METRIC_POINT_TO_POINT)  # (epsilon stays set: point-to-point ignores it)
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


def test_switch_arguments_and_refusals(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = G.reference(oracle, ("size", 257))
    ref = run_gicp(amd, m, nrm, p, U0, dmax, 3)
    with amd.Context() as ctx:
        setup_gicp(amd, ctx, m, nrm, p, None, 0.0)
        for bad in (float("nan"), -1.0, 1.5, float("inf")):  # refused, and the earlier setting stays
            with pytest.raises(amd.ICPError) as ei:
                ctx.set_plane_to_plane(bad)
            assert ei.value.code == amd.ICP_E_ARG
        with pytest.raises(amd.ICPError) as ei:  # no scene normals
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL and "icp_set_scene_normals" in str(ei.value)
        ctx.set_scene_normals(U0)
        ctx.set_plane_symmetric(True)
        with pytest.raises(amd.ICPError) as ei:  # both forms at once
            ctx.run(3, -1.0)
        print(str(ei.value))
        assert ei.value.code == amd.ICP_E_ARG
        assert "icp_set_plane_symmetric" in str(ei.value) and "icp_set_plane_to_plane" in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)  # (none of the refused calls ran anything)
        ctx.set_plane_symmetric(False)
        res, errs = ctx.run(3, -1.0)  # ... and the setting of setup_gicp is still the one in force
        np.testing.assert_array_equal(errs, ref["errs"])
        np.testing.assert_array_equal(ctx.get_scene(), ref["scene"])
        ctx.set_plane_to_plane(1.0)  # the upper end is allowed
    with amd.Context() as ctx:  # no model normals: the plane metric's own refusal
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_scene_normals(U0)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_to_plane(G.EPS)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL and "icp_set_model_normals" in str(ei.value)


def test_run_pose_run_on_one_context(icp_lib, oracle):
    """run / transform_scene / run: the second run's Q is the total's rotation, the pose included.  Against a
    fresh context given the moved scene and its current normals (1e-12: a few ulp of Q, pivots > 0.8), and
    against the reference on the same."""
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = G.reference(oracle, ("size", 2049))
    Rz, tz = P.rot((0, 0, 1), 4.0), np.array([0.02, 0.0, -0.01])
    with amd.Context() as ctx:
        setup_gicp(amd, ctx, m, nrm, p, U0, dmax)
        ctx.run(2, -1.0)
        ctx.transform_scene(1.0, Rz, tz)
        mid, umid = ctx.get_scene(), ctx.scene_normals()
        np.testing.assert_allclose(umid, U0 @ ctx.transform()[1].T, rtol=0, atol=1e-15)
        res, errs = ctx.run(3, -1.0)
        scene = ctx.get_scene()
    b = run_gicp(amd, m, nrm, mid, umid, dmax, 3)
    np.testing.assert_allclose(errs, b["errs"], rtol=1e-11)
    np.testing.assert_allclose(scene, b["scene"], rtol=0, atol=1e-12)
    r = G.gicp_ref(oracle, m, nrm, mid, umid, G.EPS, 0.0, 3, -1.0)
    TS.check_against_ref(m, dict(res=res, errs=errs, scene=scene, R=np.array(res.R).reshape(3, 3), t=np.array(res.t)), r)


def test_run_on_a_scene_in_slot_order(icp_lib):
    """test_gpu_symm.py's recipe: two point-to-point iterations at 65,536 points leave the scene in slot order
    (and a total to turn the normals by); three gated plane-to-plane iterations on that context against three
    on a fresh context given get_scene() and scene_normals() (file order)."""
    amd = icp_lib
    n = 65536
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    nrm = r.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    U0 = r.standard_normal((n, 3))
    U0 /= np.linalg.norm(U0, axis=1)[:, None]
    dmax = 0.05
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.set_scene_normals(U0)
        ctx.run(2, -1.0)
        mid, umid = ctx.get_scene(), ctx.scene_normals()
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_to_plane(G.EPS)
        ctx.set_max_distance(dmax)
        res_a, errs_a = ctx.run(3, -1.0)
        ka, (mask_a, cnt_a), scene_a = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene()
    b = run_gicp(amd, m, nrm, mid, umid, dmax, 3)
    print("K", list(ka), list(b["K"]), "err", errs_a, b["errs"])
    assert res_a.iterations == b["res"].iterations == 3
    np.testing.assert_array_equal(ka, b["K"])
    assert cnt_a == b["k"] == ka[-1] and 6 <= cnt_a < n
    np.testing.assert_array_equal(mask_a, b["mask"])
    np.testing.assert_allclose(errs_a, b["errs"], rtol=1e-11)
    np.testing.assert_allclose(scene_a, b["scene"], atol=1e-12)


# 8. ranks: two shards through a host all-reduce on one device against one context over the whole scene
def test_two_ranks_match_single(icp_lib, oracle, tukey_single):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = G.reference(oracle, ("tukey",))
    world = 2
    red = HostAllReduce(world)
    out, errors = [None] * world, []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                setup_gicp(amd, ctx, m, nrm, p[b:b + c], U0[b:b + c], dmax, np_total=p.shape[0],
                           robust=(amd.ROBUST_TUKEY, G.TUKEY_K))
                res, errs = ctx.run(G.GATE_ITERS, -1.0)
                out[r] = TS.collect(ctx, res, errs, True)
                out[r]["Kpos"] = ctx.robust_trace()[1]
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errors, errors
    ref = tukey_single
    print("single", ref["errs"], "ranks", out[0]["errs"])
    for o in out:  # identical decisions and solves on every rank
        np.testing.assert_array_equal(o["errs"], out[0]["errs"])
        np.testing.assert_array_equal(o["K"], out[0]["K"])
        np.testing.assert_array_equal(o["R"], out[0]["R"])
    np.testing.assert_array_equal(out[0]["K"], ref["K"])
    np.testing.assert_array_equal(out[0]["Kpos"], ref["Kpos"])
    np.testing.assert_allclose(out[0]["errs"], ref["errs"], rtol=1e-11)
    np.testing.assert_array_equal(np.concatenate([o["mask"] for o in out]), ref["mask"])
    np.testing.assert_allclose(np.concatenate([o["scene"] for o in out]), ref["scene"], atol=1e-12)


# 9. estimated normals, the reference-shaped class, the CLI and the pyramid
def test_estimated_normals_on_both_clouds(icp_lib, oracle):
    amd = icp_lib
    m, _nrm, p, _U0, _dmax, _r = G.reference(oracle, ("size", 2049))
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.estimate_model_normals(16)
        ctx.set_scene(p)
        ctx.estimate_scene_normals(16)
        en, eu = ctx.model_normals(), ctx.scene_normals()
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_to_plane(G.EPS)
        res, errs = ctx.run(3, -1.0)
        scene = ctx.get_scene()
    given = run_gicp(amd, m, en, p, eu, 0.0, 3)  # the same normals through the setters
    np.testing.assert_array_equal(errs, given["errs"])
    np.testing.assert_array_equal(scene, given["scene"])
    TS.check_against_ref(m, given, G.gicp_ref(oracle, m, en, p, eu, G.EPS, 0.0, 3, -1.0))


def test_reference_shaped_class_takes_plane_to_plane(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = G.reference(oracle, ("size", 257))
    ref = run_gicp(amd, m, nrm, p, U0, dmax, 3, eps=0.01)
    icp = amd.ICP(m, p, 3, threshold=-1.0, normals=nrm, scene_normals=U0, plane_to_plane=0.01)
    res = icp.find_corresponding_opti()
    assert res.iterations == 3 and icp.s == 1.0
    np.testing.assert_array_equal(icp.errors, ref["errs"])
    np.testing.assert_array_equal(icp.new_p, ref["scene"])
    assert not np.array_equal(ref["errs"], run_gicp(amd, m, nrm, p, U0, dmax, 3)["errs"])  # (epsilon is read)


def test_cli_gicp(icp_lib, tmp_path):
    amd = icp_lib
    m, nrm, p, _src = P.synth(257, 357, 0.01)
    U0 = S.scene_normals_of(nrm)
    paths = {k: str(tmp_path / (k + ".txt")) for k in ("model", "scene", "normals", "snormals")}
    for k, v in zip(("model", "scene", "normals", "snormals"), (m, p, nrm, U0)):
        amd.write_matrix(paths[k], v)
    both = ["--normals", paths["normals"], "--scene-normals", paths["snormals"]]
    base = [paths["model"], paths["scene"], "4", "--threshold", "-1"]
    outs = {}
    for eps, extra in ((G.EPS, []), (0.01, ["--gicp-epsilon", "0.01"])):
        r = TS.cli(tmp_path, *base, "--gicp", *extra, *both)
        assert r.returncode == 0, r.stderr[-2000:]
        with amd.Context() as ctx:  # the rounded clouds: the input of both sides
            setup_gicp(amd, ctx, amd.load_matrix(paths["model"]), amd.load_matrix(paths["normals"]),
                       amd.load_matrix(paths["scene"]), amd.load_matrix(paths["snormals"]), 0.0, eps=eps)
            res, _errs = ctx.run(4, -1.0)
            g = str(tmp_path / "g.txt")
            amd.write_matrix(g, ctx.get_scene())
        assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations == 4
        outs[eps] = open(tmp_path / "output.txt", "rb").read()
        assert outs[eps] == open(g, "rb").read()
    assert outs[G.EPS] != outs[0.01]
    for bad in (["--gicp", "--symmetric", *both],  # one form at a time
                ["--gicp"],  # no normals at all
                ["--gicp", "--normals", paths["normals"]],  # none of the scene's
                ["--gicp", "--scene-normals", paths["snormals"]],  # none of the model's
                ["--gicp-epsilon", "0.01", *both],  # without --gicp
                ["--gicp", "--gicp-epsilon", "0", *both],
                ["--gicp", "--gicp-epsilon", "1.5", *both],
                ["--gicp", "--gicp-epsilon", "x", *both]):
        r = TS.cli(tmp_path, *base, *bad)
        assert r.returncode != 0 and "[error]" in r.stderr, bad
        assert "[load]" not in r.stderr, bad  # (refused before any file is touched)


def test_cli_and_register_pyramid_with_plane_to_plane(icp_lib, tmp_path):
    amd = icp_lib
    m, _nrm, p, _src = P.synth(4097, 4197, 0.0, other=True)
    mp, pp = str(tmp_path / "model.txt"), str(tmp_path / "scene.txt")
    amd.write_matrix(mp, m)
    amd.write_matrix(pp, p)
    r = TS.cli(tmp_path, mp, pp, "4", "--allow-unequal", "--gicp", "--estimate-normals", "16", "--estimate-scene-normals",
               "16", "--pyramid", "0.3", "--threshold", "-1")
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:
        ctx.set_allow_unequal(True)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_to_plane(G.EPS)
        res, _pose, records = amd.register_pyramid(ctx, amd.load_matrix(mp), amd.load_matrix(pp), [0.3], 4, threshold=-1.0,
                                                   estimate_normals=16, estimate_scene_normals=16)
        g = str(tmp_path / "g.txt")
        amd.write_matrix(g, ctx.get_scene())
    print([(rec["voxel"], rec["model_points"], rec["scene_points"], rec["err"]) for rec in records])
    assert res.iterations == 4 and len(records) == 2
    assert open(tmp_path / "output.txt", "rb").read() == open(g, "rb").read()
