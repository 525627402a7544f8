"""icp_run with the symmetric point-to-plane iteration (icp_set_plane_symmetric, the symm_* kernels
of icp_plane.hip) and the scene's normals (icp_set_scene_normals*, icp_estimate_scene_normals)
against tests/symm_ref.py, the loop restated with the oracle's search and numpy.

Tolerances are test_gpu_plane.py's: K per iteration and the masks exact
(tests/test_symm_ref.py checks on the CPU that no pair of these inputs lies within 1e-6 of the gate),
err rel 1e-9 or within (1e-9 x extent)^2 absolutely -- the position tolerance squared: the floor on the
difference that an err fallen to rounding needs (n = 6, tests/test_symm_ref.py's err_close) --, R abs
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
import symm_ref as S
from test_gpu_gated import HostAllReduce

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


def setup_symm(amd, ctx, m, nrm, p, U0, dmax, np_total=None, trim=None, robust=None):
    ctx.set_model(m)
    ctx.set_model_normals(nrm)
    ctx.set_scene(p, np_total=np_total)
    if U0 is not None:
        ctx.set_scene_normals(U0)
    ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
    ctx.set_plane_symmetric(True)
    if dmax:
        ctx.set_max_distance(dmax)
    if trim is not None:
        ctx.set_trim(trim)
    if robust is not None:
        ctx.set_robust(*robust)


def collect(ctx, res, errs, gated):
    out = dict(res=res, errs=errs, scene=ctx.get_scene(), R=np.array(res.R).reshape(3, 3), t=np.array(res.t))
    if gated:
        mask, k = ctx.inliers()
        out.update(K=ctx.inlier_trace(), mask=mask, k=k)
    return out


def run_symm(amd, m, nrm, p, U0, dmax, iters, threshold=-1.0, mode=0, variant=None, trim=None, robust=None, **ctx_args):
    """-> dict(res, errs, scene, R, t, and with a gate or a trim K (trace), mask, k) of a fresh context."""
    with amd.Context(0, mode, **ctx_args) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        setup_symm(amd, ctx, m, nrm, p, U0, dmax, trim=trim, robust=robust)
        res, errs = ctx.run(iters, threshold)
        return collect(ctx, res, errs, bool(dmax) or trim is not None)


def assert_err(errs, ref, extent, rtol=1e-9):
    floor = (1e-9 * extent) ** 2
    errs, ref = np.asarray(errs, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = np.maximum(floor, rtol * np.abs(ref))
    assert np.all(np.abs(errs - ref) <= tol), (errs, ref)


def check_against_ref(m, out, r):
    print("err", out["errs"], "ref err", r["err"], "K", list(out.get("K", [])))
    extent = float(np.abs(m).max())
    assert out["res"].iterations == r["iterations"]
    assert out["res"].s == 1.0
    assert_err(out["errs"], r["err"], extent)
    np.testing.assert_allclose(out["R"], r["R"], atol=1e-9)
    np.testing.assert_allclose(out["R"] @ out["R"].T, np.eye(3), atol=1e-14)
    np.testing.assert_allclose(out["t"], r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(out["scene"], r["new_p"], atol=1e-9 * extent)
    if "K" in out:
        assert list(out["K"]) == r["K"] and out["k"] == r["K"][-1]
        np.testing.assert_array_equal(out["mask"], r["mask"])
        assert out["mask"].sum() == out["k"]


def bitwise(a, b):
    for key in ("errs", "scene", "R", "t") + (("K", "mask") if "K" in a else ()):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# 1. sizes: the wave tail, one workgroup, the first multi-workgroup fold, an odd multi-block size;
# n = 6 sits on the minimum K
@pytest.mark.parametrize("n", S.SIZES)
def test_sizes(icp_lib, oracle, n):
    """n = 6: six pairs determine the six unknowns, err falls to rounding (6.6e-8, 1.5e-14, 6.6e-21, ...) and
    the floor takes over: at err = 1.5e-14 the engine is 1.6e-23 from the reference (1.07e-9 of it: one ulp
    of a coordinate against residuals of 1e-7), as the reference is 2.0e-23 from its extended-precision twin."""
    m, nrm, p, U0, dmax, r = S.reference(oracle, ("size", n))
    out = run_symm(icp_lib, m, nrm, p, U0, dmax, S.SIZES_ITERS)
    check_against_ref(m, out, r)


# 2. the kernels do not depend on which search ran, and a run is deterministic
def test_variants_bitwise_at_4097(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("size", 4097))
    a = run_symm(amd, m, nrm, p, U0, dmax, S.SIZES_ITERS)
    bitwise(run_symm(amd, m, nrm, p, U0, dmax, S.SIZES_ITERS), a)
    for mode, variant in ((amd.NN_FP64, None), (amd.NN_CERTIFIED, amd.VARIANT_GRID)):
        bitwise(run_symm(amd, m, nrm, p, U0, dmax, S.SIZES_ITERS, mode=mode, variant=variant), a)


# 3. with the gate; with the trim and with robust weights on top
@pytest.fixture(scope="module")
def gate_single(icp_lib, oracle):
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("gate", 4097, 0.08))
    return run_symm(icp_lib, m, nrm, p, U0, dmax, S.GATES_ITERS)


@pytest.mark.parametrize("n,dmax", list(S.GATES))
def test_gate(icp_lib, oracle, gate_single, n, dmax):
    m, nrm, p, U0, d, r = S.reference(oracle, ("gate", n, dmax))
    out = gate_single if n == 4097 else run_symm(icp_lib, m, nrm, p, U0, d, S.GATES_ITERS)
    check_against_ref(m, out, r)
    assert list(out["K"]) == S.GATES[(n, dmax)]


def test_gate_with_a_trim(icp_lib, oracle):
    m, nrm, p, U0, d, r = S.reference(oracle, ("trim", 4097, 0.08))
    out = run_symm(icp_lib, m, nrm, p, U0, d, S.GATES_ITERS, trim=S.TRIM)
    check_against_ref(m, out, r)


def test_gate_with_tukey_weights(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, d, r = S.reference(oracle, ("tukey", 4097, 0.08))
    with amd.Context() as ctx:
        setup_symm(amd, ctx, m, nrm, p, U0, d, robust=(amd.ROBUST_TUKEY, S.TUKEY_K))
        res, errs = ctx.run(S.GATES_ITERS, -1.0)
        out = collect(ctx, res, errs, True)
        W, Kpos = ctx.robust_trace()
    check_against_ref(m, out, r)
    assert list(Kpos) == r["Kpos"]
    np.testing.assert_allclose(W, r["W"], rtol=1e-9)


# 4. the purpose: a different sample of the same curved surface, from 15 degrees
def test_symmetric_lands_where_point_to_plane_keeps_a_bias(icp_lib):
    amd = icp_lib
    m, nrm, p, U0, src = S.purpose()
    out = run_symm(amd, m, nrm, p, U0, 0.0, 5)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.run(8, -1.0)
        plane = ctx.get_scene()
    dsymm, dplane = float(np.abs(out["scene"] - src).max()), float(np.abs(plane - src).max())
    print("max |new_p - src|: symmetric, 5 iterations", dsymm, "point-to-plane, 8 iterations", dplane)
    assert dsymm < 2e-5
    assert dplane > 1e-4


# 5. signs and zeros
def test_the_sign_of_a_normal_changes_no_bit(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("size", 4097))
    a = run_symm(amd, m, nrm, p, U0, dmax, S.SIZES_ITERS)
    flip = np.where(np.random.default_rng(2).random(4097) < 0.5, -1.0, 1.0)[:, None]
    bitwise(run_symm(amd, m, nrm, p, U0 * flip, dmax, S.SIZES_ITERS), a)
    bitwise(run_symm(amd, m, nrm * flip, p, U0, dmax, S.SIZES_ITERS), a)


def test_zero_normals_drop_their_pairs(icp_lib, oracle):
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("size", 257))
    idx = oracle.closest(p, m)[1]
    N0, U00 = nrm.copy(), U0.copy()
    N0[idx[7]] = 0.0  # the first iteration's pair of scene point 7 (and of whichever others share that model point)
    assert idx[11] != idx[7]
    U00[11] = 0.0
    r = S.symm_ref(oracle, m, N0, p, U00, 0.0, S.SIZES_ITERS, -1.0)
    out = run_symm(icp_lib, m, N0, p, U00, 0.0, S.SIZES_ITERS)
    check_against_ref(m, out, r)
    assert not np.array_equal(out["errs"], run_symm(icp_lib, m, nrm, p, U0, 0.0, S.SIZES_ITERS)["errs"])


# 6. too few, degenerate: the run stops before the iteration changes anything
@pytest.mark.parametrize("case", ["few", "degenerate"])
def test_stops_before_the_iteration(icp_lib, case):
    amd = icp_lib
    m, nrm, p, U0 = S.five() if case == "few" else S.planar()
    with amd.Context() as ctx:
        setup_symm(amd, ctx, m, nrm, p, U0, 0.0)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(5, -1.0)
        print(str(ei.value))
        assert ei.value.code == (amd.ICP_E_TOO_FEW_POINTS if case == "few" else amd.ICP_E_DEGENERATE)
        assert "iteration 0" in str(ei.value)
        assert ("K = 5" if case == "few" else "pivot") in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)
        np.testing.assert_array_equal(ctx.scene_normals(), U0)  # (a frozen iteration does not move them)


# 7. the normals' life
def test_scene_normals_hygiene(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("size", 257))
    ref = run_symm(amd, m, nrm, p, U0, dmax, 3)
    with amd.Context() as ctx:
        with pytest.raises(amd.ICPError) as ei:  # no scene yet
            ctx.set_scene_normals(U0)
        assert ei.value.code == amd.ICP_E_NO_MODEL
        setup_symm(amd, ctx, m, nrm, p, None, 0.0)
        with pytest.raises(amd.ICPError) as ei:  # no scene normals
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL and "icp_set_scene_normals" in str(ei.value)
        with pytest.raises(amd.ICPError) as ei:
            ctx.scene_normals()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        with pytest.raises(amd.ICPError) as ei:
            ctx.set_scene_normals(U0[:-1])
        assert ei.value.code == amd.ICP_E_SIZE_MISMATCH
        bad = U0.copy()
        bad[100, 1] = np.nan
        with pytest.raises(amd.ICPError) as ei:
            ctx.set_scene_normals(bad)
        assert ei.value.code == amd.ICP_E_ARG
        np.testing.assert_array_equal(ctx.get_scene(), p)  # (none of the refused calls ran anything)
        ctx.set_scene(p)
        ctx.set_scene_normals(U0)
        np.testing.assert_array_equal(ctx.scene_normals(), U0)
        res, errs = ctx.run(3, -1.0)
        np.testing.assert_array_equal(errs, ref["errs"])
        np.testing.assert_array_equal(ctx.get_scene(), ref["scene"])
        _s, Rt, _t = ctx.transform()  # after a run the normals have turned with the scene
        np.testing.assert_allclose(ctx.scene_normals(), U0 @ Rt.T, rtol=0, atol=1e-15)
        assert np.abs(ctx.scene_normals() - U0).max() > 1e-3
        Rz = P.rot((0, 0, 1), 10.0)
        ctx.transform_scene(1.0, Rz, np.array([0.1, 0.0, 0.0]))  # ... and with a pose
        _s, Rt2, _t = ctx.transform()
        np.testing.assert_allclose(Rt2, Rz @ Rt, atol=1e-15)
        np.testing.assert_allclose(ctx.scene_normals(), U0 @ Rt2.T, rtol=0, atol=1e-15)
        ctx.set_scene(p)  # a scene upload drops them
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_NO_MODEL and "icp_set_scene_normals" in str(ei.value)
        du = torch.from_numpy(U0).to("cuda:0")  # the device setter: the host setter's run bit for bit
        torch.cuda.synchronize()
        ctx.set_scene_normals_device(du.data_ptr(), U0.shape[0])
        res, errs = ctx.run(3, -1.0)
        np.testing.assert_array_equal(errs, ref["errs"])
        np.testing.assert_array_equal(ctx.get_scene(), ref["scene"])
        np.testing.assert_array_equal(np.array(res.R).reshape(3, 3), ref["R"])


def test_a_second_run_continues_with_the_turned_normals(icp_lib, oracle):
    """3 + 3 iterations in two runs against 6 in one: the second run starts from the total's rotation.
    Not bit for bit: one run composes its steps in order, Q = R5 (R4 (R3 R2 R1)), the second of two runs
    composes its own first and then onto the first run's total, Q = (R5 R4) (R3 R2 R1) -- the same
    rotation to a few ulp.  The system's pivots are > 0.9 here (tests/test_symm_ref.py), so the
    trajectories stay within 1e-13: a thousand ulp of room over the few that the reasoning gives."""
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("size", 4097))
    one = run_symm(amd, m, nrm, p, U0, dmax, 6)
    with amd.Context() as ctx:
        setup_symm(amd, ctx, m, nrm, p, U0, dmax)
        _res, e1 = ctx.run(3, -1.0)
        res, e2 = ctx.run(3, -1.0)
        np.testing.assert_array_equal(e1, one["errs"][:3])
        np.testing.assert_allclose(e2, one["errs"][3:], rtol=1e-13)
        np.testing.assert_allclose(ctx.get_scene(), one["scene"], rtol=0, atol=1e-13)
        np.testing.assert_allclose(ctx.scene_normals(), U0 @ ctx.transform()[1].T, rtol=0, atol=1e-15)


def test_reference_shaped_class_takes_scene_normals(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("size", 257))
    ref = run_symm(amd, m, nrm, p, U0, dmax, 3)
    icp = amd.ICP(m, p, 3, threshold=-1.0, normals=nrm, scene_normals=U0)
    res = icp.find_corresponding_opti()
    assert res.iterations == 3 and icp.s == 1.0
    np.testing.assert_array_equal(icp.errors, ref["errs"])
    np.testing.assert_array_equal(icp.new_p, ref["scene"])


# 8. off is off
def cow_normals(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_off_is_off(icp_lib, oracle):
    amd = icp_lib
    cow = (oracle.load_matrix(datasets.path("cow_ref")), oracle.load_matrix(datasets.path("cow_tr1")))
    m, nrm, p, U0, _d, _r = S.reference(oracle, ("size", 4097))
    for mm, pp, N, U in ((cow[0], cow[1], cow_normals(cow[0].shape[0], 11), cow_normals(cow[1].shape[0], 12)),
                         (m, p, nrm, U0)):
        for metric in (amd.METRIC_POINT_TO_PLANE, amd.METRIC_POINT_TO_POINT):
            runs = []
            for form in ("never", "resident", "switched_on_for_the_other_metric"):
                with amd.Context() as ctx:
                    ctx.set_model(mm)
                    ctx.set_model_normals(N)
                    ctx.set_scene(pp)
                    ctx.set_metric(metric)
                    if form != "never":
                        ctx.set_scene_normals(U)
                    if form == "switched_on_for_the_other_metric":
                        if metric == amd.METRIC_POINT_TO_PLANE:
                            continue
                        ctx.set_plane_symmetric(True)  # (a switch on the plane metric: point-to-point ignores it)
                    res, errs = ctx.run(4, -1.0)
                    runs.append((errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t)))
            for other in runs[1:]:
                for a, b in zip(runs[0], other):
                    np.testing.assert_array_equal(a, b)
    with amd.Context() as ctx:
        for bad in (2, -1):
            with pytest.raises(amd.ICPError) as ei:
                ctx.set_plane_symmetric(bad)
            assert ei.value.code == amd.ICP_E_ARG


# 9. a scene in slot order, correspondences with kd positions
def test_symmetric_run_on_a_scene_in_slot_order(icp_lib):
    """test_gpu_plane.py's recipe: two point-to-point iterations at 65,536 points leave the scene in
    slot order (and a total to turn the normals by); three gated symmetric iterations on that context
    against three on a fresh context given get_scene() and scene_normals() (file order)."""
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
        ctx.set_plane_symmetric(True)
        ctx.set_max_distance(dmax)
        res_a, errs_a = ctx.run(3, -1.0)
        ka, (mask_a, cnt_a), scene_a = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene()
    b = run_symm(amd, m, nrm, mid, umid, dmax, 3)
    print("K", list(ka), list(b["K"]), "err", errs_a, b["errs"])
    assert res_a.iterations == b["res"].iterations == 3
    np.testing.assert_array_equal(ka, b["K"])
    assert cnt_a == b["k"] == ka[-1] and 6 <= cnt_a < n
    np.testing.assert_array_equal(mask_a, b["mask"])
    assert mask_a.sum() == cnt_a
    np.testing.assert_allclose(errs_a, b["errs"], rtol=1e-11)
    np.testing.assert_allclose(scene_a, b["scene"], atol=1e-12)


# 10. ranks
def run_symm_sharded(amd, m, nrm, p, U0, dmax, world, iters):
    red = HostAllReduce(world)
    results = [None] * world
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                setup_symm(amd, ctx, m, nrm, p[b:b + c], U0[b:b + c], dmax, np_total=p.shape[0])
                res, errs = ctx.run(iters, -1.0)
                results[r] = collect(ctx, res, errs, True)
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
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("gate", 4097, 0.08))
    ref = gate_single
    out = run_symm_sharded(icp_lib, m, nrm, p, U0, dmax, world, S.GATES_ITERS)
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
    amd = icp_lib
    m, nrm, p, U0, dmax, _r = S.reference(oracle, ("gate", 4097, 0.08))
    out = run_symm(amd, m, nrm, p, U0, dmax, S.GATES_ITERS, rank=0, world_size=1, rccl_id=amd.rccl_unique_id())
    bitwise(out, gate_single)
    assert out["k"] == gate_single["k"]


# 11. the scene's normals estimated on the device
def duplicated_cloud(n=257):
    p = P.synth(n, 100 + n, 0.01)[2].copy()
    p[40:60] = p[10:30]  # twenty points twice
    p[200] = p[201] = p[202]
    return p


@pytest.mark.parametrize("case", ["257", "4097", "duplicates"])
def test_estimate_is_the_model_estimators(icp_lib, case):
    amd = icp_lib
    p = duplicated_cloud() if case == "duplicates" else P.synth(int(case), 100 + int(case), 0.01)[2]
    m = P.synth(63, 163, 0.01)[0]  # (the model of the first context plays no part)
    view = np.array([0.3, -2.0, 5.0])
    for vp in (None, view):
        with amd.Context() as a, amd.Context() as b:
            a.set_model(m)
            a.set_allow_unequal(True)
            a.set_scene(p)
            da = a.estimate_scene_normals(16, vp)
            b.set_model(p)
            db = b.estimate_model_normals(16, vp)
            na, nb = a.scene_normals(), b.model_normals()
            print(case, "undetermined", da, db)
            assert da == db
            np.testing.assert_array_equal(na.view(np.uint64), nb.view(np.uint64))
            np.testing.assert_array_equal(a.get_scene(), p)
    assert np.abs(np.linalg.norm(na, axis=1) - 1.0).max() < 1e-12 or da > 0


def test_estimate_conditions_and_the_run_after_it(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, _U0, dmax, _r = S.reference(oracle, ("size", 4097))
    with amd.Context() as ctx:
        with pytest.raises(amd.ICPError) as ei:
            ctx.estimate_scene_normals(16)
        assert ei.value.code == amd.ICP_E_NO_MODEL
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_scene(p)
        for k in (2, 65, 5000):
            with pytest.raises(amd.ICPError) as ei:
                ctx.estimate_scene_normals(k)
            assert ei.value.code == amd.ICP_E_ARG and str(k) in str(ei.value)
        with pytest.raises(amd.ICPError) as ei:
            ctx.estimate_scene_normals(16, [np.inf, 0, 0])
        assert ei.value.code == amd.ICP_E_ARG
        ctx.estimate_scene_normals(16)
        est = ctx.scene_normals()
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_symmetric(True)
        res, errs = ctx.run(4, -1.0)
        scene = ctx.get_scene()
        with pytest.raises(amd.ICPError) as ei:  # refused after a run ...
            ctx.estimate_scene_normals(16)
        assert ei.value.code == amd.ICP_E_ARG and "icp_run" in str(ei.value)
        ctx.set_scene(p)
        ctx.transform_scene(1.0, np.eye(3), np.zeros(3))
        with pytest.raises(amd.ICPError) as ei:  # ... and after a pose
            ctx.estimate_scene_normals(16)
        assert ei.value.code == amd.ICP_E_ARG
    given = run_symm(amd, m, nrm, p, est, dmax, 4)  # the same normals through the setter
    np.testing.assert_array_equal(errs, given["errs"])
    np.testing.assert_array_equal(scene, given["scene"])
    with amd.Context(0, 0, rank=0, world_size=2, host_allreduce=HostAllReduce(2).for_rank(0)) as ctx:  # a shard
        ctx.set_model(m)
        ctx.set_scene(p[:2049], np_total=4097)
        with pytest.raises(amd.ICPError) as ei:
            ctx.estimate_scene_normals(16)
        assert ei.value.code == amd.ICP_E_ARG and "shard" in str(ei.value)


# 12. CLI and pyramid
def cli(tmp_path, *args):
    return subprocess.run([os.path.join(BUILD, "icp-gpu"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_cli_symmetric(icp_lib, tmp_path):
    amd = icp_lib
    m, nrm, p, _src = P.synth(257, 357, 0.01)
    U0 = S.scene_normals_of(nrm)
    paths = {k: str(tmp_path / (k + ".txt")) for k in ("model", "scene", "normals", "snormals", "short")}
    amd.write_matrix(paths["model"], m)
    amd.write_matrix(paths["scene"], p)
    amd.write_matrix(paths["normals"], nrm)
    amd.write_matrix(paths["snormals"], U0)
    amd.write_matrix(paths["short"], U0[:-1])
    wsn = str(tmp_path / "wsn.txt")
    r = cli(tmp_path, paths["model"], paths["scene"], "20", "--symmetric", "--normals", paths["normals"], "--scene-normals",
            paths["snormals"], "--write-scene-normals", wsn)
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:  # the rounded clouds: the input of both sides
        setup_symm(amd, ctx, amd.load_matrix(paths["model"]), amd.load_matrix(paths["normals"]),
                   amd.load_matrix(paths["scene"]), amd.load_matrix(paths["snormals"]), 0.0)
        res, _errs = ctx.run(20, 1e-5)
        g, gn = str(tmp_path / "g.txt"), str(tmp_path / "gn.txt")
        amd.write_matrix(g, ctx.get_scene())
        amd.write_matrix(gn, ctx.scene_normals())
    assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
    assert open(tmp_path / "output.txt", "rb").read() == open(g, "rb").read()
    assert open(wsn, "rb").read() == open(gn, "rb").read()
    base = [paths["model"], paths["scene"], "20"]
    for bad in (["--symmetric"],  # no normals at all
                ["--symmetric", "--normals", paths["normals"]],  # none of the scene's
                ["--symmetric", "--scene-normals", paths["snormals"]],  # none of the model's
                ["--symmetric", "--normals", paths["normals"], "--scene-normals", paths["snormals"],
                 "--estimate-scene-normals", "16"],  # two sources
                ["--symmetric", "--estimate-normals", "16", "--scene-normals", paths["snormals"], "--pyramid", "0.3"],
                ["--write-scene-normals", wsn],
                ["--symmetric", "--normals", paths["normals"], "--estimate-scene-normals", "2"],
                ["--symmetric", "--normals", paths["normals"], "--scene-normals", str(tmp_path / "missing.txt"),
                 "--estimate-scene-normals", "x"]):
        r = cli(tmp_path, *base, *bad)
        assert r.returncode != 0 and "[error]" in r.stderr, bad
        assert "[load]" not in r.stderr, bad  # (refused before any file is touched)
    r = cli(tmp_path, *base, "--symmetric", "--normals", paths["normals"], "--scene-normals", paths["short"])
    assert r.returncode != 0 and "[error]" in r.stderr


def test_cli_symmetric_pyramid(icp_lib, tmp_path):
    amd = icp_lib
    m, _nrm, p, _src = P.synth(4097, 4197, 0.0, other=True)
    mp, pp = str(tmp_path / "model.txt"), str(tmp_path / "scene.txt")
    amd.write_matrix(mp, m)
    amd.write_matrix(pp, p)
    r = cli(tmp_path, mp, pp, "6", "--allow-unequal", "--symmetric", "--estimate-normals", "16", "--estimate-scene-normals",
            "16", "--pyramid", "0.3", "--threshold", "-1")
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:
        ctx.set_allow_unequal(True)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_symmetric(True)
        res, _pose, records = amd.register_pyramid(ctx, amd.load_matrix(mp), amd.load_matrix(pp), [0.3], 6, threshold=-1.0,
                                                   estimate_normals=16, estimate_scene_normals=16)
        g = str(tmp_path / "g.txt")
        amd.write_matrix(g, ctx.get_scene())
        with pytest.raises(ValueError):
            amd.register_pyramid(ctx, m, p, [5.0], 6, estimate_normals=3, estimate_scene_normals=16)
    print([(rec["voxel"], rec["model_points"], rec["scene_points"], rec["err"]) for rec in records])
    assert res.iterations == 6 and len(records) == 2
    assert open(tmp_path / "output.txt", "rb").read() == open(g, "rb").read()
