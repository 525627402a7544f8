"""icp_run with one-to-one correspondences (icp_set_one_to_one, icp_unique.hip) against
tests/unique_ref.py, the loop restated with the oracle's pieces.

Tolerances are the gate tests' (test_gpu_gated.py check_against_ref): K per iteration and the masks
exact, err rel 1e-9, s and R abs 1e-9, t and new_p abs 1e-9 x extent.  The first iteration's d2 has
the oracle's bits, so its mask needs no margin; later iterations rest on the reference's margin
(tests/test_unique_ref.py: > 1e-6 for every case used here).
"""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import gated_ref as G
import gicp_ref as GI
import plane_ref as P
import robust_ref as RR
import symm_ref as S
import unique_ref as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_unique(amd, m, p, iters, dmax=0.0, f=None, mode=0, variant=None, prepare=None, on=True, unequal=False):
    """-> (res, errs, scene, K trace, mask, K last) of a fresh context."""
    with amd.Context(0, mode) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        if unequal:
            ctx.set_allow_unequal(True)
        ctx.set_model(m)
        ctx.set_scene(p)
        if prepare is not None:
            prepare(ctx)
        if on:
            ctx.set_one_to_one(True)
        if f is not None:
            ctx.set_trim(f)
        if dmax:
            ctx.set_max_distance(dmax)
        res, errs = ctx.run(iters, -1.0)
        mask, k = ctx.inliers()
        return res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, k


def check_against_ref(m, out, r):
    res, errs, scene, ktrace, mask, k = out
    print("K", list(ktrace), "ref K", r["K"], "err", errs, "ref err", r["err"])
    assert res.iterations == r["iterations"]
    assert list(ktrace) == r["K"] and k == r["K"][-1]
    np.testing.assert_array_equal(mask, r["mask"])
    assert mask.sum() == k
    np.testing.assert_allclose(errs, r["err"], rtol=1e-9)
    assert abs(res.s - r["s"]) <= 1e-9
    np.testing.assert_allclose(np.array(res.R).reshape(3, 3), r["R"], atol=1e-9)
    extent = float(np.abs(m).max())
    np.testing.assert_allclose(np.array(res.t), r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(scene, r["new_p"], atol=1e-9 * extent)


def key_id(key):
    return "-".join(str(k) for k in key)


# 1. one iteration, exact: the first iteration's d2 has the oracle's bits, so no margin is needed.
# The sizes: np 63 / 64 / 65 the ballot's wave edge, 4096 / 4097 the workgroups' edge, 9001 several.
@pytest.mark.parametrize("key", U.MULTI, ids=key_id)
def test_one_iteration_exact(icp_lib, oracle, key):
    m, p, dmax, f, _it, r = U.reference(oracle, key, iters=1)
    check_against_ref(m, run_unique(icp_lib, m, p, 1, dmax, f), r)


# 2. several iterations: plain, and with the gate, the trim and both
@pytest.mark.parametrize("key", U.MULTI, ids=key_id)
def test_several_iterations(icp_lib, oracle, key):
    m, p, dmax, f, iters, r = U.reference(oracle, key)
    assert r["margin"] > 1e-6
    check_against_ref(m, run_unique(icp_lib, m, p, iters, dmax, f), r)


def test_partial_overlap_is_registered(icp_lib, oracle):
    """The purpose: cow_partial ends below 1e-9 with one-to-one and above 0.05 without it."""
    m, p, _d, _f, iters, _r = U.reference(oracle, ("partial",))
    with icp_lib.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        _res, plain = ctx.run(iters, -1.0)
    out = run_unique(icp_lib, m, p, iters)
    print("plain", plain[-1], "one-to-one", out[1][-1])
    assert plain[-1] > 0.05 and out[1][-1] < 1e-9


# 3. ties are kept whole: both copies of every winner, K twice the single-copy run's
def test_ties_are_kept_whole(icp_lib, oracle):
    m, p = G.synth(257, 357, 0.25)
    p2 = np.repeat(p, 2, axis=0)
    one = run_unique(icp_lib, m, p, 1)
    r = U.one_to_one_ref(oracle, m, p2, 1, -1.0)
    out = run_unique(icp_lib, m, p2, 1, unequal=True)
    check_against_ref(m, out, r)
    np.testing.assert_array_equal(out[4][0::2], one[4])
    np.testing.assert_array_equal(out[4][1::2], one[4])
    assert out[5] == 2 * one[5] == 356


# 4. one address: 4,090 of 4,097 points scatter onto one model point (the contended path)
def test_one_address(icp_lib, oracle):
    m, p = U.one_address()
    r = U.one_to_one_ref(oracle, m, p, 1, -1.0)
    assert np.bincount(r["idx"], minlength=8).tolist() == [4090] + [1] * 7 and r["K"] == [8]
    check_against_ref(m, run_unique(icp_lib, m, p, 1, unequal=True), r)
    r2 = U.one_to_one_ref(oracle, m, p, 2, -1.0)
    check_against_ref(m, run_unique(icp_lib, m, p, 2, unequal=True), r2)


# 5. shapes: a model smaller and larger than the scene (the table is the model's size)
@pytest.mark.parametrize("nm", [5, 4097])
def test_unequal_model(icp_lib, oracle, nm):
    m, _p = G.synth(nm, 100 + nm, 0.0)
    p = G.synth(257, 357, 0.25)[1]
    r = U.one_to_one_ref(oracle, m, p, 3, -1.0)
    print(nm, r["K"], r["margin"])
    assert r["status"] == "ok" and r["margin"] > 1e-6
    check_against_ref(m, run_unique(icp_lib, m, p, 3, unequal=True), r)


# 6. each metric, one iteration: the metric's own reference on the kept pairs alone (the scene's
# winners against the whole model finds the same correspondences and keeps them all), with the
# tolerances of that metric's tests; the dropped points move by the same step
def metric_case(oracle, n):
    m, nrm, p = P.gate_case(n)
    r = U.one_to_one_ref(oracle, m, p, 1, -1.0)
    assert 6 <= r["K"][0] < n
    return m, nrm, p, S.scene_normals_of(nrm), r["mask"]


def check_metric(m, p, keep, out, r):
    res, errs, scene, ktrace, mask, k = out
    print("K", list(ktrace), "err", errs, "ref err", r["err"])
    extent = float(np.abs(m).max())
    assert res.iterations == r["iterations"] == 1 and res.s == 1.0
    assert list(ktrace) == r["K"] == [int(keep.sum())] and k == r["K"][0]
    np.testing.assert_array_equal(mask, keep)
    floor = (1e-9 * extent) ** 2
    assert abs(errs[0] - r["err"][0]) <= max(floor, 1e-9 * abs(r["err"][0]))
    R, t = np.array(res.R).reshape(3, 3), np.array(res.t)
    np.testing.assert_allclose(R, r["R"], atol=1e-9)
    np.testing.assert_allclose(t, r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(scene[keep], r["new_p"], atol=1e-9 * extent)
    np.testing.assert_allclose(scene[~keep], p[~keep] @ np.asarray(r["R"]).T + r["t"], atol=1e-9 * extent)


def test_point_to_plane(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, _U0, keep = metric_case(oracle, 4097)

    def prepare(ctx):
        ctx.set_model_normals(nrm)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)

    check_metric(m, p, keep, run_unique(amd, m, p, 1, prepare=prepare), P.plane_ref(oracle, m, nrm, p[keep], 0.0, 1, -1.0))


def test_point_to_plane_with_tukey_weights(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, _U0, keep = metric_case(oracle, 4097)
    k = RR.k_of("plane", RR.TUKEY, 4097)
    r = RR.robust_ref(oracle, "plane", m, nrm, p[keep], 0.0, RR.TUKEY, k, 1, -1.0)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_model_normals(nrm)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_scene(p)
        ctx.set_robust(amd.ROBUST_TUKEY, k)
        ctx.set_one_to_one(True)
        res, errs = ctx.run(1, -1.0)
        mask, kk = ctx.inliers()
        out = (res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, kk)
        W, Kpos = ctx.robust_trace()
    print("W", list(W), r["W"], "K+", list(Kpos), r["Kpos"])
    check_metric(m, p, keep, out, r)
    np.testing.assert_allclose(W, np.array(r["W"], dtype=np.float64), rtol=1e-9)
    assert list(Kpos) == r["Kpos"] and Kpos[0] < kk  # (the weights apply to the kept pairs, and bite)


def test_symmetric(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, keep = metric_case(oracle, 2049)

    def prepare(ctx):
        ctx.set_model_normals(nrm)
        ctx.set_scene_normals(U0)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_symmetric(True)

    check_metric(m, p, keep, run_unique(amd, m, p, 1, prepare=prepare),
                 S.symm_ref(oracle, m, nrm, p[keep], U0[keep], 0.0, 1, -1.0))


def test_plane_to_plane(icp_lib, oracle):
    amd = icp_lib
    m, nrm, p, U0, keep = metric_case(oracle, 2049)

    def prepare(ctx):
        ctx.set_model_normals(nrm)
        ctx.set_scene_normals(U0)
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        ctx.set_plane_to_plane(GI.EPS)

    check_metric(m, p, keep, run_unique(amd, m, p, 1, prepare=prepare),
                 GI.gicp_ref(oracle, m, nrm, p[keep], U0[keep], GI.EPS, 0.0, 1, -1.0))


# 7. search paths: the indices are the same whatever searches, and neither the min pass nor the
# kept-pairs kernels depend on the variant
def test_variants_bitwise_at_4097(icp_lib, oracle):
    amd = icp_lib
    m, p, dmax, f, iters, _r = U.reference(oracle, ("size", 4097))
    a = run_unique(amd, m, p, iters)
    for mode, variant in ((amd.NN_FP64, None), (amd.NN_CERTIFIED, amd.VARIANT_VALU), (amd.NN_CERTIFIED, amd.VARIANT_MFMA),
                          (amd.NN_CERTIFIED, amd.VARIANT_MFMA16), (amd.NN_CERTIFIED, amd.VARIANT_GRID),
                          (amd.NN_CERTIFIED, amd.VARIANT_BUNDLE)):
        b = run_unique(amd, m, p, iters, mode=mode, variant=variant)
        for j in (1, 2, 3, 4):
            np.testing.assert_array_equal(b[j], a[j])
        assert b[5] == a[5]


def test_a_scene_in_slot_order(icp_lib):
    """Two plain iterations at 65,536 points leave the scene in slot order; a one-to-one iteration on
    that context against one on a fresh context given the same scene (file order): the same bits
    enter, so K and the mask (the caller's order) are equal; the sums fold in another order."""
    amd = icp_lib
    n = 65536
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(2, -1.0)
        mid = ctx.get_scene()
        ctx.set_one_to_one(True)
        _res, errs_a = ctx.run(1, -1.0)
        ka, (mask_a, cnt_a), scene_a = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene()
    _res, errs_b, scene_b, kb, mask_b, cnt_b = run_unique(amd, m, mid, 1)
    print("K", list(ka), list(kb), "err", errs_a, errs_b)
    assert list(ka) == list(kb) and cnt_a == cnt_b == mask_a.sum() and 4 <= cnt_a < n - k
    np.testing.assert_array_equal(mask_a, mask_b)
    np.testing.assert_allclose(errs_a, errs_b, rtol=1e-11)
    np.testing.assert_allclose(scene_a, scene_b, atol=1e-12)


# 8. off is off: set_one_to_one(0) after set_one_to_one(1) equals a context that never made the call
@pytest.mark.parametrize("dmax", [0.0, 0.12], ids=["plain", "gated"])
def test_off_is_off(icp_lib, oracle, dmax):
    amd = icp_lib
    m, p, _d, _f, _it, _r = U.reference(oracle, ("noisy", 4097, "gate"))

    def run(switch):
        with amd.Context() as ctx:
            ctx.set_model(m)
            ctx.set_scene(p)
            if dmax:
                ctx.set_max_distance(dmax)
            if switch:
                ctx.set_one_to_one(1)
                ctx.set_one_to_one(0)
            res, errs = ctx.run(5, -1.0)
            if not dmax:
                with pytest.raises(amd.ICPError) as ei:  # no gated run: nothing to report
                    ctx.inliers()
                assert ei.value.code == amd.ICP_E_NO_MODEL
                extra = ()
            else:
                extra = (ctx.inliers()[0], ctx.inlier_trace())
            return (errs, ctx.get_scene(), np.array(res.R), np.array(res.t), np.float64(res.s)) + extra

    for a, b in zip(run(False), run(True)):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


# 9. K below the least count stops the run before anything changes
def test_too_few_stops_before_the_iteration(icp_lib, oracle):
    amd = icp_lib
    m, p = U.few_case()
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_one_to_one(True)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(3, -1.0)
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS
        print(str(ei.value))
        assert "iteration 0" in str(ei.value) and "K = 3" in str(ei.value) and "one-to-one is on" in str(ei.value)
        assert bits(ctx.get_scene()).tolist() == bits(p).tolist()
        mask, k = ctx.inliers()
        assert k == 3 and mask.sum() == 3
        assert ctx.inlier_trace().size == 0


# 10. ranks are refused before anything is enqueued
def test_two_ranks_are_refused(icp_lib, oracle):
    amd = icp_lib
    m, p, _d, _f, _it, _r = U.reference(oracle, ("size", 257))
    calls = []
    b, c = amd.shard_range(p.shape[0], 0, 2)
    with amd.Context(0, 0, rank=0, world_size=2, host_allreduce=lambda buf: calls.append(buf.size)) as ctx:
        ctx.set_model(m)
        ctx.set_scene(p[b:b + c], np_total=p.shape[0])
        ctx.set_one_to_one(True)
        del calls[:]
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(3, -1.0)
        print(str(ei.value))
        assert ei.value.code == amd.ICP_E_ARG and "one_to_one" in str(ei.value) and "world_size" in str(ei.value)
        assert calls == []
        assert bits(ctx.get_scene()).tolist() == bits(p[b:b + c]).tolist()


# 11. a bad argument leaves the earlier setting; the setting survives icp_set_scene / icp_set_model
def test_argument_errors(icp_lib, oracle):
    amd = icp_lib
    m, p, _d, _f, _it, r = U.reference(oracle, ("size", 257), iters=1)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_one_to_one(1)
        for bad in (2, -1, 7):
            with pytest.raises(amd.ICPError) as ei:
                ctx.set_one_to_one(bad)
            assert ei.value.code == amd.ICP_E_ARG
        ctx.run(1, -1.0)
        assert list(ctx.inlier_trace()) == r["K"]  # (still on)
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(1, -1.0)
        assert list(ctx.inlier_trace()) == r["K"]
        np.testing.assert_array_equal(ctx.inliers()[0], r["mask"])


# 12. CLI
def test_cli_one_to_one(icp_lib, oracle, tmp_path):
    amd = icp_lib
    m, p, _d, _f, iters, _r = U.reference(oracle, ("partial",))
    mf, pf = str(tmp_path / "m.txt"), str(tmp_path / "p.txt")
    amd.write_matrix(mf, m)
    amd.write_matrix(pf, p)
    model, scene = amd.load_matrix(mf), amd.load_matrix(pf)  # the rounded clouds: the input of both sides
    r = subprocess.run([os.path.join(BUILD, "icp-gpu"), mf, pf, str(iters), "--one-to-one"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:
        ctx.set_model(model)
        ctx.set_scene(scene)
        ctx.set_one_to_one(True)
        res, errs = ctx.run(iters)
        g = str(tmp_path / "g.txt")
        amd.write_matrix(g, ctx.get_scene())
    print("iterations", res.iterations, "err", errs[-1])
    assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
    assert open(tmp_path / "output.txt", "rb").read() == open(g, "rb").read()
