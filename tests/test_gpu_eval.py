"""icp_evaluate and icp_evaluate_device (icp_eval.hip) against tests/eval_ref.py, the header's rules
restated in numpy.

The per-point indices and d2 are compared exactly (the same fp64 expression, the first minimum), and so
are K, K_m, the maxima and the fitness values.  The reference sums with math.fsum (exactly rounded);
the device's S adds n non-negative terms, each addition rounding by at most 2^-53 relative of a partial sum
that is at most the total: inlier_rmse is within (n + 8) 2^-53 relative (the n roundings, the division, a
root that may be one ulp off), and an entry of the information matrix within (n + 4) 2^-53 of the sum of
the |terms| it is made of, that sum taken by the reference.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import eval_ref as E
import gated_ref as G
import plane_ref as P

pytestmark = pytest.mark.gpu

INF = float("inf")
SCALARS = ("scene_points", "correspondences", "fitness", "max_inlier_d2", "model_points", "model_correspondences",
           "model_fitness", "model_max_inlier_d2")
ALL_SCALARS = SCALARS + ("inlier_rmse", "model_rmse")


@pytest.fixture(scope="module")
def ctx(icp_lib):
    with icp_lib.Context() as c:
        yield c


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b)) if b else abs(float(a))


def check(got, ref, both, what):
    """a device result against eval_ref.evaluate's: exact but for the sums"""
    n, nm = ref["scene_points"], ref["model_points"]
    A, B = ref["information"], ref["information_bound"]
    print(what, "both" if both else "forward", "K", got["correspondences"], "of", got["scene_points"], "K_m",
          got["model_correspondences"], "rmse rel.", rel(got["inlier_rmse"], ref["inlier_rmse"]), "model rmse rel.",
          rel(got["model_rmse"], ref["model_rmse"]) if both else "-", "information: largest error / bound",
          float(np.max(np.abs(got["information"] - A) / np.where(B > 0, B, 1.0))))
    np.testing.assert_array_equal(got["idx"], ref["idx"])
    np.testing.assert_array_equal(got["d2"], ref["d2"])
    assert got["idx"].dtype == np.int32
    for k in SCALARS:
        want = ref[k] if both or not k.startswith("model_") else 0
        assert got[k] == want, (what, k, got[k], want)
    assert rel(got["inlier_rmse"], ref["inlier_rmse"]) <= (n + 8) * 2.0 ** -53
    assert got["information"].shape == (6, 6)
    assert np.all(np.abs(got["information"] - A) <= (n + 4) * 2.0 ** -53 * B)
    np.testing.assert_array_equal(got["information"], got["information"].T)
    if both:
        np.testing.assert_array_equal(got["model_idx"], ref["model_idx"])
        np.testing.assert_array_equal(got["model_d2"], ref["model_d2"])
        assert rel(got["model_rmse"], ref["model_rmse"]) <= (nm + 8) * 2.0 ** -53
    else:
        assert got["model_rmse"] == 0.0 and "model_idx" not in got


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


# 1. every row of the table, forward and both
@pytest.mark.parametrize("name", E.CASES)
def test_table(ctx, oracle, name):
    for d, K, Km in E.COUNTS[name]:
        m, p, md, ref = E.reference(name, d, oracle.load_matrix)
        ctx.set_model(m)
        ctx.set_scene(p)
        for both in (False, True):
            got = ctx.evaluate(md, both=both, per_point=True)
            check(got, ref, both, "%s at %g" % (name, md))
            assert got["correspondences"] == K
            if both and Km is not None:
                assert got["model_correspondences"] == Km
            lean = ctx.evaluate(md, both=both)  # (the per-point arrays are optional)
            for k in ALL_SCALARS:
                assert lean[k] == got[k]
            np.testing.assert_array_equal(lean["information"], got["information"])
    if name == "lattice_edge":  # K == 0 is a result, not an error
        assert got["correspondences"] == 0 and got["fitness"] == 0.0 and got["inlier_rmse"] == 0.0
        assert got["max_inlier_d2"] == 0.0 and not got["information"].any()
    if name == "cow_partial":
        assert abs(got["max_inlier_d2"] - 1.47755) < 5e-6 and got["fitness"] == 1.0


# 2. determinism and the device form
@pytest.mark.parametrize("name,d", [("synth4097", 0.08), ("cow_partial", "0.2ext"), ("far", 0.2), ("cow_partial", INF)])
def test_two_calls_and_the_device_form_give_the_same_bits(icp_lib, ctx, oracle, name, d):
    m, p, md, _ = E.reference(name, d, oracle.load_matrix)
    ctx.set_model(m)
    ctx.set_scene(p)
    a = ctx.evaluate(md, both=True, per_point=True)
    b = ctx.evaluate(md, both=True, per_point=True)
    same_bits(a, b)
    with icp_lib.Context() as other:
        other.set_model(m)
        other.set_scene(p)
        same_bits(a, other.evaluate(md, both=True, per_point=True))
    n, nm = p.shape[0], m.shape[0]
    idx = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d2 = torch.full((n,), -9.0, dtype=torch.float64, device="cuda")
    midx = torch.full((nm,), -9, dtype=torch.int32, device="cuda")
    md2 = torch.full((nm,), -9.0, dtype=torch.float64, device="cuda")
    dev = ctx.evaluate_device(md, True, idx.data_ptr(), d2.data_ptr(), midx.data_ptr(), md2.data_ptr())
    torch.cuda.synchronize()
    dev.update(idx=idx.cpu().numpy(), d2=d2.cpu().numpy(), model_idx=midx.cpu().numpy(), model_d2=md2.cpu().numpy())
    same_bits(a, dev)
    fwd = ctx.evaluate_device(md, False, idx.data_ptr())  # (every array is optional)
    for k in ("correspondences", "fitness", "inlier_rmse", "max_inlier_d2"):
        assert fwd[k] == a[k]
    np.testing.assert_array_equal(fwd["information"], a["information"])


# 3. at a moved pose: after applied iterations, and after a transform_scene
@pytest.mark.parametrize("name,d", [("synth4097", 0.12), ("cow_partial", "0.2ext")])
def test_at_a_moved_pose(icp_lib, oracle, name, d):
    m, p, md, _ = E.reference(name, d, oracle.load_matrix)
    with icp_lib.Context() as c:
        c.set_model(m)
        c.set_scene(p)
        c.run(6, -1.0)
        scene = c.get_scene()
        assert not np.array_equal(scene, p)
        check(c.evaluate(md, both=True, per_point=True), E.evaluate(m, scene, md, both=True), True, name + " after 6 iterations")
        c.transform_scene(1.01, P.rot((3, -1, 2), 2.0), np.array([0.01, 0.02, -0.015]))
        scene = c.get_scene()
        check(c.evaluate(md, both=True, per_point=True), E.evaluate(m, scene, md, both=True), True, name + " after a transform_scene")
        check(c.evaluate(md, per_point=True), E.evaluate(m, scene, md), False, name + " after a transform_scene")


# 4. the call changes nothing a run or a report depends on
def run_record(c, res, errs):
    return [errs, np.array(res.R), res.s, np.array(res.t), res.err, res.iterations, c.get_scene(), c.get_indices(),
            np.concatenate([np.ravel(x) for x in c.transform()])]


@pytest.mark.parametrize("name,d", [("synth4097", 0.12), ("cow_partial", "0.2ext")])
def test_a_run_after_the_evaluation_is_the_run_without_it(icp_lib, oracle, name, d):
    m, p, md, _ = E.reference(name, d, oracle.load_matrix)
    records = []
    for form in ("plain", "evaluated"):
        with icp_lib.Context() as c:
            c.set_model(m)
            c.set_scene(p)
            c.set_max_distance(3 * md)
            first = run_record(c, *c.run(3, -1.0))
            if form == "evaluated":
                before = (c.get_indices(), c.inliers(), c.inlier_trace())
                c.evaluate(md, both=True, per_point=True)
                c.evaluate(INF)
                after = (c.get_indices(), c.inliers(), c.inlier_trace())
                np.testing.assert_array_equal(before[0], after[0])
                np.testing.assert_array_equal(before[1][0], after[1][0])
                assert before[1][1] == after[1][1]
                np.testing.assert_array_equal(before[2], after[2])
            records.append(first + run_record(c, *c.run(3, -1.0)))
    for a, b in zip(*records):
        np.testing.assert_array_equal(a, b)


# 5. a scene the engine keeps in slot order
def test_a_slot_ordered_scene(icp_lib):
    amd = icp_lib
    n, md = 65536, 0.02
    m, p = amd.synthetic_pair(n)
    with amd.Context() as c:
        c.set_model(m)
        c.set_scene(p)
        c.run(3, -1.0)
        got = c.evaluate(md, both=True, per_point=True)
        fwd = c.evaluate(md, per_point=True)
        scene = c.get_scene()
        Y, near = c.closest_matrix(scene)
    D = np.float64(md) * np.float64(md)
    kept = got["idx"] >= 0
    K = int(kept.sum())
    print("n", n, "max_dist", md, "K", K, "K_m", got["model_correspondences"], "fitness", got["fitness"], "rmse",
          got["inlier_rmse"])
    np.testing.assert_array_equal(fwd["idx"], got["idx"])  # the resident (slot) order and the grid order of the queries
    np.testing.assert_array_equal(fwd["d2"], got["d2"])
    for k in ("correspondences", "fitness", "inlier_rmse", "max_inlier_d2"):
        assert fwd[k] == got[k]
    np.testing.assert_array_equal(fwd["information"], got["information"])
    np.testing.assert_array_equal(got["idx"][kept], near[kept])
    d_all = G.d2_of(scene, Y)
    np.testing.assert_array_equal(got["d2"][kept], d_all[kept])
    np.testing.assert_array_equal(kept, d_all <= D)
    assert np.all(np.isinf(got["d2"][~kept]))
    r = np.random.default_rng(11)
    q = r.choice(n, 256, replace=False)  # by brute force, both directions
    bi, bd = E.gate(*E.nearest(scene[q], m), md)
    np.testing.assert_array_equal(got["idx"][q], bi)
    np.testing.assert_array_equal(got["d2"][q], bd)
    bi, bd = E.gate(*E.nearest(m[q], scene), md)
    np.testing.assert_array_equal(got["model_idx"][q], bi)
    np.testing.assert_array_equal(got["model_d2"][q], bd)
    # K and the sums over the returned arrays
    assert got["correspondences"] == K and got["fitness"] == K / n and got["scene_points"] == n
    assert got["max_inlier_d2"] == (got["d2"][kept].max() if K else 0.0)
    assert rel(got["inlier_rmse"], math.sqrt(math.fsum(got["d2"][kept]) / K) if K else 0.0) <= (n + 8) * 2.0 ** -53
    A, B = E.information(m, got["idx"])
    assert np.all(np.abs(got["information"] - A) <= (n + 4) * 2.0 ** -53 * B)
    mk = got["model_idx"] >= 0
    Km = int(mk.sum())
    assert got["model_correspondences"] == Km and got["model_fitness"] == Km / n
    assert got["model_max_inlier_d2"] == (got["model_d2"][mk].max() if Km else 0.0)
    assert rel(got["model_rmse"], math.sqrt(math.fsum(got["model_d2"][mk]) / Km) if Km else 0.0) <= (n + 8) * 2.0 ** -53
    np.testing.assert_array_equal(got["model_d2"][mk], G.d2_of(m[mk], scene[got["model_idx"][mk]]))


# 6. the errors of rule 8: nothing has run, nothing is written
FILL = 123.25


def raw(amd, c, max_dist, both, null_out=False, model_arrays=False, n=8):
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ev = amd.Evaluation()
    C.memset(C.byref(ev), 0x5A, C.sizeof(ev))
    fill = bytes(ev)
    idx, d2 = np.full(n, -5, dtype=np.int32), np.full(n, FILL)
    midx, md2 = np.full(n, -5, dtype=np.int32), np.full(n, FILL)
    rc = amd.lib().icp_evaluate(c._h if c is not None else None, max_dist, both, None if null_out else C.byref(ev),
                                ip(idx), dp(d2), ip(midx) if model_arrays else None, dp(md2) if model_arrays else None)
    clean = bytes(ev) == fill and np.all(idx == -5) and np.all(d2 == FILL) and np.all(midx == -5) and np.all(md2 == FILL)
    return rc, clean


def test_refusals_name_the_value_and_write_nothing(icp_lib):
    amd = icp_lib
    A, N = amd.ICP_E_ARG, amd.ICP_E_NO_MODEL
    m, p = E.clouds("synth5")
    m8 = np.ascontiguousarray(np.concatenate([m, m[:3] + 0.5]))
    with amd.Context() as c:
        assert raw(amd, None, 1.0, 0) == (A, True)
        for args, code, word in (((1.0, 0), N, "no model"),):
            rc, clean = raw(amd, c, *args)
            assert rc == code and clean and word in amd.lib().icp_last_error(c._h).decode()
        c.set_model(m8)
        rc, clean = raw(amd, c, 1.0, 0)
        assert rc == N and clean and "no scene" in amd.lib().icp_last_error(c._h).decode()
        c.set_scene(np.ascontiguousarray(m8[::-1] + 0.01))
        cases = [((1.0, 0, True), A, "out is null"), ((0.0, 0), A, "max_dist = 0"), ((-1.0, 1), A, "max_dist = -1"),
                 ((float("nan"), 0), A, "max_dist = nan"), ((1.0, 0, False, True), A, "both = 0")]
        for args, code, word in cases:
            rc, clean = raw(amd, c, *args)
            msg = amd.lib().icp_last_error(c._h).decode()
            print(rc, msg)
            assert rc == code and clean and word in msg, (args, rc, msg)
        rc, clean = raw(amd, c, 1.0, 1, False, True)  # and a good call after all of them
        assert rc == amd.ICP_OK and not clean
        rc, clean = raw(amd, c, INF, 0)
        assert rc == amd.ICP_OK and not clean
    box = {}

    def reduce_(buf):  # (a two-rank context of host all-reduces; never called: the call is refused first)
        box["called"] = True

    with amd.Context(rank=0, world_size=2, host_allreduce=reduce_) as c2:
        c2.set_model(m8)
        c2.set_scene(np.ascontiguousarray(m8[:4]), np_total=8)
        rc, clean = raw(amd, c2, 1.0, 0, n=4)
        msg = amd.lib().icp_last_error(c2._h).decode()
        print(rc, msg)
        assert rc == A and clean and "2 ranks" in msg and "called" not in box


# 7. memory: the context keeps the call's block (engine::Scratch's kept mode, as the filters'); what that can
# get wrong is an array left over from another call or another size, so a sequence of calls of different
# sizes on ONE context -- the first with the block still empty, later ones growing it or inside it -- must
# give, bit for bit, what each gives as the first call on a fresh context (the check of
# tests/test_gpu_cloud_scratch.py).  And a second call at the same sizes allocates nothing: the first call at
# 65,536 points (some 20 MB, far above the allocator's granule) does not fit the block the 4,097-point calls
# left, takes allocations of its own, frees them and leaves the block grown; the device's free memory must
# then be the same before and after the second and the third call.  (A call's own allocations are freed
# before it returns, so free memory shows the block's growth: growth at the second call is what is ruled out.)
def test_a_sequence_on_one_context_is_each_call_on_a_fresh_one(icp_lib, oracle):
    amd = icp_lib
    steps = [("synth257", 0.12, True), ("synth4097", 0.08, True), ("synth65", 0.12, False), ("far", 0.2, True),
             ("synth4097", 0.08, True), ("pair65536", 0.02, True), ("pair65536", 0.02, True), ("pair65536", 0.02, True)]

    def clouds(name, d):
        if name == "pair65536":
            return amd.synthetic_pair(65536) + (d,)
        return E.reference(name, d)[:3]

    fresh = {}
    for name, d, both in steps:
        if (name, both) not in fresh:
            m, p, md = clouds(name, d)
            with amd.Context() as c:
                c.set_model(m)
                c.set_scene(p)
                fresh[(name, both)] = c.evaluate(md, both=both, per_point=True)
    taken = []
    with amd.Context() as c:
        for i, (name, d, both) in enumerate(steps):
            m, p, md = clouds(name, d)
            c.set_model(m)
            c.set_scene(p)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            got = c.evaluate(md, both=both, per_point=True)
            free1 = torch.cuda.mem_get_info()[0]
            taken.append(free0 - free1)
            print("step", i + 1, name, "both" if both else "forward", "device memory taken by the call", taken[-1])
            same_bits(got, fresh[(name, both)])
    assert taken[5] > 0  # (the first call at the large size grew the block: the figure can show a growth)
    assert taken[6] == 0 and taken[7] == 0
