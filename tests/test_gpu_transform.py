"""icp_get_transform and icp_transform_scene (include/icp_capi.h).

The total against the moved scene: icp_get_transform applied in numpy to the scene as it was set
agrees with icp_get_scene within 8 x G, G the gap the fp64 numpy twin shows between its own composed
total and its own moved scene (tests/test_voxel_ref.py measures it; voxel_ref.G_REL is G over the
scene's largest |coordinate|, so that it carries to other clouds).  The 8 is for the device's
different but equally fp64 summation order in the steps.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import datasets
import voxel_ref as V

pytestmark = pytest.mark.gpu


def bound(p):
    return 8.0 * V.G_REL * float(np.abs(p).max())


def total_gap(ctx, p0):
    s, R, t = ctx.transform()
    gap = float(np.abs((p0 @ (s * R).T + t) - ctx.get_scene()).max())
    print(f"total against the moved scene: {gap:.3e} (bound {bound(p0):.3e})")
    return gap


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist() for a in arrays]


def step_bits(s, R, t):
    return bits([s], np.asarray(R).reshape(-1), t)


@pytest.fixture(scope="module")
def cow(icp_lib):
    return icp_lib.load_matrix(datasets.path("cow_ref")), icp_lib.load_matrix(datasets.path("cow_tr2"))


def test_cow_one_launch_and_launch_loop(icp_lib, cow):
    amd = icp_lib
    m, p = cow
    totals = []
    for mode in (amd.RUN_PERSISTENT, amd.RUN_LAUNCHES):
        with amd.Context() as ctx:
            ctx.set_run_mode(mode)
            ctx.set_model(m)
            ctx.set_scene(p)
            assert step_bits(*ctx.transform()) == step_bits(1.0, np.eye(3), np.zeros(3))
            res, errs = ctx.run(30)
            assert res.converged and res.iterations > 3
            assert ctx.stats()["persistent_runs"] == (1 if mode == amd.RUN_PERSISTENT else 0)
            assert total_gap(ctx, p) <= bound(p)
            totals.append(step_bits(*ctx.transform()))
    assert totals[0] == totals[1]  # (the run modes are bit-identical, their totals too)


@pytest.mark.parametrize("n", [4097, 65536])
def test_synthetic_pair_fused_paths(icp_lib, n):
    """The grid variant: 4,097 points (the launch loop's fused tail) and 2^16 points (a scene in slot
    order: the canonical schedule's fused grid iterations, as tests/test_gpu_fused_lattice.py runs them)."""
    amd = icp_lib
    m, p = amd.synthetic_pair(n)
    with amd.Context() as ctx:
        ctx.set_nn_variant(amd.VARIANT_GRID)
        ctx.set_model(m)
        ctx.set_scene(p)
        res, _ = ctx.run(8, -1.0)
        assert res.iterations == 8
        assert total_gap(ctx, p) <= bound(p)


@pytest.mark.parametrize("kind", ["gated", "plane", "tukey"])
def test_kept_pairs_runs(icp_lib, cow, kind):
    amd = icp_lib
    m, p = cow
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        if kind == "gated":
            ctx.set_max_distance(0.7)
        elif kind == "plane":
            ctx.estimate_model_normals(12)
            ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
        else:
            ctx.set_robust(amd.ROBUST_TUKEY, 1.0)
        res, _ = ctx.run(12, -1.0)
        assert res.iterations == 12
        s, _, _ = ctx.transform()
        assert (s == 1.0) if kind == "plane" else (s != 1.0)
        assert total_gap(ctx, p) <= bound(p)


def test_two_runs_and_a_run_of_none(icp_lib, cow):
    amd = icp_lib
    m, p = cow
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(0)
        assert step_bits(*ctx.transform()) == step_bits(1.0, np.eye(3), np.zeros(3))
        ctx.run(3, -1.0)
        first = ctx.transform()
        ctx.run(4, -1.0)
        assert step_bits(*first) != step_bits(*ctx.transform())
        assert total_gap(ctx, p) <= bound(p)
        ctx.set_scene(p)  # a new scene: the identity again
        assert step_bits(*ctx.transform()) == step_bits(1.0, np.eye(3), np.zeros(3))


def test_increment_is_the_total_after_one_iteration(icp_lib, cow):
    amd = icp_lib
    m, p = cow
    for mode in (amd.RUN_PERSISTENT, amd.RUN_LAUNCHES):
        with amd.Context() as ctx:
            ctx.set_run_mode(mode)
            ctx.set_model(m)
            ctx.set_scene(p)
            res, _ = ctx.run(1, -1.0)
            assert step_bits(res.s, np.array(res.R[:]), np.array(res.t[:])) == step_bits(*ctx.transform())


def test_too_few_keeps_the_completed_iterations(icp_lib):
    amd = icp_lib
    m, p, dmax, completed = V.too_few_case()
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(dmax)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(8, -1.0)
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS and f"iteration {completed}" in str(ei.value)
        stopped = ctx.transform()
        assert total_gap(ctx, p) <= bound(p)
    with amd.Context() as ctx:  # the same gate, the completed iterations alone
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(dmax)
        ctx.run(completed, -1.0)
        assert step_bits(*ctx.transform()) == step_bits(*stopped)


class HostAllReduce:
    """The host all-reduce of W ranks run as W threads (the pattern of test_gpu_sharded.py)."""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world, timeout=120)
        self.bufs = [None] * world

    def for_rank(self, r):
        def reduce(buf):
            self.bufs[r] = buf.copy()
            self.bar.wait()
            acc = self.bufs[0].copy()
            for k in range(1, self.world):  # fixed rank order: identical on every rank
                acc += self.bufs[k]
            self.bar.wait()
            buf[:] = acc
        return reduce


def test_two_ranks_stop_on_the_threshold(icp_lib, cow):
    """The lagged loop: the iteration after the converged one is searched but never applied."""
    amd = icp_lib
    m, p = cow
    red = HostAllReduce(2)
    results, errors = [None, None], []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, 2)
            with amd.Context(0, amd.NN_CERTIFIED, rank=r, world_size=2, host_allreduce=red.for_rank(r)) as ctx:
                ctx.set_model(m)
                ctx.set_scene(p[b:b + c], np_total=p.shape[0])
                res, _ = ctx.run(30)
                s, R, t = ctx.transform()
                results[r] = (res.converged, res.iterations, (s, R, t), ctx.get_scene(), p[b:b + c])
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errors, errors
    assert results[0][0] and results[0][1] < 30
    assert step_bits(*results[0][2]) == step_bits(*results[1][2])
    for _, _, (s, R, t), scene, shard in results:
        gap = float(np.abs((shard @ (s * R).T + t) - scene).max())
        print(f"shard: {gap:.3e} (bound {bound(p):.3e})")
        assert gap <= bound(p)


# ---- icp_transform_scene -------------------------------------------------------------------------

def pose():
    a = np.deg2rad(7.0)
    ax = np.array([2.0, -1.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return 1.03, np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K), np.array([0.05, -0.02, 0.04])


@pytest.mark.parametrize("n", [2903, 12289])
def test_transform_scene(icp_lib, cow, n):
    amd = icp_lib
    if n == 2903:
        m, p = cow
    else:
        m, p = amd.synthetic_pair(n)
    s, R, t = pose()
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(2, -1.0)  # (a scene with correspondences and a total already)
        before, first = ctx.get_scene(), ctx.transform()
        ctx.transform_scene(s, R, t)
        moved = ctx.get_scene()
        # the moved points: sR formed once, three products and three additions a row
        sR = s * R
        tol = 4.0 * V.U * (np.abs(before) @ np.abs(sR).T + np.abs(t))
        assert (np.abs(moved - (before @ sR.T + t)) <= tol).all()
        # the total composes: (s, R, t) o first
        ts, tR, tt = ctx.transform()
        assert abs(ts - s * first[0]) <= 4 * V.U * ts
        assert np.abs(tR - R @ first[1]).max() <= 8 * V.U
        assert np.abs(tt - (sR @ first[2] + t)).max() <= 16 * V.U * (np.abs(first[2]).max() + np.abs(t).max())
        assert total_gap(ctx, p) <= bound(p)
        res, errs = ctx.run(5, -1.0)
        scene, idx = ctx.get_scene(), ctx.get_indices()
    with amd.Context() as ctx:  # a fresh context given the moved points
        ctx.set_model(m)
        ctx.set_scene(moved)
        res2, errs2 = ctx.run(5, -1.0)
        assert bits(errs) == bits(errs2)
        assert bits(scene) == bits(ctx.get_scene()) and np.array_equal(idx, ctx.get_indices())
        assert step_bits(res.s, np.array(res.R[:]), np.array(res.t[:])) == \
            step_bits(res2.s, np.array(res2.R[:]), np.array(res2.t[:]))


def check_pose_then_run(amd, m, p, allow_unequal=False, model2=None):
    """test_transform_scene's pattern: two iterations, [a new model], the pose, then the moved points
    against numpy, the total's composition, and five more iterations bit for bit against a fresh context
    given the moved points."""
    s, R, t = pose()
    with amd.Context() as ctx:
        ctx.set_allow_unequal(allow_unequal)
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(2, -1.0)
        before, first = ctx.get_scene(), ctx.transform()
        if model2 is not None:  # (a scene in slot order then waits to be put back into file order)
            ctx.set_model(model2)
        ctx.transform_scene(s, R, t)
        moved = ctx.get_scene()
        sR = s * R
        tol = 4.0 * V.U * (np.abs(before) @ np.abs(sR).T + np.abs(t))
        assert (np.abs(moved - (before @ sR.T + t)) <= tol).all()
        ts, tR, tt = ctx.transform()
        assert abs(ts - s * first[0]) <= 4 * V.U * ts
        assert np.abs(tR - R @ first[1]).max() <= 8 * V.U
        assert np.abs(tt - (sR @ first[2] + t)).max() <= 16 * V.U * (np.abs(first[2]).max() + np.abs(t).max())
        assert total_gap(ctx, p) <= bound(p)
        res, errs = ctx.run(5, -1.0)
        scene, idx = ctx.get_scene(), ctx.get_indices()
    with amd.Context() as ctx:
        ctx.set_allow_unequal(allow_unequal)
        ctx.set_model(m if model2 is None else model2)
        ctx.set_scene(moved)
        res2, errs2 = ctx.run(5, -1.0)
        assert res.iterations == res2.iterations == 5
        assert bits(errs) == bits(errs2)
        assert np.array_equal(idx, ctx.get_indices())
        assert bits(scene) == bits(ctx.get_scene())
        assert step_bits(res.s, np.array(res.R[:]), np.array(res.t[:])) == \
            step_bits(res2.s, np.array(res2.R[:]), np.array(res2.t[:]))


@pytest.mark.parametrize("n", [65536, 65537])
def test_transform_scene_in_slot_order(icp_lib, n):
    """Two iterations at 2^16 points and more leave the scene in slot order (tests/test_gpu_plane.py's case
    8 relies on it), so the pose un-permutes it.  65,536: the largest scene prepared through the mapped
    buffer; 65,537: the staged path, whose preparation sorts the moved points into a new slot order."""
    m, p = icp_lib.synthetic_pair(n)
    check_pose_then_run(icp_lib, m, p)


def test_transform_scene_staged_in_file_order(icp_lib):
    """A 70,000-point scene against a 4,097-point model: staged, and too small a model for slot order."""
    amd = icp_lib
    m, _ = amd.synthetic_pair(4097)
    r = np.random.default_rng(70000)
    p = np.tile(m, (18, 1))[:70000] + 0.01 * r.standard_normal((70000, 3))
    check_pose_then_run(amd, m, p, allow_unequal=True)


def test_transform_scene_with_a_revert_pending(icp_lib):
    """set_model on a scene in slot order only marks it (the next run puts it back into file order); a
    pose before that run moves the scene as it was, in the caller's order."""
    m, p = icp_lib.synthetic_pair(65536)
    check_pose_then_run(icp_lib, m, p, model2=m + np.array([0.01, 0.0, 0.0]))


def test_transform_scene_on_two_ranks(icp_lib, cow):
    amd = icp_lib
    m, p = cow
    s, R, t = pose()

    def sequence(ctx):
        r1, e1 = ctx.run(2, -1.0)
        ctx.transform_scene(s, R, t)
        r2, e2 = ctx.run(3, -1.0)
        assert r1.iterations == 2 and r2.iterations == 3
        return np.concatenate([e1, e2]), ctx.transform(), ctx.get_scene()

    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        single = sequence(ctx)
    red = HostAllReduce(2)
    results, errors = [None, None], []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, 2)
            with amd.Context(0, amd.NN_CERTIFIED, rank=r, world_size=2, host_allreduce=red.for_rank(r)) as ctx:
                ctx.set_model(m)
                ctx.set_scene(p[b:b + c], np_total=p.shape[0])
                results[r] = sequence(ctx) + (p[b:b + c],)
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not errors, errors
    assert step_bits(*results[0][1]) == step_bits(*results[1][1])
    assert bits(results[0][0]) == bits(results[1][0])
    for _, (ts, tR, tt), scene, shard in results:
        gap = float(np.abs((shard @ (ts * tR).T + tt) - scene).max())
        print(f"shard: {gap:.3e} (bound {bound(p):.3e})")
        assert gap <= bound(p)
    np.testing.assert_allclose(results[0][0], single[0], rtol=1e-11)
    np.testing.assert_allclose(np.concatenate([r[2] for r in results]), single[2], atol=1e-12)


def test_transform_errors(icp_lib, cow):
    amd = icp_lib
    m, p = cow
    s, R, t = pose()
    L = amd.lib()
    dp = C.POINTER(C.c_double)
    with amd.Context() as ctx:
        ctx.set_model(m)
        with pytest.raises(amd.ICPError) as e:
            ctx.transform()
        assert e.value.code == amd.ICP_E_NO_MODEL
        with pytest.raises(amd.ICPError) as e:
            ctx.transform_scene(s, R, t)
        assert e.value.code == amd.ICP_E_NO_MODEL
        ctx.set_scene(p)
        Rn, tn = R.copy(), t.copy()
        Rn[1, 1] = np.nan
        tn[2] = np.inf
        for args in ((0.0, R, t), (-1.0, R, t), (np.nan, R, t), (np.inf, R, t), (s, Rn, t), (s, R, tn)):
            with pytest.raises(amd.ICPError) as e:
                ctx.transform_scene(*args)
            assert e.value.code == amd.ICP_E_ARG
        Rf = np.ascontiguousarray(R).reshape(-1)
        assert L.icp_transform_scene(ctx._h, s, None, t.ctypes.data_as(dp)) == amd.ICP_E_ARG
        assert L.icp_transform_scene(ctx._h, s, Rf.ctypes.data_as(dp), None) == amd.ICP_E_ARG
        out = np.zeros(13)
        assert L.icp_get_transform(ctx._h, None, out[1:].ctypes.data_as(dp), out[10:].ctypes.data_as(dp)) == amd.ICP_E_ARG
        # nothing moved, nothing composed
        assert bits(ctx.get_scene()) == bits(p)
        assert step_bits(*ctx.transform()) == step_bits(1.0, np.eye(3), np.zeros(3))
