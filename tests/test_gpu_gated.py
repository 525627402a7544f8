"""icp_run with the max-correspondence-distance gate (icp_set_max_distance, icp_gated.hip)
against tests/gated_ref.py, the gated loop restated with the oracle's pieces.

Tolerances are the project's (test_gpu_parity.py): K per iteration and the masks exact
(tests/test_gated_ref.py checks on the CPU that no pair of these inputs lies within 1e-6 of the
gate), err rel 1e-9, s and R abs 1e-9, new_p abs 1e-9 x extent.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import datasets
import gated_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


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


def run_gated(amd, m, p, dmax, iters, threshold, mode=0, variant=None):
    """-> (res, errs, scene, K trace, mask, K last) of a fresh context."""
    with amd.Context(0, mode) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(dmax)
        res, errs = ctx.run(iters, threshold)
        mask, k = ctx.inliers()
        return res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, k


def check_against_ref(m, out, r):
    res, errs, scene, ktrace, mask, k = out
    print("K", list(ktrace), "err", errs, "ref err", r["err"])
    assert res.iterations == r["iterations"]
    assert list(ktrace) == r["K"] and k == r["K"][-1]
    np.testing.assert_array_equal(mask, r["mask"])
    np.testing.assert_allclose(errs, r["err"], rtol=1e-9)
    assert abs(res.s - r["s"]) <= 1e-9
    np.testing.assert_allclose(np.array(res.R).reshape(3, 3), r["R"], atol=1e-9)
    extent = float(np.abs(m).max())
    np.testing.assert_allclose(np.array(res.t), r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(scene, r["new_p"], atol=1e-9 * extent)


# 1. sizes: the wave tail, one workgroup, kRedSingle, the first multi-workgroup fold, an odd
# multi-block size; n = 5 sits on the minimum K = 4
@pytest.mark.parametrize("n", list(G.SIZES))
def test_sizes(icp_lib, oracle, n):
    m, p, dmax, r = G.reference(oracle, ("size", n))
    out = run_gated(icp_lib, m, p, dmax, G.SIZES_ITERS, -1.0)
    check_against_ref(m, out, r)
    assert list(out[3]) == [G.SIZES[n]] * G.SIZES_ITERS


def test_variants_bitwise_at_4097(icp_lib, oracle):
    """The indices are the same whatever searches, and the gated kernels do not depend on the
    variant: fp64 brute force and the grid variant give AUTO's run bit for bit."""
    amd = icp_lib
    m, p, dmax, _r = G.reference(oracle, ("size", 4097))
    a = run_gated(amd, m, p, dmax, G.SIZES_ITERS, -1.0)
    for mode, variant in ((amd.NN_FP64, None), (amd.NN_CERTIFIED, amd.VARIANT_GRID)):
        b = run_gated(amd, m, p, dmax, G.SIZES_ITERS, -1.0, mode=mode, variant=variant)
        np.testing.assert_array_equal(b[1], a[1])
        np.testing.assert_array_equal(b[2], a[2])
        np.testing.assert_array_equal(b[3], a[3])
        np.testing.assert_array_equal(b[4], a[4])


# 2. a gate that bites and moves
@pytest.mark.parametrize("n,dmax", list(G.BITES))
def test_gate_bites(icp_lib, oracle, n, dmax):
    m, p, d, r = G.reference(oracle, ("bite", n, dmax))
    out = run_gated(icp_lib, m, p, d, G.BITES_ITERS, -1.0)
    check_against_ref(m, out, r)
    assert (out[3][0], out[3][-1]) == G.BITES[(n, dmax)]


def test_partial_overlap_cow(icp_lib, oracle):
    m, p, d, r = G.reference(oracle, ("partial",))
    out = run_gated(icp_lib, m, p, d, 20, -1.0)
    check_against_ref(m, out, r)
    assert out[3][0] == 712 and max(out[3]) == 1530 and out[3][-1] == 1527


# 3. the purpose: a scan with a far clump registers once the far pairs are dropped
@pytest.fixture(scope="module")
def clump_single(icp_lib, oracle):
    m, p, dmax, _r = G.reference(oracle, ("clump",))
    return run_gated(icp_lib, m, p, dmax, 30, 1e-5)


def test_clump_converges_gated_only(icp_lib, oracle, clump_single):
    amd = icp_lib
    m, p, dmax, r = G.reference(oracle, ("clump",))
    res, errs, scene, ktrace, mask, k = clump_single
    print("K", list(ktrace), "err", errs)
    assert res.iterations == 16 and res.converged == 1
    assert list(ktrace) == [2201] + [2203] * 15 and k == 2203
    want = np.ones(p.shape[0], dtype=bool)
    want[-700:] = False
    np.testing.assert_array_equal(mask, want)
    np.testing.assert_array_equal(mask, r["mask"])
    np.testing.assert_allclose(errs[:-1], r["err"][:-1], rtol=1e-9)
    assert errs[-1] < 1e-5  # (2.3e-11 in the reference: asserted as below the threshold only)
    extent = float(np.abs(m).max())
    np.testing.assert_allclose(scene, r["new_p"], atol=1e-9 * extent)
    # the same input ungated does not converge in 30 iterations, as before
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ures, uerrs = ctx.run(30, 1e-5)
    u = oracle.icp(m, p, 30)
    assert ures.iterations == 30 and ures.converged == 0 and u["iterations"] == 30
    np.testing.assert_allclose(uerrs, u["err"], rtol=1e-9)
    assert uerrs[-1] > 1e-2


# 4. too few
def test_too_few_stops_before_the_iteration(icp_lib):
    amd = icp_lib
    m, p = G.synth(300, 1, 0.0)
    p = p + np.array([10.0, 0.0, 0.0])
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(1.0)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(5, -1.0)
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS
        assert "iteration 0" in str(ei.value) and "K = 0" in str(ei.value)
        np.testing.assert_array_equal(ctx.get_scene(), p)
        mask, k = ctx.inliers()
        assert k == 0 and not mask.any()
        assert ctx.inlier_trace().size == 0


# 5. off is off
def test_off_is_off(icp_lib, oracle):
    amd = icp_lib
    m, p, _tr2 = G.load_cow(oracle)
    runs = []
    for setting in (0.0, np.inf, None):
        with amd.Context() as ctx:
            ctx.set_model(m)
            ctx.set_scene(p)
            if setting is not None:
                ctx.set_max_distance(setting)
            res, errs = ctx.run(10)
            assert ctx.stats()["persistent_runs"] == 1
            with pytest.raises(amd.ICPError) as ei:  # no gated run: nothing to report
                ctx.inliers()
            assert ei.value.code == amd.ICP_E_NO_MODEL
            runs.append((errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)
    # a gate nothing reaches: K = n at every iteration, the ungated errors
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(1e6)
        res, errs = ctx.run(10)
        assert ctx.stats()["persistent_runs"] == 0
        assert list(ctx.inlier_trace()) == [p.shape[0]] * res.iterations
        mask, k = ctx.inliers()
        assert mask.all() and k == p.shape[0]
        np.testing.assert_allclose(errs, runs[0][0], rtol=1e-9)
        res0, errs0 = ctx.run(0)  # (no iteration, no gate evaluated: the last one stays)
        assert res0.iterations == 0 and errs0.size == 0 and ctx.inliers()[1] == p.shape[0]
        for bad in (-1.0, -np.inf, np.nan):
            with pytest.raises(amd.ICPError) as ei:
                ctx.set_max_distance(bad)
            assert ei.value.code == amd.ICP_E_ARG


# 6. state hygiene
def test_ungated_run_after_a_gated_one(icp_lib, oracle):
    """(a) gated 3, gate off, ungated 5 on one context == ungated 5 on a fresh context loaded with
    the scene the 3 gated iterations left, bit for bit."""
    amd = icp_lib
    m, p, dmax, _r = G.reference(oracle, ("clump",))
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(dmax)
        ctx.run(3, -1.0)
        mid = ctx.get_scene()
        ctx.set_max_distance(0.0)
        res_a, errs_a = ctx.run(5, -1.0)
        scene_a = ctx.get_scene()
        mask, k = ctx.inliers()  # (still the gated run's: no new scene since)
        assert k == 2203 and mask.sum() == 2203
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(mid)
        res_b, errs_b = ctx.run(5, -1.0)
        scene_b = ctx.get_scene()
    np.testing.assert_array_equal(errs_a, errs_b)
    np.testing.assert_array_equal(scene_a, scene_b)
    np.testing.assert_array_equal(np.array(res_a.R), np.array(res_b.R))


def test_gated_run_on_a_scene_in_slot_order(icp_lib):
    """(b) Two ungated iterations at 65,536 points leave the scene in slot order; three gated
    iterations on that context against three on a fresh context given the same scene (file
    order).  The two runs sum in different orders, so their scenes differ by rounding (~1e-15
    relative): a gate decision could differ only for a pair within that of the gate, which this
    fixed input does not have; K and the mask (the caller's order) are compared exactly."""
    amd = icp_lib
    n = 65536
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    # (the two ungated iterations, scale included, shrink the scene into the model: its pairs end
    # up some 0.05 apart, so that is where a gate still divides them)
    dmax = 0.05
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(2, -1.0)
        mid = ctx.get_scene()
        ctx.set_max_distance(dmax)
        res_a, errs_a = ctx.run(3, -1.0)
        ka, (mask_a, cnt_a), scene_a = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene()
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(mid)
        ctx.set_max_distance(dmax)
        res_b, errs_b = ctx.run(3, -1.0)
        kb, (mask_b, cnt_b), scene_b = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene()
    print("K", list(ka), list(kb), "err", errs_a, errs_b)
    assert res_a.iterations == res_b.iterations == 3
    np.testing.assert_array_equal(ka, kb)
    assert cnt_a == cnt_b == ka[-1] and 4 <= cnt_a < n
    np.testing.assert_array_equal(mask_a, mask_b)
    assert mask_a.sum() == cnt_a
    np.testing.assert_allclose(errs_a, errs_b, rtol=1e-11)
    np.testing.assert_allclose(scene_a, scene_b, atol=1e-12)


# 7. ranks
def run_gated_sharded(amd, m, p, dmax, world, iters, threshold):
    red = HostAllReduce(world)
    results = [None] * world
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                ctx.set_model(m)
                ctx.set_scene(p[b:b + c], np_total=p.shape[0])
                ctx.set_max_distance(dmax)
                res, errs = ctx.run(iters, threshold)
                mask, k = ctx.inliers()
                results[r] = (res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, k)
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
def test_ranks_match_single(icp_lib, oracle, clump_single, world):
    m, p, dmax, _r = G.reference(oracle, ("clump",))
    ref = clump_single
    out = run_gated_sharded(icp_lib, m, p, dmax, world, 30, 1e-5)
    print("single", ref[1], "ranks", out[0][1])
    for res, errs, _scene, ktrace, _mask, k in out:  # identical decisions and solves on every rank
        np.testing.assert_array_equal(errs, out[0][1])
        np.testing.assert_array_equal(ktrace, out[0][3])
        np.testing.assert_array_equal(np.array(res.R), np.array(out[0][0].R))
        assert k == out[0][5]
    assert out[0][0].iterations == ref[0].iterations
    np.testing.assert_array_equal(out[0][3], ref[3])
    assert out[0][5] == ref[5]
    np.testing.assert_allclose(out[0][1], ref[1], rtol=1e-11)
    np.testing.assert_array_equal(np.concatenate([o[4] for o in out]), ref[4])
    np.testing.assert_allclose(np.concatenate([o[2] for o in out]), ref[2], atol=1e-12)


def test_rccl_single_rank_communicator(icp_lib, oracle, clump_single):
    """The 18-sum and the residual all-reduce through ncclAllReduce on a 1-rank communicator: the
    identity, so the run is the plain context's bit for bit."""
    amd = icp_lib
    m, p, dmax, _r = G.reference(oracle, ("clump",))
    ref = clump_single
    with amd.Context(0, amd.NN_CERTIFIED, rank=0, world_size=1, rccl_id=amd.rccl_unique_id()) as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(dmax)
        res, errs = ctx.run(30, 1e-5)
        mask, k = ctx.inliers()
        np.testing.assert_array_equal(ctx.inlier_trace(), ref[3])
        np.testing.assert_array_equal(ctx.get_scene(), ref[2])
    assert res.iterations == ref[0].iterations and k == ref[5]
    np.testing.assert_array_equal(errs, ref[1])
    np.testing.assert_array_equal(mask, ref[4])


# 8. CLI
def test_cli_max_dist(icp_lib, oracle, tmp_path):
    amd = icp_lib
    m, p, dmax, _r = G.reference(oracle, ("clump",))
    clump =str(tmp_path / "clump.txt")
    amd.write_matrix(clump, p)
    scene = amd.load_matrix(clump)  # the rounded cloud: the scene of both sides
    f = str(tmp_path / "f.txt")
    r = subprocess.run([os.path.join(BUILD, "icp-gpu"), datasets.path("cow_ref"), clump, "30", "--max-dist",
                        repr(float(dmax)), "--out", f], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:
        ctx.set_model(amd.load_matrix(datasets.path("cow_ref")))
        ctx.set_scene(scene)
        ctx.set_max_distance(dmax)
        res, _errs = ctx.run(30, 1e-5)
        g = str(tmp_path / "g.txt")
        amd.write_matrix(g, ctx.get_scene())
    assert res.converged == 1
    assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
    assert open(f, "rb").read() == open(g, "rb").read()


def test_index_digest_and_progress_under_the_gate(icp_lib, oracle):
    """The instrumentation the gated loop keeps: one index digest per search, and the progress
    callback once per recorded iteration, neither changing the run."""
    amd = icp_lib
    m, p, d, r = G.reference(oracle, ("bite", 257, 0.12))
    plain = run_gated(amd, m, p, d, G.BITES_ITERS, -1.0)
    seen = []
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_max_distance(d)
        ctx.set_index_digest(G.BITES_ITERS)
        ctx.set_progress(lambda i, e: seen.append((i, e)))
        res, errs = ctx.run(G.BITES_ITERS, -1.0)
        dig = ctx.index_digest()
        idx = ctx.get_indices().astype(np.uint64)
    np.testing.assert_array_equal(errs, plain[1])
    assert [i for i, _ in seen] == list(range(G.BITES_ITERS))
    np.testing.assert_array_equal([e for _, e in seen], errs)
    j = np.arange(idx.size, dtype=np.uint64)
    want = np.array([idx.sum(), ((j + np.uint64(1)) * idx).sum(), (idx == j).sum()], dtype=np.uint64)
    np.testing.assert_array_equal(dig[-1], want)  # (the last search's correspondences)
    assert np.all(dig[:, 0] > 0)
