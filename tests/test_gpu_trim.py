"""icp_run with a trimmed fraction (icp_set_trim, icp_select.hip) against tests/trim_ref.py, the
trimmed loop restated with the oracle's pieces.

Tolerances are the gate tests' (test_gpu_gated.py check_against_ref): K per iteration and the masks
exact, err rel 1e-9, s and R abs 1e-9, new_p abs 1e-9 x extent; the C trace rel 1e-9.  The first
iteration's d2 has the oracle's bits, so its C is compared as uint64; later iterations rest on the
reference's margin (tests/test_trim_ref.py: > 1e-6 for every case used here).
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import datasets
import gated_ref as G
import plane_ref as P
import robust_ref as RR
import trim_ref as TR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


class HostAllReduce:
    """The host all-reduce of W ranks run as W threads (the pattern of test_gpu_gated.py)."""

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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_trim(amd, m, p, f, dmax, iters, threshold, mode=0, variant=None, prepare=None, **ctx_args):
    """-> (res, errs, scene, K trace, mask, K last, C trace) of a fresh context."""
    with amd.Context(0, mode, **ctx_args) as ctx:
        if variant is not None:
            ctx.set_nn_variant(variant)
        ctx.set_model(m)
        ctx.set_scene(p)
        if prepare is not None:
            prepare(ctx)
        if f is not None:
            ctx.set_trim(f)
        if dmax:
            ctx.set_max_distance(dmax)
        res, errs = ctx.run(iters, threshold)
        mask, k = ctx.inliers()
        return res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, k, (ctx.trim_trace() if f is not None else None)


def check_against_ref(m, out, r):
    res, errs, scene, ktrace, mask, k, ctrace = out
    print("K", list(ktrace), "C", list(ctrace), "ref C", r["C"], "err", errs, "ref err", r["err"])
    assert res.iterations == r["iterations"]
    assert list(ktrace) == r["K"] and k == r["K"][-1]
    np.testing.assert_array_equal(mask, r["mask"])
    np.testing.assert_allclose(ctrace, r["C"], rtol=1e-9)
    np.testing.assert_allclose(errs, r["err"], rtol=1e-9)
    assert abs(res.s - r["s"]) <= 1e-9
    np.testing.assert_allclose(np.array(res.R).reshape(3, 3), r["R"], atol=1e-9)
    extent = float(np.abs(m).max())
    np.testing.assert_allclose(np.array(res.t), r["t"], atol=1e-9 * extent)
    np.testing.assert_allclose(scene, r["new_p"], atol=1e-9 * extent)


def key_id(key):
    return "-".join(str(k) for k in key)


# 1. one iteration, exact: the first iteration's d2 has the oracle's bits, so no margin is needed
@pytest.mark.parametrize("key", TR.MULTI, ids=key_id)
def test_one_iteration_exact(icp_lib, oracle, key):
    m, p, f, dmax, _it, _th, r = TR.reference(oracle, key, iters=1)
    out = run_trim(icp_lib, m, p, f, dmax, 1, -1.0)
    assert bits(out[6])[0] == bits(r["C"])[0], (out[6], r["C"])
    check_against_ref(m, out, r)
    if dmax == 0.0 or r["C"][0] <= dmax * dmax:  # the trim binds
        assert out[5] >= r["T"]


# 2. ties at the cut are all kept
def test_ties_are_kept_whole(icp_lib, oracle):
    m, p = G.synth(257, 357, 0.25)
    p2 = np.repeat(p, 2, axis=0)
    for f, T, K in ((0.5, 257, 258), (0.4987, 256, 256)):
        r = TR.trimmed_ref(oracle, m, p2, f, 0.0, 1, -1.0)
        assert (r["T"], r["K"]) == (T, [K])
        with icp_lib.Context() as ctx:
            ctx.set_allow_unequal(True)
            ctx.set_model(m)
            ctx.set_scene(p2)
            ctx.set_trim(f)
            res, errs = ctx.run(1, -1.0)
            mask, k = ctx.inliers()
            out = (res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, k, ctx.trim_trace())
        assert bits(out[6])[0] == bits(r["C"])[0]
        check_against_ref(m, out, r)
        np.testing.assert_array_equal(mask[0::2], mask[1::2])  # a pair of twins is kept or dropped whole


# 3. several iterations
@pytest.mark.parametrize("key", TR.MULTI, ids=key_id)
def test_several_iterations(icp_lib, oracle, key):
    m, p, f, dmax, iters, threshold, r = TR.reference(oracle, key)
    assert r["margin"] > 1e-6
    out = run_trim(icp_lib, m, p, f, dmax, iters, threshold)
    check_against_ref(m, out, r)


# 4. too few: T = 3 < 4 stops the run before anything changes
def test_too_few_stops_before_the_iteration(icp_lib):
    amd = icp_lib
    m, p = G.synth(5, 105, 0.25)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_trim(TR.SIZES_F)
        with pytest.raises(amd.ICPError) as ei:
            ctx.run(TR.SIZES_ITERS, -1.0)
        assert ei.value.code == amd.ICP_E_TOO_FEW_POINTS
        print(str(ei.value))
        assert "iteration 0" in str(ei.value) and "T = 3" in str(ei.value) and "K = 3" in str(ei.value)
        assert bits(ctx.get_scene()).tolist() == bits(p).tolist()
        mask, k = ctx.inliers()
        assert k == 3 and mask.sum() == 3
        assert ctx.inlier_trace().size == 0 and ctx.trim_trace().size == 0


# 5. off is off
def plain_run(amd, m, p, iters):
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        res, errs = ctx.run(iters, -1.0)
        return errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t)


def test_off_is_off(icp_lib, oracle):
    amd = icp_lib
    m, p, _f, _d, _it, _th, _r = TR.reference(oracle, ("size", 4097))
    plain = plain_run(amd, m, p, 5)
    with amd.Context() as ctx:  # (a) the default, set explicitly
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_trim(1.0)
        res, errs = ctx.run(5, -1.0)
        with pytest.raises(amd.ICPError) as ei:  # no trimmed run: nothing to report
            ctx.trim_trace()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        with pytest.raises(amd.ICPError) as ei:
            ctx.inliers()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        one = (errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t))
    for a, b in zip(plain, one):
        np.testing.assert_array_equal(a, b)
    cm, cp, cf, _cd, _ci, _ct, _cr = TR.reference(oracle, ("clump",))
    with amd.Context() as ctx:  # (b) a trimmed run, then the trim switched off
        ctx.set_model(cm)
        ctx.set_scene(cp)
        ctx.set_trim(cf)
        ctx.run(3, -1.0)
        mid = ctx.get_scene()
        ctx.set_trim(1.0)
        res, errs = ctx.run(5, -1.0)
        two = (errs, ctx.get_scene(), np.array(res.R), res.s, np.array(res.t))
        assert ctx.trim_trace().size == 3  # (still the trimmed run's: no new scene since)
    for a, b in zip(plain_run(amd, cm, mid, 5), two):
        np.testing.assert_array_equal(a, b)
    # (c) T = n - 1 is a trim: the farthest pair leaves the sums
    assert TR.trim_count(0.999999, 4097) == 4096
    out = run_trim(amd, m, p, 0.999999, 0.0, 5, -1.0)
    assert list(out[3]) == [4096] * 5
    assert not np.array_equal(out[1], plain[0])


# 6. combinations at n = 4097.  A trimmed iteration is the gated iteration whose D is min(D, C): on
# one pose, a gated run whose dmax * dmax lies between C and the next distance keeps the same pairs
# and runs the same kernels, so the two agree bit for bit.  Each step runs one iteration on both
# contexts, the gate taken from the C the trimmed one reports.
def step_against_gate(amd, m, p, f, prepare, steps=3):
    with amd.Context() as a, amd.Context() as b:
        for ctx in (a, b):
            ctx.set_model(m)
            ctx.set_scene(p)
            prepare(ctx)
        a.set_trim(f)
        T = TR.trim_count(f, p.shape[0])
        for s in range(steps):
            res_a, errs_a = a.run(1, -1.0)
            C = a.trim_trace()[0]
            b.set_max_distance(np.sqrt(C) * (1.0 + 1e-9))
            res_b, errs_b = b.run(1, -1.0)
            (mask_a, ka), (mask_b, kb) = a.inliers(), b.inliers()
            print("step", s, "C", C, "K", ka, kb, "err", errs_a, errs_b)
            assert ka == kb == T
            np.testing.assert_array_equal(mask_a, mask_b)
            np.testing.assert_array_equal(errs_a, errs_b)
            np.testing.assert_array_equal(a.get_scene(), b.get_scene())
            np.testing.assert_array_equal(np.array(res_a.R), np.array(res_b.R))
        return a.get_scene()


def test_point_to_plane_with_estimated_normals(icp_lib):
    amd = icp_lib
    m, _nrm, p = P.gate_case(4097)

    def prepare(ctx):
        assert ctx.estimate_model_normals(16) == 0
        ctx.set_metric(amd.METRIC_POINT_TO_PLANE)

    step_against_gate(amd, m, p, 0.7, prepare)
    # and a whole run: every iteration keeps T pairs, none of the far quarter at the end
    out = run_trim(amd, m, p, 0.7, 0.0, 8, -1.0, prepare=prepare)
    print("K", list(out[3]), "C", list(out[6]), "err", out[1])
    assert list(out[3]) == [TR.trim_count(0.7, 4097)] * 8
    far = p[:, 0] > 2.0
    assert far.sum() == 4097 // 4 and not out[4][far].any()
    assert out[6][-1] < out[6][0] and out[1][-1] < out[1][0]


def test_tukey_weights_inside_the_trim(icp_lib):
    amd = icp_lib
    m, _nrm, p = P.gate_case(4097)
    k = RR.k_of("point", RR.TUKEY, 4097)

    def prepare(ctx):
        ctx.set_robust(amd.ROBUST_TUKEY, k)

    step_against_gate(amd, m, p, 0.7, prepare)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        prepare(ctx)
        ctx.set_trim(0.7)
        res, errs = ctx.run(8, -1.0)
        w, kpos = ctx.robust_trace()
        ktrace = ctx.inlier_trace()
    print("K", list(ktrace), "W", list(w), "K+", list(kpos))
    T = TR.trim_count(0.7, 4097)
    assert list(ktrace) == [T] * 8
    assert np.all(kpos <= T) and np.all(kpos >= 4) and np.all(w <= kpos)  # the weights apply to the kept pairs


def test_trimmed_run_on_a_scene_in_slot_order(icp_lib):
    """Two ungated iterations at 65,536 points leave the scene in slot order; three trimmed
    iterations on that context against three on a fresh context given the same scene (file order).
    The two runs sum in different orders, so their scenes differ by rounding: K, the mask (the
    caller's order) and the first C are compared exactly (test_gpu_gated.py's case b)."""
    amd = icp_lib
    n = 65536
    m, p = amd.synthetic_pair(n)
    r = np.random.default_rng(5)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    f = 0.6
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(2, -1.0)
        mid = ctx.get_scene()
        ctx.set_trim(f)
        res_a, errs_a = ctx.run(3, -1.0)
        ka, (mask_a, cnt_a), scene_a, ca = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene(), ctx.trim_trace()
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(mid)
        ctx.set_trim(f)
        res_b, errs_b = ctx.run(3, -1.0)
        kb, (mask_b, cnt_b), scene_b, cb = ctx.inlier_trace(), ctx.inliers(), ctx.get_scene(), ctx.trim_trace()
    print("K", list(ka), list(kb), "C", list(ca), list(cb), "err", errs_a, errs_b)
    assert res_a.iterations == res_b.iterations == 3
    T = TR.trim_count(f, n)
    assert list(ka) == list(kb) == [T] * 3 and cnt_a == cnt_b == T
    np.testing.assert_array_equal(mask_a, mask_b)
    assert mask_a.sum() == T
    assert bits(ca)[0] == bits(cb)[0]
    np.testing.assert_allclose(ca, cb, rtol=1e-11)
    np.testing.assert_allclose(errs_a, errs_b, rtol=1e-11)
    np.testing.assert_allclose(scene_a, scene_b, atol=1e-12)


def test_variants_bitwise_at_4097(icp_lib, oracle):
    """The indices are the same whatever searches, and neither the selection nor the kept-pairs
    kernels depend on the variant."""
    amd = icp_lib
    m, p, f, dmax, iters, th, _r = TR.reference(oracle, ("size", 4097))
    a = run_trim(amd, m, p, f, dmax, iters, th)
    for mode, variant in ((amd.NN_FP64, None), (amd.NN_CERTIFIED, amd.VARIANT_VALU), (amd.NN_CERTIFIED, amd.VARIANT_MFMA),
                          (amd.NN_CERTIFIED, amd.VARIANT_MFMA16), (amd.NN_CERTIFIED, amd.VARIANT_GRID),
                          (amd.NN_CERTIFIED, amd.VARIANT_BUNDLE)):
        b = run_trim(amd, m, p, f, dmax, iters, th, mode=mode, variant=variant)
        for j in (1, 2, 3, 4, 6):
            np.testing.assert_array_equal(b[j], a[j])


# 7. ranks
@pytest.fixture(scope="module")
def clump_single(icp_lib, oracle):
    m, p, f, dmax, iters, th, _r = TR.reference(oracle, ("clump",))
    return run_trim(icp_lib, m, p, f, dmax, iters, th)


def run_trim_sharded(amd, m, p, f, world, iters, threshold):
    red = HostAllReduce(world)
    results = [None] * world
    errors = []

    def worker(r):
        try:
            b, c = amd.shard_range(p.shape[0], r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                ctx.set_model(m)
                ctx.set_scene(p[b:b + c], np_total=p.shape[0])
                ctx.set_trim(f)
                res, errs = ctx.run(iters, threshold)
                mask, k = ctx.inliers()
                results[r] = (res, errs, ctx.get_scene(), ctx.inlier_trace(), mask, k, ctx.trim_trace())
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
    m, p, f, _dmax, iters, th, _r = TR.reference(oracle, ("clump",))
    ref = clump_single
    out = run_trim_sharded(icp_lib, m, p, f, world, iters, th)
    print("single K", list(ref[3]), "C", list(ref[6]), "ranks C", list(out[0][6]))
    for res, errs, _scene, ktrace, _mask, k, ctrace in out:  # identical decisions and solves on every rank
        np.testing.assert_array_equal(errs, out[0][1])
        np.testing.assert_array_equal(ktrace, out[0][3])
        np.testing.assert_array_equal(bits(ctrace), bits(out[0][6]))  # every rank reports the same bits
        np.testing.assert_array_equal(np.array(res.R), np.array(out[0][0].R))
        assert k == out[0][5]
    assert out[0][0].iterations == ref[0].iterations
    np.testing.assert_array_equal(out[0][3], ref[3])
    assert out[0][5] == ref[5]
    # the ranks' sums fold in another order than one rank's, so the scenes part in the last bits
    # after the first iteration: its C has the same bits, the later ones the traces' tolerance
    assert bits(out[0][6])[0] == bits(ref[6])[0]
    np.testing.assert_allclose(out[0][6], ref[6], rtol=1e-9)
    np.testing.assert_allclose(out[0][1][:-1], ref[1][:-1], rtol=1e-9)
    assert out[0][1][-1] < 1e-5
    np.testing.assert_array_equal(np.concatenate([o[4] for o in out]), ref[4])
    np.testing.assert_allclose(np.concatenate([o[2] for o in out]), ref[2], atol=1e-12)


def test_rccl_single_rank_communicator(icp_lib, oracle, clump_single):
    """Every pass's bins, the sums and the residual all-reduce through ncclAllReduce on a 1-rank
    communicator: the identity, so the run is the plain context's bit for bit."""
    amd = icp_lib
    m, p, f, dmax, iters, th, _r = TR.reference(oracle, ("clump",))
    ref = clump_single
    out = run_trim(amd, m, p, f, dmax, iters, th, mode=amd.NN_CERTIFIED, rank=0, world_size=1, rccl_id=amd.rccl_unique_id())
    assert out[0].iterations == ref[0].iterations and out[5] == ref[5]
    for j in (1, 2, 3, 4):
        np.testing.assert_array_equal(out[j], ref[j])
    np.testing.assert_array_equal(bits(out[6]), bits(ref[6]))


# 8. CLI
def test_cli_trim(icp_lib, oracle, tmp_path):
    amd = icp_lib
    m, p, f, _dmax, iters, th, _r = TR.reference(oracle, ("clump",))
    clump = str(tmp_path / "clump.txt")
    amd.write_matrix(clump, p)
    scene = amd.load_matrix(clump)  # the rounded cloud: the scene of both sides
    out_f = str(tmp_path / "f.txt")
    r = subprocess.run([os.path.join(BUILD, "icp-gpu"), datasets.path("cow_ref"), clump, str(iters), "--trim", repr(f),
                        "--out", out_f], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with amd.Context() as ctx:
        ctx.set_model(amd.load_matrix(datasets.path("cow_ref")))
        ctx.set_scene(scene)
        ctx.set_trim(f)
        res, _errs = ctx.run(iters, th)
        g = str(tmp_path / "g.txt")
        amd.write_matrix(g, ctx.get_scene())
    assert res.converged == 1
    assert len([l for l in r.stderr.splitlines() if l.startswith("[ICP]")]) == res.iterations
    assert open(out_f, "rb").read() == open(g, "rb").read()
    bad = subprocess.run([os.path.join(BUILD, "icp-gpu"), datasets.path("cow_ref"), clump, "3", "--trim", "1.5"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--trim" in bad.stderr


# 9. argument errors leave the earlier setting
def test_argument_errors(icp_lib, oracle):
    amd = icp_lib
    m, p, f, _d, _it, _th, r = TR.reference(oracle, ("size", 257), iters=1)
    with amd.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_trim(f)
        for bad in (0.0, -0.1, 1.5, np.nan):
            with pytest.raises(amd.ICPError) as ei:
                ctx.set_trim(bad)
            assert ei.value.code == amd.ICP_E_ARG
        ctx.run(1, -1.0)
        assert list(ctx.inlier_trace()) == r["K"]  # (the fraction set before the refused ones)
        assert bits(ctx.trim_trace())[0] == bits(r["C"])[0]
        # the setting survives icp_set_scene / icp_set_model, the traces do not
        ctx.set_model(m)
        ctx.set_scene(p)
        with pytest.raises(amd.ICPError) as ei:
            ctx.trim_trace()
        assert ei.value.code == amd.ICP_E_NO_MODEL
        ctx.run(1, -1.0)
        assert list(ctx.inlier_trace()) == r["K"]
