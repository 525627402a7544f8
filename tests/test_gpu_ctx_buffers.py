"""The context's resident memory (engine::DevBuf / HostBuf, icp_engine.h): every block a context or a call
obtains is a member that frees itself, and icp_debug_live_buffers counts the blocks held, process-wide.

Every case reads the count first (not zero: other fixtures of the session may hold contexts) and ends with
the count back at that baseline once its last context is destroyed; the cases that reuse, re-grow or swap
buffers also compare what they compute, bit for bit, with the same steps on a fresh context.
"""
import gc

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import filter_ref as F
import kept_ref as KR

pytestmark = pytest.mark.gpu

NBIG = 65600  # above the 65,536 points up to which the context keeps the model's host copy
NB = 8192  # kBundleMinModel: the smallest model with the bundle images and the kd scratch
NSLOT = 262144  # the smallest scene icp_run keeps in slot order over a model of NB points (NSLOT x NB = 2^31)
KEPT_CELL = ("plane", True, True, "huber", True)  # the gate, the trim, Huber weights and one-to-one together


@pytest.fixture()
def live(icp_lib):
    """-> the count's reader; after the test, the count is back at what it was before it."""
    gc.collect()  # (a context an earlier test dropped without closing it goes now, not in the middle of this one)
    base = icp_lib.debug_live_buffers()
    print("baseline", base)
    assert base >= 0
    yield icp_lib.debug_live_buffers
    assert icp_lib.debug_live_buffers() == base


def test_model_with_bundle_images(icp_lib, live):
    """A model of kBundleMinModel points: the bundle images and the kd scratch (icp_get_model_order forces
    them), icp_ensure_model twice, a run.  Before the owning types this sequence left four blocks behind at
    icp_ctx_destroy -- mstat_part, mstat_out, h_mstat and kd_scratch were allocated and never freed.  The
    fifth, cmp_diff, is icp_ensure_model's compare counter for a model too large for the kept host copy (at
    8192 points the call compares on the host): the model of NBIG points, ensured twice, allocates it."""
    base = live()
    m, p = icp_lib.synthetic_pair(NB, seed=11)
    with icp_lib.Context() as c:
        c.set_model(m)
        kd = c.model_order(NB)
        assert np.array_equal(np.sort(kd), np.arange(NB))
        assert c.ensure_model(m) is False and c.ensure_model(m) is False
        c.set_scene(p)
        res, errs = c.run(3, -1.0)
        assert res.iterations == 3 and np.isfinite(errs).all()
        big, _ = icp_lib.synthetic_pair(NBIG, seed=13)
        assert c.ensure_model(big) is True
        before = live()
        assert c.ensure_model(big) is False  # (compared on the device)
        assert live() == before + 1  # (the compare counter)
        held = live() - base
        print("blocks held by the context", held)
        assert held > 0


def test_one_launch_pair(icp_lib, live):
    m, p = icp_lib.synthetic_pair(64, seed=12)
    with icp_lib.Context() as c:
        c.set_run_mode(icp_lib.RUN_PERSISTENT)
        c.set_model(m)
        c.set_scene(p)
        res, errs = c.run(5, -1.0)
        assert res.iterations == 5 and c.stats()["persistent_runs"] == 1 and np.isfinite(errs).all()


def kept_context(amd, n):
    m, nrm, p, _ = KR.matrix_case(n)
    opt = KR.cell_options(KEPT_CELL, n)
    c = amd.Context()
    c.set_model(m)
    c.set_model_normals(nrm)
    c.set_metric(amd.METRIC_POINT_TO_PLANE)
    c.set_scene(p)
    c.set_max_distance(opt["dmax"])
    c.set_trim(opt["trim"])
    c.set_robust(amd.ROBUST_HUBER, opt["robust"][1])
    c.set_one_to_one(opt["one_to_one"])
    return c, p


def kept_run(amd, c, max_iter):
    res, errs = c.run(max_iter, -1.0)
    (w, kpos), (_mask, k) = c.robust_trace(), c.inliers()
    return dict(iterations=res.iterations, errs=errs, K=c.inlier_trace(), C=c.trim_trace(), W=w, Kpos=kpos, k=k,
                scene=c.get_scene())


def test_kept_traces_regrow(icp_lib, live):
    """One kept-pairs run with every option at 257 points and max_iter 4 (every mapped trace at its first 64
    entries), then the same scene again with max_iter 200 on the same context: every trace re-grows, and
    holds what a fresh context's run of 200 holds."""
    n = 257
    c, p = kept_context(icp_lib, n)
    with c:
        first = kept_run(icp_lib, c, 4)
        held = live()
        c.set_scene(p)  # (the run moved the scene: the second starts where the fresh context's starts)
        again = kept_run(icp_lib, c, 200)
        assert live() == held  # (each trace's block replaced, none added)
    c, _ = kept_context(icp_lib, n)
    with c:
        fresh = kept_run(icp_lib, c, 200)
    print("iterations", first["iterations"], again["iterations"], fresh["iterations"], "K", fresh["K"][-3:])
    assert first["iterations"] == 4 and len(first["K"]) == 4 and fresh["iterations"] > 64
    for key, want in fresh.items():
        got, want = np.asarray(again[key]), np.asarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), key


def test_filter_evaluate_voxel_on_one_context(icp_lib, live):
    """The two kept blocks (the filters', the evaluation's) and the voxel scratch on one context."""
    x = F.cloud("ell257")
    with icp_lib.Context() as c:
        before = live()
        kept = c.filter_statistical(x, 16, 2.0)
        assert 0 < len(kept) <= 257
        c.set_allow_unequal(True)
        c.set_model(x)
        c.set_scene(kept)
        ev = c.evaluate(float("inf"), both=True)
        assert ev["correspondences"] == len(kept) and ev["inlier_rmse"] == 0.0 and ev["model_points"] == 257
        vox = c.voxel_downsample(x, 0.25 * float(np.ptp(x, axis=0).max()))
        assert 0 < len(vox) < 257
        assert live() > before


def registration(amd, m, p, iters):
    """-> (errs, scene, indices) of icp_run on a context of its own: the model first, so the scene of NSLOT
    points is sorted into slot order while it is uploaded and no buffer is ever swapped."""
    with amd.Context() as c:
        c.set_allow_unequal(True)
        c.set_model(m)
        c.set_scene(p)
        _, errs = c.run(iters, -1.0)
        return errs, c.get_scene(), c.get_indices()


def probe_adds(live, c):
    """The blocks icp_get_indices adds: for a scene in slot order it permutes idx into s_tmp_idx, which it
    allocates unless scene_to_slot_order has already swapped a block into it."""
    before = live()
    idx = c.get_indices()
    return live() - before, idx


def test_swaps(icp_lib, live):
    """scene with s_tmp, idx with s_tmp_idx, model with model_alt and m4 with m4_alt, each against a reference
    that swaps nothing (registration).  The scene is set BEFORE the model, so it is uploaded in file order; a
    gated run (the kept-pairs loop reorders nothing) leaves correspondences over it; the ungated run that
    follows then moves the scene AND idx into slot order through their second buffers (scene_to_slot_order
    with its indices).  That this happened is read from the state: icp_get_indices then finds s_tmp_idx
    allocated (the swap left idx's old block there), while on the control context -- the model first, the
    scene in slot order from its upload, the same sizes -- it has to allocate it."""
    amd = icp_lib
    m1, _ = amd.synthetic_pair(NB, seed=21)
    m2, _ = amd.synthetic_pair(NB, seed=22)
    _, p = amd.synthetic_pair(NSLOT, seed=23)
    with amd.Context() as ctl:  # the control: slot order without a swap
        ctl.set_allow_unequal(True)
        ctl.set_model(m1)
        ctl.set_scene(p)
        ctl.set_max_distance(1e30)
        ctl.run(2, -1.0)
        ctl.set_max_distance(0.0)
        ctl.run(0, -1.0)
        ctl_adds, _ = probe_adds(live, ctl)
    with amd.Context() as c:
        c.set_allow_unequal(True)
        c.set_scene(p)
        c.set_model(m1)
        c.set_max_distance(1e30)
        c.run(2, -1.0)
        c.set_max_distance(0.0)
        scene_a, idx_a = c.get_scene(), c.get_indices()  # (file order on the device: nothing permuted, nothing allocated)
        res, _ = c.run(0, -1.0)  # (the set-up alone: the scene and idx into slot order)
        adds, idx_0 = probe_adds(live, c)
        print("icp_get_indices added", adds, "block(s); on the control", ctl_adds)
        assert res.iterations == 0 and ctl_adds == 1 and adds == 0
        assert np.array_equal(idx_0, idx_a) and np.array_equal(c.get_scene(), scene_a)
        _, e1 = c.run(3, -1.0)
        scene_b, idx_b = c.get_scene(), c.get_indices()
        c.set_model(m2)  # (model with model_alt, m4 with m4_alt; the scene to go back into file order)
        _, e2 = c.run(3, -1.0)  # (back through s_tmp, and into the new model's slot order)
        scene_c, idx_c = c.get_scene(), c.get_indices()
    for tag, got, want in (("m1", (e1, scene_b, idx_b), registration(amd, m1, scene_a, 3)),
                           ("m2", (e2, scene_c, idx_c), registration(amd, m2, scene_b, 3))):
        print(tag, "errs", got[0], "reference", want[0])
        assert len(got[0]) == 3
        for what, g, w in zip(("errs", "scene", "indices"), got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (tag, what)


@pytest.mark.parametrize("reverse", [False, True], ids=["creation-order", "reverse-order"])
def test_two_contexts(icp_lib, live, reverse):
    m, p = icp_lib.synthetic_pair(64, seed=31)

    def create_and_use():
        c = icp_lib.Context()
        c.set_model(m)
        c.set_scene(p)
        c.run(3, -1.0)
        return c

    base = live()
    a = create_and_use()
    held_a = live() - base
    b = create_and_use()
    held_b = live() - base - held_a
    print("held", held_a, held_b)
    assert held_a > 0 and held_b > 0
    first, second, held_second = (b, a, held_a) if reverse else (a, b, held_b)
    first.close()
    assert live() == base + held_second
    res, _ = second.run(2, -1.0)  # (the other context's memory is its own)
    assert res.iterations == 2
    second.close()
    assert live() == base
