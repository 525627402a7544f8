"""Global registration on the device (icp_global.hip: icp_fpfh, icp_match_features, icp_ransac_pose,
icp_global_pose) against tests/global_ref.py.

Descriptors: bit for bit on the rows the f1 filter keeps (every f1 the row depends on at least 1e-9 of a
bin from an edge; at most 1 % of a case's rows may be left out), with the normals the call itself
returns, which in turn are the model estimator's bits.  Matches: indices and distances exactly.  RANSAC:
every count inside the reference's bracket, -1 exactly where it rejects, the winner by the rule on the
returned counts.  The chain equals the public calls chained by hand, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import global_ref as G
import plane_ref as P

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def ctx(icp_lib):
    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as c:
        yield c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def descriptor(ctx, icp_lib, name):
    """(x, k, the device's (fpfh, spfh, normals), fpfh_ref with those normals): once, shared, never changed"""
    if name not in _REF:
        x, k = G.cloud(name, icp_lib.load_matrix)
        got = ctx.fpfh(x, k, k_normals=min(G.K_NORMALS, x.shape[0]), spfh=True, return_normals=True)
        _REF[name] = (x, k, got, G.fpfh_ref(x, got[2], k))
    return _REF[name]


@pytest.mark.parametrize("name", G.FPFH_CASES)
def test_descriptors_match_the_reference(ctx, icp_lib, name):
    x, k, (fpfh, spfh, nrm), ref = descriptor(ctx, icp_lib, name)
    ok_s, ok_f = ref["spfh_ok"], ref["fpfh_ok"]
    bad_s = (bits(spfh) != bits(ref["spfh"])).any(axis=1)
    bad_f = (bits(fpfh) != bits(ref["fpfh"])).any(axis=1)
    print(f"{name}: n {x.shape[0]}, k {k}, filter leaves out {int((~ok_f).sum())}, "
          f"SPFH rows differing {int((bad_s & ok_s).sum())}, FPFH rows differing {int((bad_f & ok_f).sum())}")
    assert (~ok_f).mean() <= G.FILTER_MAX
    assert not (bad_s & ok_s).any()
    assert not (bad_f & ok_f).any()
    if name == "line":  # zero normals: every row zero
        assert (nrm == 0.0).all() and (fpfh == 0.0).all() and (spfh == 0.0).all()


@pytest.mark.parametrize("name", ["ell257k32", "cow", "plane", "duplicates"])
def test_estimated_normals_are_the_model_estimators(ctx, icp_lib, name):
    x, k, (fpfh, _, nrm), _ = descriptor(ctx, icp_lib, name)
    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as fresh:
        fresh.set_model(x)
        fresh.estimate_model_normals(min(G.K_NORMALS, x.shape[0]))
        want = fresh.model_normals()
    assert np.array_equal(bits(nrm), bits(want))
    # given normals: the same descriptors as with the estimated ones
    assert np.array_equal(bits(ctx.fpfh(x, k, normals=nrm)), bits(fpfh))
    # a viewpoint changes signs only where the estimator's rule does
    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as fresh:
        fresh.set_model(x)
        fresh.estimate_model_normals(min(G.K_NORMALS, x.shape[0]), (0.0, 0.0, 10.0))
        want = fresh.model_normals()
    got = ctx.fpfh(x, k, k_normals=min(G.K_NORMALS, x.shape[0]), viewpoint=(0.0, 0.0, 10.0), return_normals=True)[1]
    assert np.array_equal(bits(got), bits(want))


def test_planar_lattice_with_equal_normals(ctx):
    """All normals equal: f1 = atan2(0, 1) = 0 for every pair, the middle bin of the first third."""
    x, k = G.cloud("plane")
    R = P.rot((1.0, -2.0, 0.5), 33.0)
    nrm = np.tile(R[:, 2], (x.shape[0], 1))
    fpfh, spfh = ctx.fpfh(x, k, normals=nrm, spfh=True)
    ref = G.fpfh_ref(x, nrm, k)
    assert ref["fpfh_ok"].all()
    assert np.array_equal(bits(spfh), bits(ref["spfh"])) and np.array_equal(bits(fpfh), bits(ref["fpfh"]))


@pytest.mark.parametrize("name", ["ell65k32", "ell4097k32", "cow", "duplicates"])
def test_two_calls_give_the_same_bits(ctx, icp_lib, name):
    x, k, (fpfh, spfh, nrm), _ = descriptor(ctx, icp_lib, name)
    again = ctx.fpfh(x, k, k_normals=min(G.K_NORMALS, x.shape[0]), spfh=True, return_normals=True)
    for a, b in zip((fpfh, spfh, nrm), again):
        assert np.array_equal(bits(a), bits(b))


def raw_fpfh(icp_lib, ctx, x, normals, k_normals, viewpoint, k, null_out=False):
    """icp_fpfh through ctypes with filled outputs -> (rc, the three outputs)"""
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    n = x.shape[0]
    outs = [np.full((max(n, 1), 33), -7.0), np.full((max(n, 1), 33), -7.0), np.full((max(n, 1), 3), -7.0)]
    rc = icp_lib.lib().icp_fpfh(ctx._h, dp(x), n, dp(normals), k_normals, dp(viewpoint), k,
                                None if null_out else dp(outs[0]), dp(outs[1]), dp(outs[2]))
    return rc, outs


def test_fpfh_errors_leave_the_outputs_untouched(ctx, icp_lib):
    x = np.ascontiguousarray(P.ellipsoid(40, 9)[0])
    nan_x = x.copy()
    nan_x[7, 1] = np.nan
    nan_n = np.ones_like(x)
    nan_n[3, 0] = np.inf
    cases = [(x, None, 16, None, 2, icp_lib.ICP_E_ARG), (x, None, 16, None, 65, icp_lib.ICP_E_ARG),
             (x, None, 16, None, 41, icp_lib.ICP_E_ARG), (x, None, 2, None, 8, icp_lib.ICP_E_ARG),
             (x, None, 41, None, 8, icp_lib.ICP_E_ARG), (x, None, 16, np.array([0.0, np.nan, 0.0]), 8, icp_lib.ICP_E_ARG),
             (x, nan_n, 16, None, 8, icp_lib.ICP_E_ARG), (nan_x, None, 16, None, 8, icp_lib.ICP_E_RANGE)]
    for xs, nr, kn, view, k, want in cases:
        rc, outs = raw_fpfh(icp_lib, ctx, xs, nr, kn, view, k)
        assert rc == want, (kn, k, rc)
        assert all((o == -7.0).all() for o in outs)
    assert raw_fpfh(icp_lib, ctx, x, None, 16, None, 8, null_out=True)[0] == icp_lib.ICP_E_ARG
    # given normals: k_normals is not looked at
    rc, outs = raw_fpfh(icp_lib, ctx, x, np.ascontiguousarray(P.ellipsoid(40, 9)[1]), 0, None, 8)
    assert rc == icp_lib.ICP_OK and np.isfinite(outs[0]).all() and (outs[2] != -7.0).all()


# ---- the feature match --------------------------------------------------------------------------

def features(n, seed):
    r = np.random.default_rng(seed)
    return np.round(r.uniform(0.0, 100.0, (n, G.DIM)), 1)  # (coarse values: equal distances do occur)


MATCH_SIZES = (1, 5, 63, 64, 65, 257)


@pytest.mark.parametrize("na", MATCH_SIZES)
def test_match_sizes(ctx, na):
    fa = features(na, 10 + na)
    for nb in MATCH_SIZES:
        fb = features(nb, 500 + nb)
        idx, d = ctx.match_features(fa, fb, distances=True)
        want, wd = G.match_ref(fa, fb)
        assert np.array_equal(idx, want) and np.array_equal(bits(d), bits(wd)), (na, nb)


def test_match_at_the_tile_and_the_range_sizes(ctx, icp_lib):
    """nb at the staged tile, at a range of several tiles and at the largest number of ranges, each +- 1."""
    tile, chunk, splits = icp_lib.match_plan(5, 8192)
    assert tile == 64 and chunk == 128 and splits == 64  # (the plan these sizes were chosen for)
    assert icp_lib.match_plan(5, 8193)[1:] == (192, 43)
    fa = features(5, 77)
    sizes = [tile - 1, tile, tile + 1, 2 * tile, 8191, 8192, 8193, 8192 + chunk - 1, 8192 + chunk, 8192 + chunk + 1]
    fb_all = features(max(sizes), 78)
    fb_all[-1] = fa[0]  # (the minimiser is the very last row of the largest)
    for nb in sizes:
        fb = fb_all[-nb:]
        idx, d = ctx.match_features(fa, fb, distances=True)
        want, wd = G.match_ref(fa, fb)
        assert np.array_equal(idx, want) and np.array_equal(bits(d), bits(wd)), nb
        assert idx[0] == nb - 1 and d[0] == 0.0
    # many queries: one range, several tiles
    assert icp_lib.match_plan(70000, 300)[1:] == (320, 1)


def test_match_real_descriptors_duplicates_nan_identity(ctx, icp_lib):
    m, p, _, _ = G.cow_pair(icp_lib.load_matrix)
    fm = ctx.fpfh(ctx.voxel_downsample(m, G.COW_VOXEL), 32)
    fp = ctx.fpfh(ctx.voxel_downsample(p, G.COW_VOXEL), 32)
    print(f"descriptors {fm.shape[0]} x {fp.shape[0]}")
    idx, d = ctx.match_features(fm, fp, distances=True)
    want, wd = G.match_ref(fm, fp)
    assert np.array_equal(idx, want) and np.array_equal(bits(d), bits(wd))
    # identical arrays: the identity (a row is its own first minimiser unless an earlier row equals it)
    same = ctx.match_features(fm, fm)
    assert np.array_equal(same, G.match_ref(fm, fm)[0])
    rows = features(300, 4)
    assert np.array_equal(ctx.match_features(rows, rows), np.arange(300))
    # duplicated rows of fb: the lowest index; a NaN row never wins; an all-NaN query gets -1
    fb = rows.copy()
    fb[[100, 200, 299]] = fb[7]
    fb[3, 5] = np.nan
    fa = np.concatenate([fb[[7, 100]], rows[[3]], np.full((1, G.DIM), np.nan)])
    idx, d = ctx.match_features(fa, fb, distances=True)
    assert idx[:2].tolist() == [7, 7] and idx[2] != 3 and idx[3] == -1 and np.isnan(d[3])
    want, wd = G.match_ref(fa, fb)
    assert np.array_equal(idx, want) and np.array_equal(bits(d), bits(wd))
    only_nan = np.full((2, G.DIM), np.nan)
    assert ctx.match_features(rows[:5], only_nan).tolist() == [-1] * 5


def test_match_errors(ctx, icp_lib):
    f = features(4, 1)
    ip = C.POINTER(C.c_int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    out = np.full(4, -7, dtype=np.int32)
    L = icp_lib.lib()
    assert L.icp_match_features(ctx._h, None, 4, dp(f), 4, out.ctypes.data_as(ip), None) == icp_lib.ICP_E_ARG
    assert L.icp_match_features(ctx._h, dp(f), 4, dp(f), 4, None, None) == icp_lib.ICP_E_ARG
    assert L.icp_match_features(ctx._h, dp(f), 0, dp(f), 4, out.ctypes.data_as(ip), None) == icp_lib.ICP_E_ARG
    assert L.icp_match_features(ctx._h, dp(f), 4, dp(f), 0, out.ctypes.data_as(ip), None) == icp_lib.ICP_E_ARG
    assert L.icp_match_features(ctx._h, dp(f), 4, dp(f), 2 ** 31, out.ctypes.data_as(ip), None) == icp_lib.ICP_E_ARG
    assert (out == -7).all()


# ---- RANSAC -------------------------------------------------------------------------------------

def check_winner(got):
    h, count = G.winner(got["counts"])
    assert (got["best_h"], got["inliers"]) == (h, count)
    assert got["evaluated"] == int((got["counts"] >= 0).sum())
    assert int(got["mask"].sum()) == got["inliers"]


@pytest.mark.parametrize("name", list(G.RANSAC_CASES))
def test_ransac_counts_lie_in_the_bracket(ctx, icp_lib, name):
    p, q, H, seed, max_dist, edge = G.ransac_case(name)
    ref = G.ransac_ref(p, q, H, seed, max_dist, edge, icp_lib.horn_solve)
    got = ctx.ransac_pose(p, q, H, seed, max_dist, edge, counts=True, mask=True)
    counts = got["counts"]
    print(f"{name}: kept {got['evaluated']} of {H}, bracket open for {ref['open']}, winner h {got['best_h']} "
          f"with {got['inliers']}")
    assert ref["open"] <= G.BRACKET_MAX * H
    assert np.array_equal(counts == -1, ~ref["kept"])
    assert ((counts >= ref["lo"]) & (counts <= ref["hi"])).all()
    check_winner(got)
    # two calls, and the mask: the same bits
    again = ctx.ransac_pose(p, q, H, seed, max_dist, edge, counts=True, mask=True)
    assert np.array_equal(bits(again["R"]), bits(got["R"])) and np.array_equal(bits(again["t"]), bits(got["t"]))
    assert np.array_equal(again["counts"], counts) and np.array_equal(again["mask"], got["mask"])


def test_ransac_h63_and_batches(ctx, icp_lib):
    """H = 63 is the first 63 of H = 64; H beyond a batch of 65,536 gives the counts of the batches' own runs."""
    p, q, _, seed, max_dist, edge = G.ransac_case("h64")
    a = ctx.ransac_pose(p, q, 63, seed, max_dist, edge, counts=True, mask=True)
    b = ctx.ransac_pose(p, q, 64, seed, max_dist, edge, counts=True, mask=True)
    assert np.array_equal(a["counts"], b["counts"][:63])
    check_winner(a)
    big = ctx.ransac_pose(p, q, 65536 + 65, seed, max_dist, edge, counts=True, mask=True)
    assert np.array_equal(big["counts"][:64], b["counts"])
    check_winner(big)
    ref = G.ransac_ref(p, q, 65536 + 65, seed, max_dist, edge, None)
    assert np.array_equal(big["counts"] == -1, ~ref["kept"])  # (the draw and the edge check past the first batch)


def test_ransac_planted_pose(ctx):
    p, q, R, t = G.planted()
    got = ctx.ransac_pose(p, q, 2000, 1, 1e-6, 0.9, counts=True, mask=True)
    assert got["inliers"] >= 120 and got["mask"][:120].all()
    assert np.abs(got["R"] - R).max() <= 1e-9 and np.abs(got["t"] - t).max() <= 1e-9
    check_winner(got)


def test_ransac_seeds_repeat(ctx):
    p, q, _, _, max_dist, edge = G.ransac_case("c65")
    runs = [ctx.ransac_pose(p, q, 500, s, max_dist, edge, counts=True) for s in (1, 2, 1, 2)]
    for a, b in ((0, 2), (1, 3)):
        assert np.array_equal(runs[a]["counts"], runs[b]["counts"])
        assert np.array_equal(bits(runs[a]["R"]), bits(runs[b]["R"])) and runs[a]["best_h"] == runs[b]["best_h"]
    assert not np.array_equal(runs[0]["counts"], runs[1]["counts"])


def test_ransac_errors(ctx, icp_lib):
    p, q, _, _ = G.planted()
    # triangles of very different size in p and q: every hypothesis is rejected
    with pytest.raises(icp_lib.ICPError) as e:
        ctx.ransac_pose(p, 3.0 * q, 200, 4, 0.1, 0.9)
    assert e.value.code == icp_lib.ICP_E_DEGENERATE and "200" in str(e.value) and "seed 4" in str(e.value)
    for kw in (dict(hypotheses=0), dict(hypotheses=2 ** 32), dict(max_dist=0.0), dict(max_dist=float("nan")),
               dict(edge_ratio=-0.1), dict(edge_ratio=1.5)):
        args = dict(hypotheses=10, seed=1, max_dist=0.1, edge_ratio=0.5)
        args.update(kw)
        with pytest.raises(icp_lib.ICPError) as e:
            ctx.ransac_pose(p, q, **args)
        assert e.value.code == icp_lib.ICP_E_ARG, kw
    with pytest.raises(icp_lib.ICPError) as e:
        ctx.ransac_pose(p[:2], q[:2], 10, 1, 0.1, 0.5)
    assert e.value.code == icp_lib.ICP_E_ARG


# ---- the chain, the purpose, off is off --------------------------------------------------------------

def test_global_pose_is_the_chain_by_hand(ctx, icp_lib):
    m, p, _, _ = G.cow_pair(icp_lib.load_matrix)
    for mutual in (True, False):
        R, t, rep = ctx.global_pose(m, p, G.COW_VOXEL, mutual=mutual, seed=G.PURPOSE_SEED, hypotheses=20000)
        mc, pc = ctx.voxel_downsample(m, G.COW_VOXEL), ctx.voxel_downsample(p, G.COW_VOXEL)
        fm, fp = ctx.fpfh(mc, 32, k_normals=16), ctx.fpfh(pc, 32, k_normals=16)
        pm = ctx.match_features(fp, fm)
        keep = G.mutual(pm, ctx.match_features(fm, fp)) if mutual else np.arange(pc.shape[0])
        got = ctx.ransac_pose(pc[keep], mc[pm[keep]], 20000, G.PURPOSE_SEED, 1.5 * G.COW_VOXEL, 0.9)
        assert np.array_equal(bits(R), bits(got["R"])) and np.array_equal(bits(t), bits(got["t"]))
        assert rep == {"model_points": mc.shape[0], "scene_points": pc.shape[0], "matches": keep.size,
                       "evaluated": got["evaluated"], "inliers": got["inliers"], "best_h": got["best_h"]}
    with pytest.raises(icp_lib.ICPError) as e:  # a level of fewer points than k
        ctx.global_pose(m, p, 2.0)
    assert e.value.code == icp_lib.ICP_E_TOO_FEW_POINTS
    with pytest.raises(icp_lib.ICPError) as e:
        ctx.global_pose(m, p, 0.0)
    assert e.value.code == icp_lib.ICP_E_ARG
    # a value a later call would refuse is refused before anything runs, as a bad argument
    for kw in (dict(k_normals=-1), dict(k_normals=2), dict(k_fpfh=-5), dict(k_fpfh=65), dict(hypotheses=-1),
               dict(hypotheses=2 ** 32), dict(max_dist=-0.1), dict(max_dist=float("inf")), dict(edge_ratio=-0.5),
               dict(edge_ratio=1.5)):
        with pytest.raises(icp_lib.ICPError) as e:
            ctx.global_pose(m, p, 2.0, **kw)  # (a voxel that would otherwise be ICP_E_TOO_FEW_POINTS)
        assert e.value.code == icp_lib.ICP_E_ARG and next(iter(kw)) in str(e.value), kw


def test_purpose_global_start_where_plain_icp_is_stuck(ctx, icp_lib):
    """The cow against itself turned 120 degrees about (1, 2, 3): 30 plain iterations stay far from the answer;
    the global pose (the defaults, the seed tests/test_global_ref.py checked) lands within 5 degrees and the
    same 30 iterations then reach it."""
    m, p, R_true, t_true = G.cow_pair(icp_lib.load_matrix)
    ctx.set_model(m)
    ctx.set_scene(p)
    plain, _ = ctx.run(30, -1.0)
    res, errs, total, (R0, t0), rep = icp_lib.register_global(ctx, m, p, G.COW_VOXEL, 30, -1.0, seed=G.PURPOSE_SEED)
    ang = G.angle_deg(R0, R_true)
    print(f"plain err {plain.err:.3e}; global {rep}, {ang:.3f} degrees, |dt| {np.abs(t0 - t_true).max():.4f}; "
          f"then err {res.err:.3e} after {res.iterations} iterations")
    assert plain.err > 1e-2
    assert ang < 5.0
    assert res.err < 1e-9
    assert G.angle_deg(total[1], R_true) < 1e-6


def test_off_is_off(ctx, icp_lib):
    """An icp_run after the four calls is bit-identical to that run on a fresh context."""
    m = icp_lib.load_matrix(__import__("datasets").path("cow_ref"))
    p = icp_lib.load_matrix(__import__("datasets").path("cow_tr2"))

    def run(c, between):
        c.set_model(m)
        c.set_scene(p)
        between(c)
        res, errs = c.run(12, -1.0)
        return errs, c.get_scene(), c.transform()

    def calls(c):
        f = c.fpfh(p[:500], 16)
        c.match_features(f, f[:100])
        pp, qq, _, _ = G.planted()
        c.ransac_pose(pp, qq, 300, 1, 0.01, 0.9)
        c.global_pose(m, p, G.COW_VOXEL, hypotheses=2000)

    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as fresh:
        want = run(fresh, lambda c: None)
    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as other:
        got = run(other, calls)
    assert np.array_equal(bits(want[0]), bits(got[0])) and np.array_equal(bits(want[1]), bits(got[1]))
    assert np.array_equal(bits(want[2][1]), bits(got[2][1])) and np.array_equal(bits(want[2][2]), bits(got[2][2]))
