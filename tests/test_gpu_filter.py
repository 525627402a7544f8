"""Outlier removal on the device (icp_filter_statistical, icp_filter_radius and their device forms;
icp_filter.hip) against tests/filter_ref.py, the header's rules restated in numpy.

Statistical: the mask, n_out and the kept points are compared exactly (tests/test_filter_ref.py keeps
every case's means at least 1e-9 of T away from T).  mean_dist is within (k + 3) 2^-52 relative of the
reference: each of the k + 1 roots is at most 1 ulp off if the device's root is not correctly rounded,
and each of the k + 1 additions rounds a non-negative partial sum by at most 1/2 ulp.  mu, sigma and T
are within 1e-12 relative: a sum of n <= 9,001 non-negative terms in any order is within n 2^-53 of the
exact one.  Radius: the counts are integers and are compared exactly.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import datasets
import filter_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "iterative-closest-point_amd", "build")


@pytest.fixture(scope="module")
def ctx(icp_lib):
    with icp_lib.Context() as c:
        yield c


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# 1. the statistical filter
@pytest.mark.parametrize("name", F.CASES)
def test_statistical(ctx, oracle, name):
    for k, ratio in F.STAT_PARAMS[name]:
        m, r = F.reference("stat", name, (k, ratio), oracle.load_matrix)
        out, mask, mean, stats = ctx.filter_statistical(m, k, ratio, mask=True, mean_dist=True, stats=True)
        only = ctx.filter_statistical(m, k, ratio)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(r["mean"] > 0, np.abs(mean - r["mean"]) / r["mean"], np.abs(mean))
        print(name, "n", m.shape[0], "k", k, "ratio", ratio, "kept", out.shape[0], "of which the reference keeps",
              int(r["mask"].sum()), "mean_dist bit-equal:", bool(np.array_equal(mean, r["mean"])), "largest rel. error",
              err.max(), "mu sigma T rel.", rel(stats[0], r["mu"]), rel(stats[1], r["sigma"]), rel(stats[2], r["T"]))
        assert mask.dtype == np.uint8 and mask.shape == (m.shape[0],)
        np.testing.assert_array_equal(mask.astype(bool), r["mask"])
        assert out.shape[0] == int(r["mask"].sum())
        np.testing.assert_array_equal(out, m[r["mask"]])
        np.testing.assert_array_equal(only, out)
        assert np.all(err <= (k + 3) * 2.0 ** -52)
        assert rel(stats[0], r["mu"]) <= 1e-12 and rel(stats[1], r["sigma"]) <= 1e-12 and rel(stats[2], r["T"]) <= 1e-12


# 2. the radius filter
@pytest.mark.parametrize("name", F.CASES)
def test_radius(ctx, oracle, name):
    m = F.cloud(name, oracle.load_matrix)
    for radius, min_nb in F.radius_params(name, m):
        _, c = F.reference("radius", name, radius, oracle.load_matrix)
        out, mask, counts = ctx.filter_radius(m, radius, min_nb, mask=True, counts=True)
        out2, mask2 = ctx.filter_radius(m, radius, min_nb, mask=True)  # (the scan may stop early)
        keep = c > min_nb
        print(name, "n", m.shape[0], "radius", radius, "min_neighbors", min_nb, "counts that differ",
              int((counts != c).sum()), "kept", out.shape[0], "reference", int(keep.sum()))
        assert counts.dtype == np.int32
        np.testing.assert_array_equal(counts, c)
        np.testing.assert_array_equal(mask.astype(bool), keep)
        np.testing.assert_array_equal(mask2, mask)
        np.testing.assert_array_equal(out, m[keep])
        np.testing.assert_array_equal(out2, out)
    if name == "ell257":
        assert np.all(c == 257)  # (the last radius is the diameter)


# 3. edges
def test_edges(ctx, oracle):
    m17 = F.cloud("ell17")  # n = k + 1: every list is the whole cloud
    out, mask = ctx.filter_statistical(m17, 16, 2.0, mask=True)
    _, r = F.reference("stat", "ell17", (16, 2.0))
    np.testing.assert_array_equal(mask.astype(bool), r["mask"])
    m = F.cloud("ell257")
    out, mask, stats = ctx.filter_statistical(m, 8, 0.0, mask=True, stats=True)  # T = mu
    assert stats[2] == stats[0] and 0 < out.shape[0] < 257
    out = ctx.filter_statistical(m, 16, 1e6)  # everything kept
    np.testing.assert_array_equal(out, m)
    for min_nb in (257, 258, 2 ** 31 - 1):  # min_neighbors >= n: nothing kept, and that is ICP_OK
        out, mask, counts = ctx.filter_radius(m, 0.3, min_nb, mask=True, counts=True)
        assert out.shape == (0, 3) and not mask.any() and counts.min() >= 1
        assert ctx.filter_radius(m, 0.3, min_nb).shape == (0, 3)
    out = ctx.filter_radius(m, 0.3, 0)  # the point itself counts: everything kept
    np.testing.assert_array_equal(out, m)
    d = F.cloud("duplicates")
    equal = np.all(d == d[5], axis=1)
    _, _, mean = ctx.filter_statistical(d, 16, 2.0, mask=True, mean_dist=True)
    np.testing.assert_array_equal(mean[equal], 0.0)
    _, counts = ctx.filter_radius(d, 1e-6, 19, counts=True)
    np.testing.assert_array_equal(counts[equal], 20)


FILL = 123.25


def raw_statistical(amd, ctx, xyz, n, k, ratio, null=()):
    """icp_filter_statistical through ctypes with filled outputs -> (rc, the outputs)"""
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out, mask, mean, stats = np.full((8, 3), FILL), np.full(8, 7, dtype=np.uint8), np.full(8, FILL), np.full(3, FILL)
    n_out = C.c_size_t(99)
    rc = amd.lib().icp_filter_statistical(ctx._h, None if "xyz" in null else dp(xyz), n, k, ratio, dp(out),
                                          mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          None if "n_out" in null else C.byref(n_out), dp(mean), dp(stats))
    return rc, (out, mask, mean, stats, n_out.value)


def raw_radius(amd, ctx, xyz, n, radius, min_nb, null=()):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out, mask, cnt = np.full((8, 3), FILL), np.full(8, 7, dtype=np.uint8), np.full(8, -5, dtype=np.int32)
    n_out = C.c_size_t(99)
    rc = amd.lib().icp_filter_radius(ctx._h, None if "xyz" in null else dp(xyz), n, radius, min_nb, dp(out),
                                     mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     None if "n_out" in null else C.byref(n_out),
                                     cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, (out, mask, cnt, n_out.value)


def untouched(outs):
    return all((np.all(o == FILL) if o.dtype == np.float64 else np.all(o == (7 if o.dtype == np.uint8 else -5)))
               if isinstance(o, np.ndarray) else o == 99 for o in outs)


def test_refusals_name_the_value_and_write_nothing(icp_lib, ctx):
    amd = icp_lib
    x = np.ascontiguousarray(F.cloud("ell17")[:8])
    bad = x.copy()
    bad[3, 1] = np.inf
    A, R = amd.ICP_E_ARG, amd.ICP_E_RANGE
    stat = [((x, 8, 4, 1.0, ("xyz",)), A, "null"), ((x, 8, 4, 1.0, ("n_out",)), A, "null"),
            ((x, 0, 4, 1.0), A, "n = 0"), ((x, 2 ** 31, 4, 1.0), A, "n = 2147483648"),
            ((x, 8, 1, 1.0), A, "k = 1"), ((x, 8, 64, 1.0), A, "k = 64"), ((x, 8, 8, 1.0), A, "k + 1 = 9"),
            ((x, 8, 4, -0.5), A, "std_ratio = -0.5"), ((x, 8, 4, float("nan")), A, "std_ratio = nan"),
            ((x, 8, 4, float("inf")), A, "std_ratio = inf"), ((bad, 8, 4, 1.0), R, "point 3")]
    for args, code, word in stat:
        rc, outs = raw_statistical(amd, ctx, *args)
        msg = amd.lib().icp_last_error(ctx._h).decode()
        print(rc, msg)
        assert rc == code and word in msg and untouched(outs), (args[1:], rc, msg)
    rad = [((x, 8, 0.5, 1, ("xyz",)), A, "null"), ((x, 8, 0.5, 1, ("n_out",)), A, "null"),
           ((x, 0, 0.5, 1), A, "n = 0"), ((x, 2 ** 31, 0.5, 1), A, "n = 2147483648"),
           ((x, 8, 0.0, 1), A, "radius = 0"), ((x, 8, -1.0, 1), A, "radius = -1"),
           ((x, 8, float("nan"), 1), A, "radius = nan"), ((x, 8, float("inf"), 1), A, "radius = inf"),
           ((x, 8, 0.5, -1), A, "min_neighbors = -1"), ((bad, 8, 0.5, 1), R, "point 3")]
    for args, code, word in rad:
        rc, outs = raw_radius(amd, ctx, *args)
        msg = amd.lib().icp_last_error(ctx._h).decode()
        print(rc, msg)
        assert rc == code and word in msg and untouched(outs), (args[1:], rc, msg)
    # the device forms find a non-finite coordinate on the device
    d = torch.from_numpy(bad).cuda()
    o = torch.full((8, 3), FILL, dtype=torch.float64, device="cuda")
    for call in (lambda: ctx.filter_statistical_device(d.data_ptr(), 8, 4, 1.0, o.data_ptr()),
                 lambda: ctx.filter_radius_device(d.data_ptr(), 8, 0.5, 1, o.data_ptr())):
        with pytest.raises(amd.ICPError) as ei:
            call()
        assert ei.value.code == R and "non-finite" in str(ei.value)
        assert bool((o == FILL).all())
    # and a good call after all of them
    rc, outs = raw_statistical(amd, ctx, x, 8, 4, 1.0)
    assert rc == amd.ICP_OK and outs[4] <= 8 and not untouched(outs)


# 4. determinism, the device forms, isolation
def test_two_calls_and_the_device_forms_give_the_same_bits(icp_lib, ctx, oracle):
    m = F.cloud("cow_clutter", oracle.load_matrix)
    n = m.shape[0]
    a = ctx.filter_statistical(m, 16, 1.0, mask=True, mean_dist=True, stats=True)
    b = ctx.filter_statistical(m, 16, 1.0, mask=True, mean_dist=True, stats=True)
    with icp_lib.Context() as other:
        c = other.filter_statistical(m, 16, 1.0, mask=True, mean_dist=True, stats=True)
    ra = ctx.filter_radius(m, 0.4, 8, mask=True, counts=True)
    rb = ctx.filter_radius(m, 0.4, 8, mask=True, counts=True)
    for u, v, w in zip(a, b, c):
        np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(u, w)
    for u, v in zip(ra, rb):
        np.testing.assert_array_equal(u, v)
    d = torch.from_numpy(m).cuda()
    out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mean = torch.zeros(n, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    kept, stats = ctx.filter_statistical_device(d.data_ptr(), n, 16, 1.0, out.data_ptr(), mask.data_ptr(), mean.data_ptr())
    torch.cuda.synchronize()
    assert kept == a[0].shape[0]
    np.testing.assert_array_equal(out[:kept].cpu().numpy(), a[0])
    np.testing.assert_array_equal(mask.cpu().numpy(), a[1])
    np.testing.assert_array_equal(mean.cpu().numpy(), a[2])
    np.testing.assert_array_equal(stats, a[3])
    assert ctx.filter_statistical_device(d.data_ptr(), n, 16, 1.0, None)[0] == kept  # (every output is optional)
    kept = ctx.filter_radius_device(d.data_ptr(), n, 0.4, 8, out.data_ptr(), mask.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    assert kept == ra[0].shape[0]
    np.testing.assert_array_equal(out[:kept].cpu().numpy(), ra[0])
    np.testing.assert_array_equal(mask.cpu().numpy(), ra[1])
    np.testing.assert_array_equal(cnt.cpu().numpy(), ra[2])
    np.testing.assert_array_equal(d.cpu().numpy(), m)  # (the input is read only)


def test_a_run_after_the_filters_is_the_fresh_run(icp_lib, oracle):
    amd = icp_lib
    m = oracle.load_matrix(datasets.path("cow_ref"))
    p = oracle.load_matrix(datasets.path("cow_tr1"))
    clutter = F.cloud("cow_clutter", oracle.load_matrix)
    runs = []
    for form in ("fresh", "filtered"):
        with amd.Context() as c:
            c.set_model(m)
            c.set_scene(p)
            if form == "filtered":
                c.filter_statistical(clutter, 16, 1.0)
                c.filter_radius(clutter, 0.4, 8)
            res, errs = c.run(10)
            st = c.stats()
            runs.append((errs, c.get_scene(), np.array(res.R), res.s, np.array(res.t), c.get_indices(),
                         [st[key] for key in ("persistent_runs", "iterations", "ambiguous", "grid_fallback",
                                              "run_grid_searches", "run_certified", "run_walked")]))
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)


# 5. CLI
def test_cli_sor(icp_lib, ctx, oracle, tmp_path):
    amd = icp_lib
    cloud = F.cloud("cow_clutter", oracle.load_matrix)
    n = cloud.shape[0]
    cow = datasets.path("cow_ref")
    scene, nfile, out, tf, mn, mn2 = (str(tmp_path / name) for name in ("clutter.txt", "normals.txt", "out.txt", "t.txt",
                                                                        "mn.txt", "mn2.txt"))
    amd.write_matrix(scene, cloud)
    cloud = amd.load_matrix(scene)  # (what the program reads: the file's digits)
    rows = np.arange(3.0 * n).reshape(n, 3)  # row j of the "normals" names point j
    amd.write_matrix(nfile, rows)
    model = amd.load_matrix(cow)
    with amd.Context() as c2:  # the unfiltered model's normals, one row a model point
        c2.set_model(model)
        c2.estimate_model_normals(16)
        amd.write_matrix(mn, c2.model_normals())
    exe = os.path.join(BUILD, "icp-gpu")
    r = subprocess.run([exe, cow, scene, "5", "--sor", "16,2", "--out", out], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--allow-unequal" in r.stderr and "sizes will differ" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(out)
    r = subprocess.run([exe, cow, scene, "5", "--sor", "16,2", "--allow-unequal", "--normals", mn, "--write-normals", mn2,
                        "--scene-normals", nfile,
                        "--write-scene-normals", str(tmp_path / "sn.txt"), "--write-transform", tf, "--out", out],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("[sor]")]
    print("\n".join(lines))
    assert len(lines) == 2 and lines[0].startswith("[sor] model ") and lines[1].startswith("[sor] scene ")
    masks = []
    for line, xyz in zip(lines, (model, cloud)):
        kept, mask, stats = ctx.filter_statistical(xyz, 16, 2.0, mask=True, stats=True)
        masks.append(mask.astype(bool))
        w = line.split()
        assert (int(w[2]), int(w[5].rstrip(","))) == (xyz.shape[0], kept.shape[0])
        assert [float("%g" % v) for v in stats] == [float(w[7]), float(w[9]), float(w[11])]
    assert amd.load_matrix(out).shape == (kept.shape[0], 3)  # the kept scene points, registered
    # a --normals file of the unfiltered size is accepted and trimmed: the run's normals are the kept rows
    np.testing.assert_array_equal(amd.load_matrix(mn2), amd.load_matrix(mn)[masks[0]])
    # the scene file's rows followed the mask too (the written normals are the kept rows, turned by the run's rotation)
    sn = amd.load_matrix(str(tmp_path / "sn.txt"))
    T = np.loadtxt(tf, delimiter=",")[:3, :3]
    Q = T / np.cbrt(np.linalg.det(T))  # (the total is s R; the normals turn by R)
    np.testing.assert_allclose(sn, rows[mask.astype(bool)] @ Q.T, rtol=1e-4, atol=1e-4 * np.abs(rows).max())
    # --sor before --ror, one line per cloud and filter
    r = subprocess.run([exe, cow, scene, "2", "--ror", "0.4,8", "--sor", "16,2", "--allow-unequal", "--out", out],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    tags = [l.split()[0] + l.split()[1] for l in r.stderr.splitlines() if l.startswith(("[sor]", "[ror]"))]
    assert tags == ["[sor]model", "[ror]model", "[sor]scene", "[ror]scene"]
    last = [l for l in r.stderr.splitlines() if l.startswith("[ror] scene")][0].split()
    assert int(last[2]) == kept.shape[0]
    assert int(last[5]) == ctx.filter_radius(kept, 0.4, 8).shape[0] == amd.load_matrix(out).shape[0]
