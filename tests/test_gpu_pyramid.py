"""Coarse-to-fine registration from the engine's three calls (icp_voxel_downsample,
icp_transform_scene, icp_get_transform): icp_amd.register_pyramid and the CLI's --pyramid.

The voxel of the cow pair's coarse level is extent / 16 (voxel_ref.COW_VOXEL_DIV: tests/test_voxel_ref.py
checks on the CPU that the numpy twin then needs at most half the plain run's iterations).
test_matches_the_numpy_twin holds one- and two-level pyramids to voxel_ref.pyramid_twin itself.
"""
import os
import subprocess

import numpy as np
import pytest

import datasets
import voxel_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iterative-closest-point_amd", "build", "icp-gpu")
LEVEL_ITERS = 30


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


@pytest.fixture(scope="module")
def cow(icp_lib):
    return icp_lib.load_matrix(datasets.path("cow_ref")), icp_lib.load_matrix(datasets.path("cow_tr2"))


@pytest.fixture(scope="module")
def pyramid(icp_lib, cow):
    """The cow pair's coarse-to-fine run, once: (res, total, records, final scene)."""
    m, p = cow
    with icp_lib.Context() as ctx:
        res, total, records = icp_lib.register_pyramid(ctx, m, p, [V.extent(m) / V.COW_VOXEL_DIV], 30, LEVEL_ITERS)
        return res, total, records, ctx.get_scene()


def test_equals_the_hand_made_sequence(icp_lib, cow, pyramid):
    amd = icp_lib
    m, p = cow
    res, total, records, scene = pyramid
    h = V.extent(m) / V.COW_VOXEL_DIV
    with amd.Context() as ctx:
        mc, pc = ctx.voxel_downsample(m, h), ctx.voxel_downsample(p, h)
        ctx.set_allow_unequal(True)
        ctx.set_model(mc)
        ctx.set_scene(pc)
        ctx.transform_scene(1.0, np.eye(3), np.zeros(3))
        r0, e0 = ctx.run(LEVEL_ITERS)
        pose = ctx.transform()
        ctx.set_allow_unequal(False)
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.transform_scene(*pose)
        r1, e1 = ctx.run(30)
        s, R, t = ctx.transform()
        assert bits(ctx.get_scene()) == bits(scene)
    assert (mc.shape[0], pc.shape[0], r0.iterations) == tuple(records[0][k] for k in ("model_points", "scene_points",
                                                                                      "iterations"))
    assert bits(e0) == bits(records[0]["errs"]) and bits(e1) == bits(records[1]["errs"])
    assert r1.iterations == res.iterations and bits([r1.err]) == bits([res.err])
    assert bits([s]) == bits([total[0]]) and bits(R) == bits(total[1]) and bits(t) == bits(total[2])


def test_fine_level_needs_at_most_half_the_iterations(icp_lib, cow, pyramid):
    m, p = cow
    res, _, records, _ = pyramid
    with icp_lib.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        plain, _ = ctx.run(30)
    print(f"plain {plain.iterations} iterations; after a coarse pass ({records[0]['model_points']} / "
          f"{records[0]['scene_points']} points, {records[0]['iterations']} iterations) {res.iterations}, err {res.err:.3g}")
    assert plain.converged and res.converged and res.err < 1e-5
    assert records[1]["voxel"] is None and records[1]["iterations"] == res.iterations
    assert 2 * res.iterations <= plain.iterations


def test_total_moves_the_original_scene_onto_the_final_one(cow, pyramid):
    _, p = cow
    _, (s, R, t), _, scene = pyramid
    gap = float(np.abs((p @ (s * R).T + t) - scene).max())
    bound = 8.0 * V.G_REL * float(np.abs(p).max())
    print(f"total against the final scene: {gap:.3e} (bound {bound:.3e})")
    assert gap <= bound


_TWIN = {}


def twin(m, p, divs):
    """voxel_ref.pyramid_twin on the order rule's coarse clouds, every run its full count: once per pyramid."""
    if tuple(divs) not in _TWIN:
        _TWIN[tuple(divs)] = V.pyramid_twin(m, p, [V.extent(m) / d for d in divs], V.PYRAMID_FINE_ITERS,
                                            V.PYRAMID_LEVEL_ITERS, -1.0, V.coarse_rule)
    return _TWIN[tuple(divs)]


@pytest.mark.parametrize("divs", V.COW_PYRAMIDS)
def test_matches_the_numpy_twin(icp_lib, cow, divs):
    """One level and two against the numpy twin, at the tolerances tests/test_gpu_parity.py holds the cow
    pair's plain run to (tests/test_voxel_ref.py: the twin moves by less than a hundredth of them when its
    coarse means are rounded another way)."""
    m, p = cow
    moved, errs, (s, R, t), levels = twin(m, p, divs)
    with icp_lib.Context() as ctx:
        res, total, records = icp_lib.register_pyramid(ctx, m, p, [V.extent(m) / d for d in divs], V.PYRAMID_FINE_ITERS,
                                                       V.PYRAMID_LEVEL_ITERS, threshold=-1.0)
        scene = ctx.get_scene()
    assert len(records) == len(divs) + 1
    for rec, lev in zip(records, levels):
        assert (rec["model_points"], rec["scene_points"], rec["iterations"]) == lev[:3]
        print(f"{divs} level h = {rec['voxel']:.4g}: errs {np.max(np.abs(rec['errs'] - lev[3]) / lev[3]):.3e} relative")
    assert records[-1]["iterations"] == res.iterations == len(errs) == V.PYRAMID_FINE_ITERS
    scale = float(np.abs(m).max())
    print(f"{divs}: errs {np.max(np.abs(records[-1]['errs'] - errs) / errs):.3e} relative, scene "
          f"{np.abs(scene - moved).max():.3e}, s {abs(total[0] - s):.3e}, R {np.abs(total[1] - R).max():.3e}, "
          f"t {np.abs(total[2] - t).max():.3e}")
    np.testing.assert_allclose(records[-1]["errs"], errs, rtol=1e-9)
    np.testing.assert_allclose(scene, moved, atol=1e-9 * scale)
    assert abs(total[0] - s) <= 1e-9
    np.testing.assert_allclose(total[1], R, atol=1e-9)
    np.testing.assert_allclose(total[2], t, atol=1e-9 * scale)


def test_cli_pyramid_writes_the_python_paths_scene(icp_lib, cow, pyramid, tmp_path):
    m, _ = cow
    _, (s, R, t), records, scene = pyramid
    h = V.extent(m) / V.COW_VOXEL_DIV
    r = subprocess.run([EXE, datasets.path("cow_ref"), datasets.path("cow_tr2"), "30", "--pyramid", repr(h),
                        "--pyramid-iters", str(LEVEL_ITERS), "--write-transform", "total.txt"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    icp_lib.write_matrix(str(tmp_path / "python.txt"), scene)
    assert (tmp_path / "output.txt").read_bytes() == (tmp_path / "python.txt").read_bytes()
    level = [l for l in r.stderr.splitlines() if l.startswith("[pyramid] level")]
    assert len(level) == 1
    assert f"model {records[0]['model_points']} scene {records[0]['scene_points']} points, {records[0]['iterations']} iterations" in level[0]
    assert any(l.startswith("[pyramid] total s=") for l in r.stderr.splitlines())
    T = np.array([[float(v) for v in l.split(",")] for l in (tmp_path / "total.txt").read_text().splitlines()])
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = s * R, t
    want = np.array([[float("%g" % v) for v in row] for row in want])
    assert T.shape == (4, 4) and np.array_equal(T, want)


def test_cli_write_transform_without_a_pyramid(icp_lib, cow, tmp_path):
    m, p = cow
    r = subprocess.run([EXE, datasets.path("cow_ref"), datasets.path("cow_tr2"), "5", "--write-transform", "total.txt"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with icp_lib.Context() as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.run(5)
        s, R, t = ctx.transform()
    T = np.array([[float(v) for v in l.split(",")] for l in (tmp_path / "total.txt").read_text().splitlines()])
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = s * R, t
    assert np.array_equal(T, np.array([[float("%g" % v) for v in row] for row in want]))


@pytest.mark.parametrize("extra", [
    ["--pyramid", "0.3,,0.1"], ["--pyramid", "0.3,"], ["--pyramid", ""], ["--pyramid", "0.3,-0.1"], ["--pyramid", "0"],
    ["--pyramid", "abc"], ["--pyramid", "0.3", "--normals", "normals.txt"], ["--pyramid-iters", "5"],
    ["--pyramid", "0.3", "--pyramid-iters", "x"],
])
def test_cli_bad_options_exit_before_any_load(tmp_path, extra):
    r = subprocess.run([EXE, datasets.path("cow_ref"), datasets.path("cow_tr2"), "5"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "[load]" not in r.stderr and "[error]" in r.stderr


def test_cli_level_too_small_for_the_normals(tmp_path):
    """A level whose model has fewer than K points is an error raised before any run."""
    r = subprocess.run([EXE, datasets.path("cow_ref"), datasets.path("cow_tr2"), "5", "--pyramid", "100",
                        "--estimate-normals", "8"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "--estimate-normals" in r.stderr
    assert "[ICP]" not in r.stderr and "[pyramid] level" not in r.stderr
