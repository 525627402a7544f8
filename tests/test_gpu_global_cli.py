"""icp-gpu --global (icp_cli.cpp): the CLI makes icp_amd.register_global's calls in its order, so the
moved scene it writes is that path's, byte for byte; the [global] line reports icp_global_pose's figures;
--write-transform holds the total, the global pose included; bad values exit in the CLI's error style.
"""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import datasets
import global_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iterative-closest-point_amd", "build", "icp-gpu")
ITERS = 30


@pytest.fixture(scope="module")
def turned_cow(icp_lib, tmp_path_factory):
    """The cow turned 120 degrees, as a scene file, and the file's own values -> (path, m, p, R_true)"""
    m, p, R_true, _ = G.cow_pair(icp_lib.load_matrix)
    path = str(tmp_path_factory.mktemp("global") / "cow_turned.txt")
    icp_lib.write_matrix(path, p)
    return path, m, icp_lib.load_matrix(path), R_true


def test_cli_global_writes_the_python_paths_scene(icp_lib, turned_cow, tmp_path):
    path, m, p, R_true = turned_cow
    r = subprocess.run([EXE, datasets.path("cow_ref"), path, str(ITERS), "--global", repr(G.COW_VOXEL), "--global-seed",
                        str(G.PURPOSE_SEED), "--threshold", "-1", "--write-transform", "total.txt"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with icp_lib.Context() as ctx:
        res, _, (s, R, t), (R0, _), rep = icp_lib.register_global(ctx, m, p, G.COW_VOXEL, ITERS, -1.0,
                                                                    seed=G.PURPOSE_SEED)
        icp_lib.write_matrix(str(tmp_path / "python.txt"), ctx.get_scene())
    assert (tmp_path / "output.txt").read_bytes() == (tmp_path / "python.txt").read_bytes()
    line = [l for l in r.stderr.splitlines() if l.startswith("[global]")]
    assert line == [f"[global] model {rep['model_points']} scene {rep['scene_points']} points, matches {rep['matches']}, "
                    f"evaluated {rep['evaluated']}, inliers {rep['inliers']}, hypothesis {rep['best_h']}"]
    # the total holds the global pose: it is the true motion, not the few degrees the iterations added
    T = np.array([[float(v) for v in l.split(",")] for l in (tmp_path / "total.txt").read_text().splitlines()])
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = s * R, t
    assert T.shape == (4, 4) and np.array_equal(T, np.array([[float("%g" % v) for v in row] for row in want]))
    assert G.angle_deg(R0, R_true) < 5.0 and G.angle_deg(T[:3, :3], R_true) < 0.01
    assert res.err < 1e-9  # (the file's six digits: a squared rounding error of at most 7.5e-11 a point)
    # the aligned scene lies on the model
    moved = icp_lib.load_matrix(str(tmp_path / "output.txt"))
    assert np.abs(moved - m).max() < 1e-4


def test_cli_global_under_a_pyramid_and_with_normals(icp_lib, turned_cow, tmp_path):
    """The pose is the pyramid's initial pose, and the scene's normals are estimated before the scene moves."""
    path, m, _, R_true = turned_cow
    for extra in (["--pyramid", "0.2", "--pyramid-iters", "10"],
                  ["--estimate-normals", "12", "--estimate-scene-normals", "12", "--symmetric"]):
        r = subprocess.run([EXE, datasets.path("cow_ref"), path, str(ITERS), "--global", repr(G.COW_VOXEL), "--global-seed",
                            str(G.PURPOSE_SEED), "--global-hyp", "20000", "--threshold", "-1", "--write-transform", "total.txt"] + extra,
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sum(l.startswith("[global]") for l in r.stderr.splitlines()) == 1
        T = np.array([[float(v) for v in l.split(",")] for l in (tmp_path / "total.txt").read_text().splitlines()])
        assert G.angle_deg(T[:3, :3], R_true) < 0.01, extra
        assert np.abs(icp_lib.load_matrix(str(tmp_path / "output.txt")) - m).max() < 1e-4, extra


NEED = "need --global"


@pytest.mark.parametrize("extra, names", [
    (["--global", "0"], "--global: 0 "), (["--global", "-0.1"], "--global: -0.1 "), (["--global", "abc"], "--global: abc "),
    (["--global", "0.1x"], "--global: 0.1x "), (["--global-k", "32"], NEED), (["--global-seed", "3"], NEED),
    (["--global-normals-k", "16"], NEED), (["--global-hyp", "10"], NEED), (["--global-dist", "0.1"], NEED),
    (["--global", "0.12", "--global-k", "2"], "--global-k: K = 2 "),
    (["--global", "0.12", "--global-k", "65"], "--global-k: K = 65 "),
    (["--global", "0.12", "--global-normals-k", "x"], "--global-normals-k: K = x "),
    (["--global", "0.12", "--global-hyp", "0"], "--global-hyp: 0 "),
    (["--global", "0.12", "--global-hyp", "4294967296"], "--global-hyp: 4294967296 "),
    (["--global", "0.12", "--global-seed", "-1"], "--global-seed: -1 "),
    (["--global", "0.12", "--global-dist", "0"], "--global-dist: 0 "),
    (["--global", "0.12", "--global-dist", "nan"], "--global-dist: nan "),
])
def test_cli_bad_values_exit_before_any_load(tmp_path, extra, names):
    """The new validation's own message (an unknown option would exit the same way with another one)."""
    r = subprocess.run([EXE, datasets.path("cow_ref"), datasets.path("cow_tr2"), "5"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "[load]" not in r.stderr and "unknown option" not in r.stderr
    assert "[error] " + names in r.stderr or (names == NEED and NEED in r.stderr), r.stderr


def test_cli_voxel_too_coarse_is_the_engines_error(tmp_path):
    r = subprocess.run([EXE, datasets.path("cow_ref"), datasets.path("cow_tr2"), "5", "--global", "2.0"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "[error] --global:" in r.stderr and "[ICP]" not in r.stderr
