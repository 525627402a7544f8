"""The fused grid iteration (icp_grid.hip nn_grid_iter2_kernel) at the smallest scenes the run
policy gives it, where a task's edge cases are a large share of the work.

icp_run takes the fused kernel for a scene kept in slot order (more than 49,152 points and at
least 2^31 query-model pairs, whatever the run mode), so the scenes have 2^16 + 37 points: not a
multiple of 64, the last task ragged, its walkers' batch no power of two.  Each case runs 8
iterations of the GRID variant

  * with the fused kernel (the default),
  * with the separate transform / seeded search / moments kernels (ICP_GRID_ITER=0),
  * with the fused kernel on 64-bit addresses (ICP_ITER2_A32=0: the form it takes when an array
    reaches 4 GiB),

each setting in its own process (the switches are read once a process), and the three agree bit
for bit: errors, per-iteration index digests, final scene, transform.  The fused run's final
indices are the oracle's brute-force first minimum of every query (over the scene of 7 iterations,
from a second context: the trajectory is exact), and its statistics show that the fused kernel ran
and walked.

  ragged   a synthetic pair of 2^16 + 37 points
  far      a model 5e4 from the origin with extent 3: the fp32 image's room at its tightest
  clump    a uniform cube; 600 scene points in a clump a dozen cells outside the model's box: their
           boxes exceed the walk's (the whole-wave path)
  lattice  a 41^3 integer lattice; the scene on the lattice's cell faces (half-integer offsets
           on two axes, no rotation): every query tied between four model points at the first
           iteration, coordinates on floor()'s edges
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (1 << 16) + 37
ITERS = 8
CASES = ["ragged", "far", "clump", "lattice"]

SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import icp_amd
from test_gpu_iter_small import ITERS, CASES, case
out = {}
for name in CASES:
    m, p = case(name)
    with icp_amd.Context(0) as ctx:
        ctx.set_nn_variant(icp_amd.VARIANT_GRID)
        ctx.set_allow_unequal(True)  # (the lattice: 41^3 model points)
        ctx.set_model(m)
        ctx.set_scene(p)
        ctx.set_index_digest(ITERS)
        res, errs = ctx.run(ITERS, -1.0)
        st = ctx.stats()
        out[name + "_errs"] = errs
        out[name + "_dig"] = ctx.index_digest(ITERS)
        out[name + "_scene"] = ctx.get_scene()
        out[name + "_xf"] = np.concatenate([[res.s], np.array(res.R[:]), np.array(res.t[:])])
        out[name + "_idx"] = ctx.get_indices()
        out[name + "_stats"] = np.array([st["run_grid_searches"], st["run_walked"], st["run_certified"]])
    if sys.argv[4] == "prev":  # the scene the last search ran on
        with icp_amd.Context(0) as ctx:
            ctx.set_nn_variant(icp_amd.VARIANT_GRID)
            ctx.set_allow_unequal(True)
            ctx.set_model(m)
            ctx.set_scene(p)
            ctx.run(ITERS - 1, -1.0)
            out[name + "_prev"] = ctx.get_scene()
np.savez(sys.argv[3], **out)
print("iter small ok")
"""


def rotation(deg, axis=(1.0, 2.0, 3.0)):
    a = np.asarray(axis) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def case(name):
    rng = np.random.default_rng(23)
    if name == "ragged":
        import icp_amd
        return icp_amd.synthetic_pair(N, seed=41, angle_deg=4.0)
    if name == "far":
        c = np.array([5e4, 5e4, 5e4])
        m = c + rng.uniform(-1.5, 1.5, size=(N, 3))
        p = (m - c) @ rotation(2.0).T + c + [0.01, -0.02, 0.015]
        return m, p[rng.permutation(N)]
    if name == "clump":
        m = rng.uniform(-1.0, 1.0, size=(N, 3))
        p = m @ rotation(2.0).T + [0.01, -0.02, 0.015]
        h = np.cbrt(8.0 * 2.0 / N)  # (about the grid's cell: two points a cell)
        p[:600] = [1.0 + 12.0 * h, 0.3, -0.2] + rng.uniform(-h, h, size=(600, 3))
        return m, p[rng.permutation(N)]
    g = np.stack(np.meshgrid(np.arange(41), np.arange(41), np.arange(41), indexing="ij"), -1)
    m = g.reshape(-1, 3).astype(np.float64)
    p = m[rng.permutation(len(m))[:N]] + [0.5, 0.5, 0.0]
    return m, p


def run_setting(tmp_path, name, env, prev):
    out = str(tmp_path / f"iter_small_{name}.npz")
    r = subprocess.run([sys.executable, "-c", SCRIPT, os.path.join(ROOT, "iterative-closest-point_amd"),
                        os.path.join(ROOT, "tests"), out, "prev" if prev else "-"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and "iter small ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def settings(icp_lib, tmp_path_factory):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    tmp = tmp_path_factory.mktemp("iter_small")
    return {"fused": run_setting(tmp, "fused", {}, True),
            "separate": run_setting(tmp, "separate", {"ICP_GRID_ITER": "0"}, False),
            "addr64": run_setting(tmp, "addr64", {"ICP_ITER2_A32": "0"}, False)}


@pytest.mark.parametrize("other", ["separate", "addr64"])
@pytest.mark.parametrize("name", CASES)
def test_fused_small_scene_equals_other_paths_bitwise(settings, name, other):
    a, b = settings["fused"], settings[other]
    searches, walked, _ = a[name + "_stats"]
    assert searches == ITERS and walked > 0, a[name + "_stats"]  # (the fused kernel ran, and walked)
    for k in ("errs", "dig", "scene", "xf", "idx"):
        assert np.array_equal(a[f"{name}_{k}"], b[f"{name}_{k}"]), k


@pytest.mark.parametrize("name", CASES)
def test_fused_small_scene_matches_brute_force(settings, oracle, name):
    a = settings["fused"]
    m, p = case(name)
    assert len(p) == N and N % 64 != 0
    _, ref = oracle.closest_blocked(a[name + "_prev"], m)
    got = a[name + "_idx"]
    assert np.array_equal(got, ref), (name, int(np.sum(got != ref)))
