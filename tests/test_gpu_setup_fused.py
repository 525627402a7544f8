"""The registration's set-up with its fused and deferred pieces against the set-up before.

Before the loop a registration prepares the model (statistics, images, the grid: two radix sorts
between model and scene) and orders the scene.  The pieces under test change launches, not values:

  * ICP_SORT_WAVES / ICP_SORT_PREFIX: the sort's workgroup size and its in-scatter prefix
    (icp_sort.hip);
  * ICP_GRID_FUSED: each cell's start from the sorted ids' neighbours, in the gather (icp_grid.hip);
  * ICP_M32_LAZY: the fp32 operand images m32 / mperm / mm built at their first reader, from the
    resident SoA model (ensure_m32), not at icp_set_model from the caller's array.

Every switch is read once, so a setting runs in a subprocess.  trajectory() is that of
test_gpu_setup_path.py (8 iterations: errors, index digest, scene, R, t, s) at model 2^16 and scene
2^16 + 37, the smallest size at which the scene takes the slot order (n > 49,152, n nm >= 2^31).
Checked bit for bit:

  * the defaults against every switch off;
  * host setters against device setters (a torch tensor's pointer), under both;
  * a context that runs a grid-served registration first and then the same clouds under an fp32
    filter variant (VALU: m32; MFMA: mperm and mm) against a fresh context of that variant -- the
    images built late, after the caller's array could be gone, equal those built at once.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OFF = dict(ICP_SORT_WAVES="4", ICP_SORT_PREFIX="0", ICP_GRID_FUSED="0", ICP_M32_LAZY="0")

SCRIPT = r"""
import sys, numpy as np
import torch  # (before the first HIP call: torch then sees the device)
sys.path.insert(0, sys.argv[1])
import icp_amd
nm = 1 << 16
n = nm + 37
m, p = icp_amd.synthetic_pair(n, seed=21)
m = np.ascontiguousarray(m[:nm])
out = {}

def trajectory(ctx, tag, iters=8):
    ctx.set_index_digest(iters)
    res, errs = ctx.run(iters, -1.0)
    out[tag + "_errs"] = np.asarray(errs)
    out[tag + "_dig"] = np.asarray(ctx.index_digest(iters))
    out[tag + "_scene"] = ctx.get_scene()
    out[tag + "_R"] = np.array(res.R[:])
    out[tag + "_t"] = np.array(res.t[:])
    out[tag + "_s"] = np.array([res.s])

with icp_amd.Context(0) as ctx:
    ctx.set_allow_unequal(True)
    ctx.set_model(m)
    ctx.set_scene(p)
    trajectory(ctx, "host")
dm = torch.from_numpy(m).to("cuda:0")
dp = torch.from_numpy(p).to("cuda:0")
torch.cuda.synchronize()
with icp_amd.Context(0) as ctx:
    ctx.set_allow_unequal(True)
    ctx.set_model_device(dm.data_ptr(), nm)
    ctx.set_scene_device(dp.data_ptr(), n)
    trajectory(ctx, "device")
for name, variant in (("valu", icp_amd.VARIANT_VALU), ("mfma", icp_amd.VARIANT_MFMA)):
    with icp_amd.Context(0) as ctx:  # grid-served first, the variant afterwards
        ctx.set_allow_unequal(True)
        dm2 = dm.clone()
        torch.cuda.synchronize()
        ctx.set_model_device(dm2.data_ptr(), nm)
        ctx.set_scene(p)
        ctx.run(3, -1.0)
        dm2.zero_()  # (the caller's array is only promised until icp_run returns)
        torch.cuda.synchronize()
        ctx.set_nn_variant(variant)
        ctx.set_scene(p)
        trajectory(ctx, name + "_late", iters=4)
    with icp_amd.Context(0) as ctx:
        ctx.set_allow_unequal(True)
        ctx.set_nn_variant(variant)
        ctx.set_model(m)
        ctx.set_scene(p)
        trajectory(ctx, name + "_fresh", iters=4)
np.savez(sys.argv[2], **out)
print("setup ok")
"""

KEYS = ("errs", "dig", "scene", "R", "t", "s")


def run_setup(tmp_path_factory, tag, extra):
    out = str(tmp_path_factory.mktemp("setup") / f"setup_{tag}.npz")
    env = dict(os.environ, **extra)
    r = subprocess.run([sys.executable, "-c", SCRIPT, os.path.join(ROOT, "iterative-closest-point_amd"), out],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "setup ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(icp_lib, tmp_path_factory):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return {"new": run_setup(tmp_path_factory, "new", {}), "old": run_setup(tmp_path_factory, "old", OFF)}


def assert_same(d, a, e, b):
    for k in KEYS:
        assert np.array_equal(d[f"{a}_{k}"], e[f"{b}_{k}"]), (a, b, k)


def test_new_setup_matches_every_switch_off(runs):
    assert runs["new"].keys() == runs["old"].keys()
    for k in runs["new"]:
        assert np.array_equal(runs["new"][k], runs["old"][k]), k


@pytest.mark.parametrize("which", ["new", "old"])
def test_host_setters_match_device_setters(runs, which):
    assert_same(runs[which], "host", runs[which], "device")


@pytest.mark.parametrize("which", ["new", "old"])
@pytest.mark.parametrize("variant", ["valu", "mfma"])
def test_fp32_images_built_late_match_a_fresh_context(runs, which, variant):
    d = runs[which]
    assert len(d[f"{variant}_late_errs"]) == 4
    assert_same(d, f"{variant}_late", d, f"{variant}_fresh")
