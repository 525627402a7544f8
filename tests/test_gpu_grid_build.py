"""The model grid's build (icp_grid.hip: launch_grid_build) against numpy, through icp_get_grid.

The grid is a list of the model's points sorted by cell id (ties in index order) and, per cell,
the first position of the list at or after it.  The build takes each cell's start from the sorted
ids' neighbours in the kernel that gathers the points (position k writes start[c] = k for every
c in (id[k - 1], id[k]], the last position also start[c] = nm for the cells after it) instead of a
binary search per cell; ICP_GRID_FUSED=0 is the build before (read once: a subprocess per
setting).  Checked for both settings, and one against the other bit for bit:

  * order = the stable argsort of the cell ids, cell = clip(floor((x - lo) * inv_h), 0, g - 1) per
    axis in float64 (the device's own arithmetic: no FMA there), id = (cz g_y + cy) g_x + cx;
  * start = searchsorted(sorted ids, arange(ncell + 1)).

Models: one point; 4,097 identical points (one cell); 2^16 + 37 uniform points; 2^16 points on a
plane and on a line, both running from one corner of the box to the opposite one so that the id
range begins and ends with empty cells and holds long runs of them; two far clumps (almost every
cell empty, the first and the last too).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODELS = ["one", "same", "uniform", "plane", "line", "clumps"]

SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import icp_amd
from test_gpu_grid_build import MODELS, model
out = {}
for name in MODELS:
    m = model(name)
    with icp_amd.Context(0) as ctx:
        ctx.set_model(m)
        g = ctx.get_grid(m.shape[0])
    for k, v in g.items():
        out[f"{name}_{k}"] = np.asarray(v)
np.savez(sys.argv[3], **out)
print("grid build ok")
"""


def model(name):
    rng = np.random.default_rng(11)
    n = 1 << 16
    if name == "one":
        return np.array([[0.25, -1.5, 3.0]])
    if name == "same":
        return np.tile(np.array([[1.0, 2.0, -3.0]]), (4097, 1))
    if name == "uniform":
        return rng.uniform(-1, 1, size=(n + 37, 3))
    if name == "plane":  # z = -x: cell (0, 0, 0) and the last cell are empty
        xy = rng.uniform(-1, 1, size=(n, 2))
        return np.column_stack([xy[:, 0], xy[:, 1], -xy[:, 0]])
    if name == "line":  # along (1, -1, -1)
        t = rng.uniform(-1, 1, size=n)
        return np.column_stack([t, -t, -t])
    if name == "clumps":
        c = np.where(rng.random(n)[:, None] < 0.5, [[-10.0, 10.0, 0.0]], [[10.0, -10.0, 0.5]])
        return c + rng.uniform(-0.1, 0.1, size=(n, 3))
    raise KeyError(name)


def build(tmp_path_factory, flag):
    out = str(tmp_path_factory.mktemp("grid") / f"grid_{flag}.npz")
    env = dict(os.environ, ICP_GRID_FUSED=flag)
    r = subprocess.run([sys.executable, "-c", SCRIPT, os.path.join(ROOT, "iterative-closest-point_amd"),
                        os.path.join(ROOT, "tests"), out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "grid build ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def grids(icp_lib, tmp_path_factory):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return {flag: build(tmp_path_factory, flag) for flag in ("1", "0")}


@pytest.fixture(scope="module")
def expected():
    """Per model and grid geometry: (order, start) from numpy (the geometry is the build's own)."""
    cache = {}

    def get(name, g, lo, inv_h):
        key = (name, tuple(g), tuple(lo), inv_h)
        if key not in cache:
            m = model(name)
            c = [np.clip(np.floor((m[:, a] - lo[a]) * inv_h), 0, g[a] - 1).astype(np.int64) for a in range(3)]
            ids = (c[2] * g[1] + c[1]) * g[0] + c[0]
            order = np.argsort(ids, kind="stable")
            ncell = int(g[0]) * int(g[1]) * int(g[2])
            cache[key] = (order.astype(np.int32),
                          np.searchsorted(ids[order], np.arange(ncell + 1), side="left").astype(np.int32))
        return cache[key]

    return get


@pytest.mark.parametrize("flag", ["1", "0"])
@pytest.mark.parametrize("name", MODELS)
def test_grid_matches_numpy(grids, expected, name, flag):
    d = grids[flag]
    g, lo, inv_h = d[f"{name}_g"], d[f"{name}_lo"], float(d[f"{name}_inv_h"])
    order, start = expected(name, g, lo, inv_h)
    assert np.array_equal(d[f"{name}_order"], order)
    assert np.array_equal(d[f"{name}_start"], start)
    if name in ("plane", "line", "clumps"):  # (the case is what it claims: empty ends, long empty runs)
        assert start[1] == 0 and start[-2] == start[-1]
        assert np.max(np.diff(np.flatnonzero(np.diff(start)))) > 16


def test_fused_build_matches_build_before(grids):
    new, old = grids["1"], grids["0"]
    assert new.keys() == old.keys()
    for k in new:
        assert np.array_equal(new[k], old[k]), k
