"""A plain `bench.py` run on the GPU: the lean result line and `--dump-outputs`.

One run of the benchmark at a small size (one step, no warm-up).  Its line carries the headline
fields and none of what `--full` adds, and the arrays it writes are what the same registration
gives a caller of the engine directly: the inputs are seeded, so the comparison is exact.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20001  # odd, above the one-launch LDS path's 4096 queries
FULL_ONLY = ("steady_state", "step_phases", "registration", "value_pcie_inclusive", "streaming", "cow_frame_rate",
             "reference_cases", "baseline_configs", "csv_io", "grid_nn", "full_nxm_filter", "cpu_baseline")


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, icp_lib):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                        "--points", str(N), "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(30 * 1e3 / line["ms_per_step"])
    assert not [k for k in FULL_ONLY if k in line]

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["correspondences", "err_trace", "result", "scene", "transform"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    m, p = icp_lib.synthetic_pair(N, seed=42)
    with icp_lib.Context(0) as ctx:
        ctx.set_model(m)
        ctx.set_scene(p)
        res, errs = ctx.run(30, -1.0)
        scene, idx = ctx.get_scene(), ctx.get_indices()
    assert np.array_equal(got["err_trace"], errs) and line["final_err"] == errs[-1]
    assert np.array_equal(got["transform"], [res.s] + list(res.R) + list(res.t))
    assert np.array_equal(got["result"], [res.iterations, res.converged, res.err])
    assert np.array_equal(got["scene"], scene)
    assert np.array_equal(got["correspondences"], idx)
