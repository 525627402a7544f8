"""bench.py's command line under the driver's launcher (CPU only: argument parsing, no engine).

The multi-GPU runs go through `python -m torch.distributed.run ... bench.py --gpus N ...`; that
launcher's own parser must hand every bench option to bench.py (a bare `--n` was taken as an
ambiguous prefix of --nnodes / --nproc-per-node and the launch stopped).
"""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BENCH_FLAGS = ["--full", "--gpus", "8", "--steps", "30", "--warmup", "2", "--points", "8388608", "--no-cow",
               "--no-cases", "--no-cpu-baseline", "--variant", "auto", "--nn", "certified",
               "--dump-outputs", "out"]


def test_torchrun_passes_every_bench_flag_through():
    from torch.distributed.run import get_args_parser
    args = get_args_parser().parse_args(["--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                                         "--master-port", "29500", "bench.py"] + BENCH_FLAGS)
    assert args.training_script == "bench.py"
    assert args.training_script_args == BENCH_FLAGS


def test_bench_help_lists_points_and_keeps_n_alias():
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert re.search(r"--points N, --n N", out.stdout), out.stdout
    assert "--full" in out.stdout and "--dump-outputs DIR" in out.stdout, out.stdout


@pytest.mark.parametrize("doc", ["README.md", "DESIGN.md"])
def test_documented_torchrun_commands_parse(doc):
    """Every `bench.py` line of a documented torchrun command passes the launcher's parser."""
    from torch.distributed.run import get_args_parser
    text = (ROOT / doc).read_text()
    cmds = re.findall(r"torch\.distributed\.run ([^\n]*\\\n[^\n]*|[^\n]*)", text)
    checked = 0
    for c in cmds:
        argv = c.replace("\\\n", " ").split("#")[0].split()
        if "bench.py" not in argv:
            continue
        argv = [a for a in argv if "$" not in a]
        args = get_args_parser().parse_args(argv)
        assert args.training_script == "bench.py"
        checked += 1
    assert checked > 0


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float64_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: every output of the last step as float64 <name>.npy; a shard above
    DUMP_MAX_ROWS is written as the same seeded, ascending sample of rows on every call."""
    import numpy as np
    bench = _bench_module()
    scene = np.arange(30.0).reshape(10, 3)
    idx = np.arange(10, dtype=np.int32)[::-1].copy()

    class Ctx:
        def get_scene(self):
            return scene.copy()

        def get_indices(self):
            return idx.copy()

    class Res:
        iterations, converged, err, s, R, t = 3, 0, 0.25, 1.0, list(range(9)), [0.5, 0.25, 0.125]

    errs = np.array([1.0, 0.5, 0.25])
    bench.dump_outputs(Ctx(), Res(), errs, str(tmp_path / "a"), 0, 1)
    got = {f.stem: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["correspondences", "err_trace", "result", "scene", "transform"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["scene"], scene) and np.array_equal(got["correspondences"], idx)
    assert np.array_equal(got["transform"], [1.0] + list(range(9)) + [0.5, 0.25, 0.125])
    assert np.array_equal(got["result"], [3, 0, 0.25]) and np.array_equal(got["err_trace"], errs)

    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 4)
    for d in ("b", "c"):
        bench.dump_outputs(Ctx(), Res(), errs, str(tmp_path / d), 1, 2)
    b = {f.stem: np.load(f) for f in (tmp_path / "b").iterdir()}
    rows = b["sample_rows_rank1"].astype(int)
    assert rows.size == 4 and np.all(np.diff(rows) > 0)
    assert np.array_equal(b["scene_rank1"], scene[rows]) and np.array_equal(b["correspondences_rank1"], idx[rows])
    for name, a in b.items():
        assert np.array_equal(a, np.load(tmp_path / "c" / f"{name}.npy"))


def test_dtype_describes_what_ran():
    """The line's dtype is composed from one registration's counters (icp_stats), not fixed text:
    a C4 registration that ran only grid searches names the grid kernel and its certified share and
    no bundle filter; one whose early searches took the bundle cascade names both."""
    bench = _bench_module()
    grid_only = {"run_grid_searches": 30, "run_bundle_searches": 0, "run_certified": 750, "run_walked": 250}
    d = bench.path_description(grid_only)
    assert "30 exact fp64 grid searches" in d and bench.grid_kernel() in d and "75%" in d
    assert "bundle" not in d
    mixed = {"run_grid_searches": 27, "run_bundle_searches": 3, "run_certified": 0, "run_walked": 0}
    d = bench.path_description(mixed)
    assert "27 exact fp64 grid searches" in d and "3 searches through the f16" in d


def test_committed_bench_line_dtype_matches_its_counters():
    """The round-6 GPU bench lines (profiles/r06*/*bench*.log) carry step_paths, and the last one's
    dtype is the description of exactly those counters."""
    import json
    logs = sorted(ROOT.glob("profiles/r06*/*bench*.log"))
    lines = [json.loads(x) for f in logs for x in f.read_text().splitlines() if x.startswith("{")]
    lines = [x for x in lines if "step_paths" in x]
    if not lines:
        pytest.skip("no round-6 bench line with step_paths committed yet")
    bench = _bench_module()
    last = lines[-1]
    sp = {k: last["step_paths"][k] for k in ("run_grid_searches", "run_bundle_searches", "run_certified",
                                             "run_walked")}
    assert last["dtype"] == "f64 (" + bench.path_description(sp) + ")"
