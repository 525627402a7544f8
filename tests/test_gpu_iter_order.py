"""The fused grid iteration's dispatch order (icp_kernels.h IterOrder, ICP_ITER2_ORDER): which
block takes which strand changes no bit of any result, and every strand is taken exactly once.

The column fold after a fused launch sorts each XCD's strands by the walker counts that launch
left (heavy first), and the next fused launch reads its strand from that table instead of
xcd_row.  Each setting runs in its own process (the knobs are read once a process), the
processes side by side, once for the module:

  ICP_ITER2_ORDER = 0 (xcd_row), 1, 2, 3 (the three forms), 5, 6, 7 (the same tables light-first:
  the adversarial order), and the separate-kernel path (ICP_GRID_ITER=0)

on two shapes:

  A  2^16 + 37 points (test_gpu_iter_small.py's), ICP_ITER_XCD_L=4: runs of 16 strands; the 2,050
     strands give 2,048 blocks in xcd_row's bijection and 2 past it, which keep their index
  B  49,152 + 5 points, the default mapping: one run an XCD, 1,537 strands (8 x 192 + 1: the XCDs'
     lists differ in length).  icp_run keeps a scene in slot order, and so reaches the fused
     kernel, only above 49,152 points: this is the smallest such scene.  A scene of 3,000 points
     runs alongside (the one-launch loop: no fused launch, no table), bitwise equal as well.

Every setting runs the same sequence on one context per shape -- 8 iterations; icp_set_scene with
the other shape's size and 8 more; the first scene again; a gated run (icp_set_max_distance); an
ungated one -- and each step's error trace, transform, registered scene and correspondences equal
order 0's bit for bit, and the separate-kernel path's.  A table never outlives its run, so the
steps after the first are the invalidation cases.

Exactly-once coverage is a condition, not a tolerance: a run of 8 iterations is one first search
and 7 fused launches, each of which counts every query as certified or walked, so
run_certified + run_walked grows by 7 n a run whatever the order.

Two ranks: tests/dist_engine_worker.py on shards of a 131,072-point scene, order 3 against order
0, every rank's record equal.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NA = (1 << 16) + 37
NB = 49152 + 5
NSMALL = 3000
ITERS = 8
FUSED = ITERS - 1  # (fused launches a run: every iteration but the first search)
ORDERS = [0, 1, 2, 3, 5, 6, 7]
SHAPES = {"A": {"ICP_ITER_XCD_L": "4"}, "B": {}}
STEPS = ["run", "other_n", "back", "gated", "ungated"]
KEYS = ("errs", "xf", "scene", "idx")

SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import icp_amd
from test_gpu_iter_order import ITERS, STEPS, NSMALL, scenes
shape, path = sys.argv[3], sys.argv[4]
m, p, p_other = scenes(shape)
out = {}
def record(ctx, step, res, errs, before):
    st = ctx.stats()
    out[step + "_errs"] = errs
    out[step + "_xf"] = np.concatenate([[res.s], np.array(res.R[:]), np.array(res.t[:])])
    out[step + "_scene"] = ctx.get_scene()
    out[step + "_idx"] = ctx.get_indices()
    now = np.array([st["run_certified"], st["run_walked"]])
    out[step + "_counts"] = now - before
    return now
with icp_amd.Context(0) as ctx:
    ctx.set_nn_variant(icp_amd.VARIANT_GRID)
    ctx.set_allow_unequal(True)
    ctx.set_model(m)
    c = np.zeros(2, dtype=np.int64)
    for step in STEPS:
        if step == "run" or step == "back":
            ctx.set_scene(p)
        elif step == "other_n":
            ctx.set_scene(p_other)
        elif step == "gated":
            ctx.set_max_distance(1.0)
        else:
            ctx.set_max_distance(0.0)
        res, errs = ctx.run(ITERS, -1.0)
        c = record(ctx, step, res, errs, c)
    if shape == "B":
        ctx.set_scene(p[:NSMALL])
        res, errs = ctx.run(ITERS, -1.0)
        record(ctx, "small", res, errs, c)
np.savez(path, **out)
print("iter order ok")
"""


def scenes(shape):
    """(model, scene, a scene of the other shape's size against the same model)"""
    sys.path.insert(0, os.path.join(ROOT, "iterative-closest-point_amd"))
    import icp_amd
    n, other = (NA, NB) if shape == "A" else (NB, NA)
    m, p = icp_amd.synthetic_pair(max(n, other), seed=41, angle_deg=4.0)
    rng = np.random.default_rng(5)
    return m, np.ascontiguousarray(p[:n]), np.ascontiguousarray(p[rng.permutation(len(p))[:other]])


def start(tmp, shape, name, env):
    out = str(tmp / f"iter_order_{shape}_{name}.npz")
    cmd = [sys.executable, "-c", SCRIPT, os.path.join(ROOT, "iterative-closest-point_amd"), HERE, shape, out]
    return out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                 env=dict(os.environ, **SHAPES[shape], **env))


@pytest.fixture(scope="module")
def settings(icp_lib, tmp_path_factory):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    tmp = tmp_path_factory.mktemp("iter_order")
    got = {}
    for shape in SHAPES:  # (8 processes at a time)
        procs = {o: start(tmp, shape, f"o{o}", {"ICP_ITER2_ORDER": str(o)}) for o in ORDERS}
        procs["separate"] = start(tmp, shape, "separate", {"ICP_GRID_ITER": "0"})
        for name, (out, pr) in procs.items():
            text, _ = pr.communicate(timeout=300)
            assert pr.returncode == 0 and "iter order ok" in text, (shape, name, text[-3000:])
            got[shape, name] = dict(np.load(out))
    return got


def steps_of(shape):
    return STEPS + (["small"] if shape == "B" else [])


@pytest.mark.parametrize("order", ORDERS[1:])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_order_changes_no_bit(settings, shape, order):
    a, b = settings[shape, 0], settings[shape, order]
    for step in steps_of(shape):
        for k in KEYS:
            assert np.array_equal(a[f"{step}_{k}"], b[f"{step}_{k}"]), (step, k)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_order_equals_separate_kernels_bitwise(settings, shape, order):
    a, b = settings[shape, "separate"], settings[shape, order]
    for step in steps_of(shape):
        for k in KEYS:
            assert np.array_equal(a[f"{step}_{k}"], b[f"{step}_{k}"]), (step, k)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_query_counted_exactly_once_a_launch(settings, shape, order):
    a = settings[shape, order]
    n, other = (NA, NB) if shape == "A" else (NB, NA)
    for step, pts in (("run", n), ("other_n", other), ("back", n), ("ungated", n)):
        cert, walked = a[step + "_counts"]
        assert walked > 0 and cert > 0, (step, cert, walked)  # (the fused kernel ran, with its certificate)
        assert cert + walked == pts * FUSED, (step, cert, walked, pts * FUSED)
        assert np.array_equal(a[step + "_counts"], settings[shape, 0][step + "_counts"]), step
    assert a["gated_counts"].sum() == 0  # (the gated loop: no fused launch)


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_shards_equal_order_0(icp_lib, tmp_path):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    worker = os.path.join(HERE, "dist_engine_worker.py")
    procs = {}
    for order in (0, 3):
        out = str(tmp_path / f"ranks_o{order}.json")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
               "127.0.0.1", "--master-port", str(free_port()), worker, out, "synthetic131072", "6", "-1.0", "0"]
        env = dict(os.environ, OMP_NUM_THREADS="1", ICP_ITER2_ORDER=str(order))
        procs[order] = out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    got = {}
    for order, (out, pr) in procs.items():
        text, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, text[-3000:]
        with open(out) as f:
            got[order] = json.load(f)
    assert [r["rank"] for r in got[3]] == [0, 1]
    assert got[0] == got[3]
