"""The canonical schedule's iteration fold (icp_canon.hip canon_fold_cols_kernel) with its loads
batched -- a thread's rows in one pass of unconditional loads (indices clamped, the conditions
selecting afterwards), the 18 column sums kept in registers for the steps, the error step's
state words loaded with them (icp_fold.h err_step_body) -- and with the error step's host side
(the error, the mirrored far count and queue size the host's policy reads, the flags and the
ticket) written by the residual column's workgroup as soon as that column is summed
(err_publish_running), while the last workgroup's thread 0 steps the device state; a step that
ends the run is published by that thread, whole mirror and all.

The reference is the one-workgroup fold (ICP_FOLD_ONE=1, canon_fold_kernel: its own row loads, the
sums through LDS).  Each setting runs in its own child process (the switch is
read once a process) and the two agree bit for bit: error trace, per-iteration index digests,
final scene, the result's transform, icp_get_transform, iterations / converged and the
statistics (the search counters the state carries and the run's paths).

  sizes    the smallest scenes the canonical schedule takes (more than 49,152 points; a strand is
           a chunk of 32 points, a row four strands), at the fold's edges with 512 threads and 8
           rows a thread, 6 iterations of the GRID variant each:
             49,153   R = 385    not every thread has a row
             65,536   R = 512    one row a thread
             65,573   R = 513    thread 0 alone has a second row; its strands run past S
             262,145  R = 2,049
             524,291  R = 4,096  S = 16,384: every thread's eight rows
  stop     65,573 points, the threshold between the 4th and 5th error of a fixed 8-iteration
           run: the run stops at 5 iterations, converged, on the fixed run's prefix (four steps
           published early, the last with the whole-state mirror by the stepping thread, which
           also publishes the finished state for the iterations queued behind it).  A further run(3) with the same threshold goes on from
           there -- one iteration, the fixed run's 6th error up to rounding -- and differs in
           nothing between the forms.
  auto     65,573 points, the AUTO variant (its policy reads the mirrored far count and queue
           size while the run goes on): the run's paths equal between the forms and across three
           registrations of one process.
  ring     200 consecutive set_scene + run(2) on one context: the ticket ring wraps; every call
           returns 2 iterations and the first call's trace.
  rank     65,573 points through a 1-rank communicator (the fold's sums only, the all-reduce,
           then err_horn_step_kernel): the run without ranks, bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [49153, 65536, 65573, 262145, 524291]
N = 65573
ITERS = 6
FIXED = 8
RING = 200
KEYS = ("errs", "dig", "scene", "xf", "tot", "it", "st")
STAT_KEYS = ("ambiguous", "level1_queued", "level1_unrecovered", "grid_fallback", "iterations", "last_filter",
             "run_bundle_searches", "run_grid_searches", "run_certified", "run_walked", "run_path_bits")

SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import icp_amd
from test_gpu_fold_publish import SIZES, N, ITERS, FIXED, RING, STAT_KEYS, pair

out = {}

def put(tag, ctx, res, errs, digests):
    st = ctx.stats()
    s, R, t = ctx.transform()
    out[tag + "_errs"] = errs
    out[tag + "_dig"] = ctx.index_digest(digests) if digests else np.zeros(0)
    out[tag + "_scene"] = ctx.get_scene()
    out[tag + "_xf"] = np.concatenate([[res.s], np.array(res.R[:]), np.array(res.t[:])])
    out[tag + "_tot"] = np.concatenate([[s], R.ravel(), t])
    out[tag + "_it"] = np.array([res.iterations, res.converged])
    out[tag + "_st"] = np.array([int(st[k]) for k in STAT_KEYS], dtype=np.uint64)

def registration(tag, ctx, m, p, iters, thr=-1.0):
    ctx.set_model(m)
    ctx.set_scene(p)
    ctx.set_index_digest(iters)
    ctx.reset_stats()
    res, errs = ctx.run(iters, thr)
    put(tag, ctx, res, errs, res.iterations)
    return errs

for n in SIZES:
    m, p = pair(n)
    with icp_amd.Context(0) as ctx:
        ctx.set_nn_variant(icp_amd.VARIANT_GRID)
        registration(f"n{n}", ctx, m, p, ITERS)

m, p = pair(N)
with icp_amd.Context(0) as ctx:
    ctx.set_nn_variant(icp_amd.VARIANT_GRID)
    errs = registration("fixed", ctx, m, p, FIXED)
    thr = 0.5 * (errs[3] + errs[4])
    out["thr"] = np.array([thr])
    registration("stop", ctx, m, p, FIXED, thr)
    ctx.reset_stats()
    res, more = ctx.run(3, thr)
    put("more", ctx, res, more, 0)

with icp_amd.Context(0) as ctx:  # (AUTO, the default variant)
    for rep in range(3):
        registration(f"auto{rep}", ctx, m, p, ITERS)

with icp_amd.Context(0) as ctx:
    ctx.set_nn_variant(icp_amd.VARIANT_GRID)
    ctx.set_model(m)
    its, traces = [], []
    for _ in range(RING):
        ctx.set_scene(p)
        res, errs = ctx.run(2, -1.0)
        its.append(res.iterations)
        traces.append(np.resize(errs, 2))
    out["ring_it"] = np.array(its)
    out["ring_errs"] = np.array(traces)

if sys.argv[4] == "rank":
    with icp_amd.Context(0, icp_amd.NN_CERTIFIED, rank=0, world_size=1, rccl_id=icp_amd.rccl_unique_id()) as ctx:
        ctx.set_nn_variant(icp_amd.VARIANT_GRID)
        registration("rank", ctx, m, p, ITERS)
np.savez(sys.argv[3], **out)
print("fold publish ok")
"""


def pair(n):
    import icp_amd
    return icp_amd.synthetic_pair(n, seed=41, angle_deg=4.0)


def run_setting(tmp_path, name, fold_one, rank):
    out = str(tmp_path / f"fold_publish_{name}.npz")
    env = {k: v for k, v in os.environ.items() if k != "ICP_FOLD_ONE"}
    if fold_one:
        env["ICP_FOLD_ONE"] = "1"
    r = subprocess.run([sys.executable, "-c", SCRIPT, os.path.join(ROOT, "iterative-closest-point_amd"),
                        os.path.join(ROOT, "tests"), out, "rank" if rank else "-"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "fold publish ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def forms(icp_lib, tmp_path_factory):
    if icp_lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    tmp = tmp_path_factory.mktemp("fold_publish")
    return {"cols": run_setting(tmp, "cols", False, True), "one": run_setting(tmp, "one", True, False)}


def same(a, ta, b, tb, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[f"{ta}_{k}"], b[f"{tb}_{k}"]), (ta, tb, k)


def stat(d, tag, name):
    return int(d[tag + "_st"][STAT_KEYS.index(name)])


@pytest.mark.parametrize("n", SIZES)
def test_fold_forms_agree_bitwise(forms, n):
    a, b = forms["cols"], forms["one"]
    tag = f"n{n}"
    assert tuple(a[tag + "_it"]) == (ITERS, 0) and len(a[tag + "_errs"]) == ITERS
    assert stat(a, tag, "run_grid_searches") == ITERS  # (the grid's searches: the canonical schedule)
    assert np.all(np.isfinite(a[tag + "_errs"])) and a[tag + "_errs"][-1] < a[tag + "_errs"][0]
    same(a, tag, b, tag)


def test_threshold_stop_mid_run(forms):
    a, b = forms["cols"], forms["one"]
    errs = a["fixed_errs"]
    assert len(errs) == FIXED and errs[2] > errs[3] > errs[4] > errs[5]  # (strictly decreasing there)
    assert errs[4] < a["thr"][0] < errs[3]
    assert tuple(a["stop_it"]) == (5, 1)
    assert np.array_equal(a["stop_errs"], errs[:5])
    same(a, "fixed", b, "fixed")
    same(a, "stop", b, "stop")
    # the run went on from the stopped state: one iteration, under the threshold at once -- the
    # fixed run's next error up to rounding (a run's first iteration takes the two-pass moments,
    # the fixed run's 6th the one-pass ones: the tolerance the smoke run gives the oracle)
    assert tuple(a["more_it"]) == (1, 1)
    np.testing.assert_allclose(a["more_errs"], errs[5:6], rtol=1e-9)
    same(a, "more", b, "more", keys=("errs", "scene", "xf", "tot", "it", "st"))


def test_mirrored_counts_steer_the_same_paths(forms):
    a, b = forms["cols"], forms["one"]
    for rep in range(3):
        for name in ("run_path_bits", "run_grid_searches", "run_bundle_searches"):
            assert stat(a, f"auto{rep}", name) == stat(b, f"auto{rep}", name), (rep, name)
            assert stat(a, f"auto{rep}", name) == stat(a, "auto0", name), (rep, name)
        same(a, f"auto{rep}", b, f"auto{rep}")
        same(a, f"auto{rep}", a, "auto0")
    assert stat(a, "auto0", "run_grid_searches") + stat(a, "auto0", "run_bundle_searches") == ITERS


def test_ticket_ring(forms):
    for d in forms.values():
        assert d["ring_it"].shape == (RING,) and np.all(d["ring_it"] == 2)
        assert np.all(d["ring_errs"] == d["ring_errs"][0])
    assert np.array_equal(forms["cols"]["ring_errs"][0], forms["one"]["ring_errs"][0])
    assert np.array_equal(forms["cols"]["ring_errs"][0], forms["cols"][f"n{N}_errs"][:2])


def test_rank_path_equals_no_ranks(forms):
    a = forms["cols"]
    assert tuple(a["rank_it"]) == (ITERS, 0)
    same(a, "rank", a, f"n{N}", keys=("errs", "dig", "scene", "xf", "tot", "it"))
    same(a, "rank", forms["one"], f"n{N}", keys=("errs", "dig", "scene", "xf", "tot", "it"))
