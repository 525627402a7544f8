"""Every cell of the kept-pairs loop's options -- metric (point, plane, symmetric, plane-to-plane) x gate x
trim x robust kind x one-to-one, 128 cells -- against tests/kept_ref.py, the loop restated once with all of
them (tests/test_kept_ref.py checks that reference and these inputs on the CPU).

Tolerances are the project's (test_gpu_unique.check_against_ref, test_gpu_symm): iterations, the K trace and
k, K+ and the mask exact and mask.sum() == K; err rel 1e-9 or within (1e-9 x extent)^2; s and R abs 1e-9;
t and the scene abs 1e-9 x extent; W rel 1e-9; C's first entry bit for bit (the first iteration's d2 has
the oracle's bits) and the rest rel 1e-9.
  a. every cell on a fresh context at 257 points
  b. the 16 cells with the gate, the trim and one-to-one on at 4097 (one point past kRedSingle: the moments
     fold several workgroups' rows, the selection leaves its single-workgroup form)
  c. no state survives a run: one context per metric walks its 32 cells changing one option at a time,
     forwards and backwards, through the public setters alone; every output has the bits of the same cell
     on a fresh context (same library, same inputs, same order of the sums; the only atomic is an
     integer minimum)
  d. two ranks (HostAllReduce) on the 32 cells without one-to-one and with no weights or Tukey's
Each cell prints K, K+ and err beside the reference's and "dev": the cell's deviation from the reference
per quantity, in the units of its tolerance.
Measured on one MI355X, the worst dev over the 176 compared runs (a, b and d): err 2.1e-12, R 1.3e-12,
t 1.7e-12 and the scene 4.1e-12 (all four in the ungated, untrimmed, unweighted one-sided plane cell, where the
fp64 reference is 2.1e-12, 1.2e-12, 1.8e-12 and 4.1e-12 from its longdouble twin), s 2.1e-15, W 2.6e-14,
C 2.5e-14: under 0.5 % of the 1e-9 allowed.
"""
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import gicp_ref as GI
import kept_ref as KR
from test_gpu_gated import HostAllReduce

pytestmark = pytest.mark.gpu

DEFAULTS = dict(dmax=0.0, trim=None, robust=None, one_to_one=False)


def kind_of(amd, robust):
    """kept_ref's (kind, k) or None -> set_robust's arguments."""
    if robust is None:
        return amd.ROBUST_NONE, 0.0
    names = {v: k for k, v in KR.KINDS.items()}
    return {"huber": amd.ROBUST_HUBER, "tukey": amd.ROBUST_TUKEY, "cauchy": amd.ROBUST_CAUCHY}[names[robust[0]]], robust[1]


def set_option(amd, ctx, name, value):
    """One option through its public setter, on or off."""
    if name == "dmax":
        ctx.set_max_distance(value)  # (0: off)
    elif name == "trim":
        ctx.set_trim(1.0 if value is None else value)
    elif name == "robust":
        ctx.set_robust(*kind_of(amd, value))
    else:
        ctx.set_one_to_one(bool(value))


def set_model_and_metric(amd, ctx, metric, m, nrm):
    """The model, its normals and the metric's switches, the other form off before the one goes on."""
    ctx.set_model(m)
    if metric == "point":
        ctx.set_metric(amd.METRIC_POINT_TO_POINT)
        return
    ctx.set_model_normals(nrm)
    ctx.set_metric(amd.METRIC_POINT_TO_PLANE)
    ctx.set_plane_symmetric(False)
    ctx.set_plane_to_plane(0.0)
    if metric == "symm":
        ctx.set_plane_symmetric(True)
    elif metric == "gicp":
        ctx.set_plane_to_plane(GI.EPS)


def set_scene(ctx, metric, p, U0, np_total=None):
    ctx.set_scene(p, np_total=np_total)
    if metric in ("symm", "gicp"):
        ctx.set_scene_normals(U0)


def run_and_collect(amd, ctx):
    """-> dict(iterations, errs, scene, R, t, s, and what the run left: K (trace), mask, k; W, Kpos; C)."""
    res, errs = ctx.run(KR.MATRIX_ITERS, -1.0)
    out = dict(iterations=res.iterations, errs=errs, scene=ctx.get_scene(), R=np.array(res.R).reshape(3, 3),
               t=np.array(res.t), s=np.float64(res.s))
    try:
        out["mask"], out["k"] = ctx.inliers()
        out["K"] = ctx.inlier_trace()
    except amd.ICPError as e:  # (no gate, trim or one-to-one since set_scene)
        assert e.code == amd.ICP_E_NO_MODEL
    try:
        out["W"], out["Kpos"] = ctx.robust_trace()
    except amd.ICPError as e:
        assert e.code == amd.ICP_E_NO_MODEL
    try:
        out["C"] = ctx.trim_trace()
    except amd.ICPError as e:
        assert e.code == amd.ICP_E_NO_MODEL
    return out


_fresh = {}


def fresh(amd, n, cell):
    """The cell on a context of its own that sets only what the cell has on; once a session."""
    if (n, cell) not in _fresh:
        m, nrm, p, U0 = KR.matrix_case(n)
        with amd.Context() as ctx:
            set_model_and_metric(amd, ctx, cell[0], m, nrm)
            set_scene(ctx, cell[0], p, U0)
            for name, value in KR.cell_options(cell, n).items():
                if value != DEFAULTS[name]:
                    set_option(amd, ctx, name, value)
            _fresh[(n, cell)] = run_and_collect(amd, ctx)
    return _fresh[(n, cell)]


def check_against_ref(n, cell, out, r, tag=""):
    _metric, gate, trim, kname, uniq = cell
    extent = float(np.abs(KR.matrix_case(n)[0]).max())
    print(tag + KR.cell_id(cell), "K", list(out.get("K", [])), "ref", r["K"], "K+", list(out.get("Kpos", [])), "ref", r["Kpos"],
          "err", out["errs"], "ref", np.asarray(r["err"]))
    assert ("K" in out) == (gate or trim or uniq) and ("W" in out) == (kname != "none") and ("C" in out) == trim
    assert r["status"] == "ok" and out["iterations"] == r["iterations"] == KR.MATRIX_ITERS
    if "K" in out:
        assert list(out["K"]) == r["K"] and out["k"] == r["K"][-1]
        np.testing.assert_array_equal(out["mask"], r["mask"])
        assert out["mask"].sum() == out["k"]
    else:
        assert r["K"] == [n] * KR.MATRIX_ITERS
    ref_err = np.asarray(r["err"], dtype=np.float64)
    de = np.abs(out["errs"] - ref_err)
    dev = dict(err=float(np.max(de / np.abs(ref_err))), s=abs(float(out["s"]) - float(r["s"])),
               R=float(np.abs(out["R"] - r["R"]).max()), t=float(np.abs(out["t"] - r["t"]).max()) / extent,
               scene=float(np.abs(out["scene"] - r["new_p"]).max()) / extent)
    if "W" in out:
        assert list(out["Kpos"]) == r["Kpos"]
        ref_w = np.array(r["W"], dtype=np.float64)
        dev["W"] = float(np.max(np.abs(out["W"] - ref_w) / ref_w))
    if "C" in out:
        ref_c = np.array(r["C"], dtype=np.float64)
        assert out["C"][0] == ref_c[0]
        dev["C"] = float(np.max(np.abs(out["C"] - ref_c) / ref_c))
    print("   dev", " ".join("%s=%.2e" % kv for kv in dev.items()))
    assert np.all((de <= 1e-9 * np.abs(ref_err)) | (de <= (1e-9 * extent) ** 2)), (out["errs"], ref_err)
    for name in ("s", "R", "t", "scene", "W", "C"):
        assert dev.get(name, 0.0) <= 1e-9, (name, dev[name])


# a. every cell, fresh context
@pytest.mark.parametrize("uniq", [False, True], ids=["all", "one_to_one"])
@pytest.mark.parametrize("metric", KR.METRICS)
def test_every_cell_at_257(icp_lib, oracle, metric, uniq):
    for cell in KR.cells(metric):
        if cell[4] == uniq:
            check_against_ref(KR.MATRIX_N, cell, fresh(icp_lib, KR.MATRIX_N, cell), KR.reference(oracle, KR.MATRIX_N, cell))


# b. the everything-on row at 4097
@pytest.mark.parametrize("cell", KR.row_cells(), ids=KR.cell_id)
def test_everything_on_at_4097(icp_lib, oracle, cell):
    r = KR.reference(oracle, KR.ROW_N, cell)
    assert r["K"] == KR.ROW_K[cell]
    check_against_ref(KR.ROW_N, cell, fresh(icp_lib, KR.ROW_N, cell), r)


# c. no state survives a run
def gray_walk(metric):
    """The metric's 32 cells in a reflected Gray order: neighbours differ in one option (the robust kind
    by one step of none, Huber, Tukey, Cauchy)."""
    kinds = list(KR.KINDS)
    seq = [()]
    for radix in (2, 2, 4, 2):
        seq = [pre + (d,) for i, pre in enumerate(seq) for d in (range(radix) if i % 2 == 0 else reversed(range(radix)))]
    return [(metric, bool(g), bool(t), kinds[k], bool(u)) for g, t, k, u in seq]


def test_the_walk_changes_one_option_at_a_time():
    for metric in KR.METRICS:
        walk = gray_walk(metric)
        assert sorted(walk) == sorted(KR.cells(metric))
        for a, b in zip(walk, walk[1:]):
            assert sum(x != y for x, y in zip(a, b)) == 1


@pytest.mark.parametrize("order", ["forwards", "backwards"])
@pytest.mark.parametrize("metric", KR.METRICS)
def test_no_state_survives_a_run(icp_lib, metric, order):
    amd = icp_lib
    n = KR.MATRIX_N
    m, nrm, p, U0 = KR.matrix_case(n)
    walk = gray_walk(metric)
    if order == "backwards":
        walk = walk[::-1]
    current = dict(DEFAULTS)
    with amd.Context() as ctx:
        set_model_and_metric(amd, ctx, metric, m, nrm)
        for cell in walk:
            set_scene(ctx, metric, p, U0)
            changed = []
            for name, value in KR.cell_options(cell, n).items():
                if value != current[name]:
                    set_option(amd, ctx, name, value)
                    current[name] = value
                    changed.append(name)
            out, want = run_and_collect(amd, ctx), fresh(amd, n, cell)
            print(KR.cell_id(cell), "changed", changed, "K", list(out.get("K", [])), "K+", list(out.get("Kpos", [])), "err",
                  out["errs"])
            assert sorted(out) == sorted(want), KR.cell_id(cell)
            for key in out:
                a, b = np.asarray(out[key]), np.asarray(want[key])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (KR.cell_id(cell), key)


# d. two ranks
def run_sharded(amd, n, cell, world):
    m, nrm, p, U0 = KR.matrix_case(n)
    red = HostAllReduce(world)
    results, errors = [None] * world, []

    def worker(r):
        try:
            b, c = amd.shard_range(n, r, world)
            with amd.Context(0, 0, rank=r, world_size=world, host_allreduce=red.for_rank(r)) as ctx:
                set_model_and_metric(amd, ctx, cell[0], m, nrm)
                set_scene(ctx, cell[0], p[b:b + c], U0[b:b + c], np_total=n)
                for name, value in KR.cell_options(cell, n).items():
                    if value != DEFAULTS[name]:
                        set_option(amd, ctx, name, value)
                results[r] = run_and_collect(amd, ctx)
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    return results


@pytest.mark.parametrize("metric", KR.METRICS)
def test_two_ranks(icp_lib, oracle, metric):
    n = KR.MATRIX_N
    for cell in KR.cells(metric):
        if cell[4] or cell[3] not in ("none", "tukey"):
            continue
        ranks = run_sharded(icp_lib, n, cell, 2)
        for o in ranks[1:]:  # identical decisions and solves on every rank
            for key in ("errs", "R", "t", "s", "K", "k", "W", "Kpos", "C"):
                assert (key in o) == (key in ranks[0])
                if key in o:
                    np.testing.assert_array_equal(o[key], ranks[0][key], err_msg=key)
        whole = dict(ranks[0], scene=np.concatenate([o["scene"] for o in ranks]))
        if "mask" in whole:
            whole["mask"] = np.concatenate([o["mask"] for o in ranks])
        check_against_ref(n, cell, whole, KR.reference(oracle, n, cell), tag="world2 ")
