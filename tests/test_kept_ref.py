"""tests/kept_ref.py checked on the CPU, before tests/test_gpu_kept_matrix.py relies on it.

a. The composed reference restates the seven feature references: on one of each module's own cases at
   257 points, with that module's own options, kept_ref returns the feature reference's bits in every
   field the two share, and its margins fold to the feature reference's one.  No field needed an
   exception: where the feature references sum in different ways (plane_ref's a^T a against the weighted
   (a w)^T a of robust_ref and symm_ref; the oracle's Horn against robust_ref.weighted_horn) kept_ref
   takes the expression of the module that owns the cell.
b. The matrix inputs (kept_ref.matrix_case, DMAX, TRIM, SCALE) are fit for an exact comparison of masks
   and counts: every cell of metric x gate x trim x weights x one-to-one at 257 points and the
   everything-on row at 4097.

Measured, fp64 against longdouble (the bound is GAP = 1e-11, 1 % of the GPU comparison's 1e-9):
  257, 128 cells: err rel 2.1e-12, R 1.2e-12, t 1.8e-12 and new_p 4.1e-12 of the extent (all four in the
    ungated, untrimmed, unweighted one-sided plane cell, which keeps its outlier quarter), s 4.3e-16,
    W rel 2.6e-14; no err needed the floor
  4097, 16 cells: err rel 5.6e-14, R 4.8e-16, s 2.1e-15, t 8.1e-17, new_p 7.1e-15, W rel 9.7e-15
Smallest margins (the floor is 1e-6):
  257: gate 2.1e-5, trim 9.4e-5, one-to-one 9.3e-5, k 1.4e-4
  4097: gate 3.2e-5, trim 3.2e-5, one-to-one 5.4e-6, k 7.1e-5
K is at least 87 and K+ at least 54 at 257 (1,824 and 1,291 at 4097).
The issue's starting values that moved: the trim 0.45 -> 0.414 at 257 (T = 106: under the gate the one-sided
plane metric with Tukey weights keeps 104, 106, 103, 100 pairs, so only T <= 106 lets its trim bind while
the gate's first 104 stay below T) and 0.55 -> 0.627 at 4097 (T = 2568 above the gate's first 2543); Tukey's k
for the point metric 0.08 -> 0.06 (k = dmax gives no gated pair the weight 0) and for the symmetric one
0.2 -> 0.08 (as the point metric's, twice the one-sided plane's: |n| <= 2); Huber's k for the point metric
at 257 0.03 -> 0.031 (the k margin was 6.0e-6) and for the plane metric at 4097 0.01 -> 0.012 (the
one-to-one margin was 4.2e-6).

Both cuts bind in a gate-and-trim cell: an iteration's cut is min(D, C), so the gate binds where C > D
and the trim where C <= D -- asserted on the C list in every cell.  Without one-to-one that is the K
list's K < T and K == T (no ties at the cut: the trim margin), asserted as well; with one-to-one K
counts the winners among the pairs under the cut and stays below T either way, so there the C list
alone says which cut bound.  All four metrics give both within 4 iterations, at both sizes.
"""
import numpy as np
import pytest

import gated_ref as G
import gicp_ref as GI
import kept_ref as KR
import plane_ref as P
import robust_ref as RB
import symm_ref as S
import trim_ref as TR
import unique_ref as U

GAP = 1e-11  # test_robust_ref.py's: 1 % of the GPU comparison's 1e-9
FLOOR = 1e-6  # the margins' (test_unique_ref.py, test_trim_ref.py)
SHARED = ("new_p", "err", "K", "mask", "s", "R", "t", "Q", "iterations", "status", "W", "Kpos", "C", "T", "min_pivot",
          "fail_iter")


def same_bits(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, name
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        assert a.dtype == b.dtype == np.float64, (name, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), name
    else:
        np.testing.assert_array_equal(a, b, err_msg=name)


def restates(ours, theirs, expect):
    """Every shared field bit for bit (`expect`: the fields that must be among them), and the margins."""
    shared = [k for k in SHARED if k in ours and k in theirs]
    assert set(expect) <= set(shared), (expect, shared)
    assert theirs["status"] == "ok" and theirs["iterations"] > 0
    for k in shared:
        same_bits(ours[k], theirs[k], k)
    if "margin" in theirs:
        assert min(ours["gate_margin"], ours["trim_margin"], ours["unique_margin"]) == theirs["margin"]
    return shared


BASE = ("new_p", "err", "K", "mask", "s", "R", "t", "iterations", "status")


# ---- a. the seven, and the plain loop ----------------------------------------------------------

def test_restates_gated_ref(oracle):
    m, p, dmax, r = G.reference(oracle, ("bite", 257, 0.08))
    a = KR.kept_ref(oracle, m, p, metric="point", dmax=dmax, max_iter=G.BITES_ITERS, threshold=-1.0)
    restates(a, r, BASE)
    assert a["K"][0] == G.BITES[(257, 0.08)][0] and a["trim_margin"] == a["unique_margin"] == np.inf


def test_restates_the_untrimmed_unweighted_point_loop(oracle):
    m, p = G.synth(257, 357, 0.25)
    r = G.gated_ref(oracle, m, p, np.inf, 6, -1.0)
    a = KR.kept_ref(oracle, m, p, metric="point", max_iter=6, threshold=-1.0)
    restates(a, r, BASE)
    assert a["K"] == [257] * 6 and a["mask"].all() and a["gate_margin"] == np.inf
    np.testing.assert_allclose(a["err"], oracle.icp(m, p, 6)["err"][:6], rtol=1e-12)


def test_restates_trimmed_ref(oracle):
    m, p, f, dmax, iters, thr, r = TR.reference(oracle, ("noisy", 257, 0.5))
    a = KR.kept_ref(oracle, m, p, metric="point", dmax=dmax, trim=f, max_iter=iters, threshold=thr)
    restates(a, r, BASE + ("C", "T"))
    assert a["K"] == [TR.NOISY[(257, 0.5)]] * iters


def test_restates_one_to_one_ref(oracle):
    m, p, dmax, f, iters, r = U.reference(oracle, ("noisy", 257, "both"))
    a = KR.kept_ref(oracle, m, p, metric="point", dmax=dmax, trim=f, one_to_one=True, max_iter=iters, threshold=-1.0)
    restates(a, r, BASE + ("T",))
    assert a["K"] == U.NOISY[(257, "both")]


def test_restates_plane_ref(oracle):
    m, nrm, p, dmax, r = P.reference(oracle, ("gate", 257, 0.08))
    a = KR.kept_ref(oracle, m, p, metric="plane", N=nrm, dmax=dmax, max_iter=P.GATES_ITERS, threshold=-1.0)
    restates(a, r, BASE + ("min_pivot",))
    assert a["K"] == P.GATES[(257, 0.08)]


@pytest.mark.parametrize("kname", list(RB.KINDS))
@pytest.mark.parametrize("metric", RB.METRICS)
def test_restates_robust_ref(oracle, metric, kname):
    kind = RB.KINDS[kname]
    m, nrm, p, dmax, _kind, k, r = RB.reference(oracle, ("size", metric, kind, 257))
    a = KR.kept_ref(oracle, m, p, metric=metric, N=nrm, dmax=dmax, robust=(kind, k), max_iter=RB.SIZES_ITERS, threshold=-1.0)
    restates(a, r, BASE + ("W", "Kpos"))
    if kind != RB.CAUCHY:
        assert a["k_margin"] == r["kmargin"]


@pytest.mark.parametrize("key", ["trim", "tukey"])
def test_restates_symm_ref(oracle, key):
    m, nrm, p, U0, dmax, r = S.reference(oracle, (key, 257, 0.08))
    more = dict(trim=S.TRIM) if key == "trim" else dict(robust=(RB.TUKEY, S.TUKEY_K))
    a = KR.kept_ref(oracle, m, p, metric="symm", N=nrm, U0=U0, dmax=dmax, max_iter=S.GATES_ITERS, threshold=-1.0, **more)
    restates(a, r, BASE + ("Q", "W", "Kpos", "C", "min_pivot"))
    assert len(a["C"]) == (S.GATES_ITERS if key == "trim" else 0) and len(a["W"]) == (0 if key == "trim" else S.GATES_ITERS)


@pytest.mark.parametrize("key", ["trim", "tukey"])
def test_restates_gicp_ref(oracle, key):
    """gicp_ref's named trim and Tukey cases are 2,049 points: its generator and options at 257."""
    m, nrm, p = P.gate_case(257)
    U0 = S.scene_normals_of(nrm)
    more = dict(trim=GI.TRIM) if key == "trim" else dict(robust=(RB.TUKEY, GI.TUKEY_K))
    r = GI.gicp_ref(oracle, m, nrm, p, U0, GI.EPS, GI.GATE[1], GI.GATE_ITERS, -1.0, **more)
    a = KR.kept_ref(oracle, m, p, metric="gicp", N=nrm, U0=U0, eps=GI.EPS, dmax=GI.GATE[1], max_iter=GI.GATE_ITERS,
                    threshold=-1.0, **more)
    restates(a, r, BASE + ("Q", "W", "Kpos", "C", "min_pivot"))
    if key == "tukey":
        assert a["k_margin"] == r["wmargin"] and any(kp < k for kp, k in zip(a["Kpos"], a["K"]))


def test_the_wide_one_to_one_mask_is_the_fp64_rule(oracle):
    """kept_ref._unique hands unique_ref.unique_mask ranks when d2 is wider than its table: the same mask
    as on the values, ties kept whole and a NaN never kept."""
    r = np.random.default_rng(3)
    idx = r.integers(0, 40, size=300)
    d2 = r.random(300)
    d2[10], idx[10] = d2[20], idx[20]  # a tie
    d2[30] = np.nan
    want = U.unique_mask(idx, d2, 40)
    np.testing.assert_array_equal(KR._unique(idx, d2.astype(np.longdouble), 40, np.longdouble), want)
    assert want[10] == want[20] and not want[30]


# ---- b. the matrix ------------------------------------------------------------------------------

def check_cell(oracle, n, cell, table):
    metric, gate, trim, kname, uniq = cell
    a = KR.reference(oracle, n, cell)
    b = KR.reference(oracle, n, cell, np.longdouble)
    m = KR.matrix_case(n)[0]
    extent = float(np.abs(m).max())
    L = np.longdouble
    margins = {k: min(a[k + "_margin"], b[k + "_margin"]) for k in ("gate", "trim", "unique", "k")}
    print(KR.cell_id(cell), "K", a["K"], "K+", a["Kpos"], "over", a["Kover"], {k: "%.1e" % v for k, v in margins.items()})
    assert a["status"] == b["status"] == "ok" and a["iterations"] == b["iterations"] == KR.MATRIX_ITERS
    assert a["K"] == table[cell]
    # the margins that apply
    for name, on in (("gate", gate), ("trim", trim), ("unique", uniq), ("k", kname in ("huber", "tukey"))):
        assert (margins[name] > FLOOR) if on else (margins[name] == np.inf), (name, margins[name])
    # the weights bite
    if kname == "tukey":
        assert any(kp < k for kp, k in zip(a["Kpos"], a["K"]))
    if kname == "huber":
        assert any(o > 0 for o in a["Kover"]) and any(o < kp for o, kp in zip(a["Kover"], a["Kpos"]))
    # both cuts bind (the module's docstring: the C list in every cell, the K list without one-to-one)
    if gate and trim:
        D = np.float64(KR.DMAX) * np.float64(KR.DMAX)
        assert any(c > D for c in a["C"]) and any(c <= D for c in a["C"]), a["C"]
        if not uniq:
            assert any(k < a["T"] for k in a["K"]) and any(k == a["T"] for k in a["K"]), (a["K"], a["T"])
    # fp64 against longdouble
    assert a["K"] == b["K"] and a["Kpos"] == b["Kpos"]
    np.testing.assert_array_equal(a["mask"], b["mask"])
    eb = b["err"]
    de = np.abs(a["err"].astype(L) - eb)
    ok = de <= GAP * np.abs(eb)
    if metric in ("symm", "gicp"):  # (test_symm_ref.err_close's floor, for an err fallen to rounding)
        ok |= de <= (1e-9 * extent) ** 2
    gaps = dict(err=float(np.max(de / np.abs(eb))), R=float(np.max(np.abs(np.asarray(a["R"], dtype=L) - b["R"]))),
                s=float(abs(L(a["s"]) - b["s"])), t=float(np.max(np.abs(np.asarray(a["t"], dtype=L) - b["t"]))) / extent,
                new_p=float(np.max(np.abs(a["new_p"].astype(L) - b["new_p"]))) / extent)
    if a["W"]:
        wb = np.array(b["W"], dtype=L)
        gaps["W"] = float(np.max(np.abs(np.array(a["W"], dtype=L) - wb) / wb))
    print("   gaps", {k: "%.1e" % v for k, v in gaps.items()})
    assert np.all(ok), (a["err"], eb)
    for name in ("R", "s", "t", "new_p", "W"):
        assert gaps.get(name, 0.0) < GAP, (name, gaps[name])


@pytest.mark.parametrize("cell", KR.cells(), ids=KR.cell_id)
def test_matrix_cell(oracle, cell):
    check_cell(oracle, KR.MATRIX_N, cell, KR.MATRIX_K)


@pytest.mark.parametrize("cell", KR.row_cells(), ids=KR.cell_id)
def test_everything_on_row_at_4097(oracle, cell):
    check_cell(oracle, KR.ROW_N, cell, KR.ROW_K)


def test_the_tables_cover_the_matrix():
    assert len(KR.cells()) == 128 == len(set(KR.cells())) and set(KR.MATRIX_K) == set(KR.cells())
    assert len(KR.row_cells()) == 16 and set(KR.ROW_K) == set(KR.row_cells()) <= set(KR.cells())
    assert [len(KR.cells(mt)) for mt in KR.METRICS] == [32] * 4
    assert TR.trim_count(KR.TRIM[257], 257) == 106 and TR.trim_count(KR.TRIM[4097], 4097) == 2568
