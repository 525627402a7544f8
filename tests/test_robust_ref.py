"""tests/robust_ref.py checked on the CPU, before tests/test_gpu_robust.py relies on it.

Measured (fp64 reference against the longdouble one, every named case; the GPU comparison allows 1e-9,
and the reference has to sit within 1 % of that, plane_ref's own rule):
  sizes (2 metrics x 3 kinds x 7 sizes, 6 iterations): err rel at most 3.7e-12 (point-to-plane, Tukey,
    n = 6; 2.9e-12 for Cauchy at n = 6; every case above n = 7 under 1e-14), R 3.6e-14, new_p 2.4e-13 of
    the extent, W rel 2.0e-12; K, K+ and the status equal in every iteration
  far (10 x the extent, n = 4097): err rel 2.0e-15, new_p 2.0e-15
  outlier shell, Tukey: err rel 4.9e-15 / 2.0e-15 (point-to-point / point-to-plane), new_p 1.2e-15
kmargin (min |r2 - k2| / k2): sizes at least 1.6e-5 (point-to-point, Huber, n = 4097), the shell's Tukey
runs 5.9e-5 and 7.1e-4, against the 1e-9 the GPU tests need.
The outlier shell at n = 2048, dmax = 0.25 (K = 2048 in every iteration: the gate removes nothing),
largest distance of an inlier from its model point:
  point-to-point, 20 iterations: unweighted 2.798e-2, Tukey k = 0.06 9.81e-3 (2.85 x closer)
  point-to-plane, 12 iterations: unweighted 2.860e-2, Tukey k = 0.06 1.137e-2 (2.52 x closer)
  (Cauchy k = 0.03: 1.05e-2 / 1.18e-2; Huber k = 0.02: 1.18e-2 / 1.27e-2; 4 sigma of the noise is 8e-3)
"""
import numpy as np
import pytest

import gated_ref as G
import plane_ref as P
import robust_ref as R

GAP = 1e-11  # 1 % of the GPU comparison's 1e-9


def check_gap(m, a, b):
    """a: the fp64 reference, b: the longdouble one."""
    assert a["status"] == b["status"] == "ok" and a["iterations"] == b["iterations"]
    assert a["K"] == b["K"] and a["Kpos"] == b["Kpos"]
    extent = float(np.abs(m).max())
    eb = b["err"]
    gaps = dict(err=float(np.max(np.abs(a["err"].astype(np.longdouble) - eb) / np.abs(eb))),
                R=float(np.max(np.abs(a["R"].astype(np.longdouble) - b["R"]))),
                t=float(np.max(np.abs(np.asarray(a["t"], dtype=np.longdouble) - b["t"]))) / extent,
                new_p=float(np.max(np.abs(a["new_p"].astype(np.longdouble) - b["new_p"]))) / extent,
                W=float(np.max(np.abs(np.array(a["W"], dtype=np.longdouble) - np.array(b["W"], dtype=np.longdouble))
                               / np.array(b["W"], dtype=np.longdouble))))
    print({k: "%.1e" % v for k, v in gaps.items()}, "kmargin %.2e" % a["kmargin"], "K+", a["Kpos"])
    for name, g in gaps.items():
        assert g < GAP, (name, g)


def test_none_equals_the_unweighted_references(oracle):
    m, nrm, p, _src = P.synth(257, 357, 0.01)
    for dmax in (0.0, 0.08):
        a = R.robust_ref(oracle, "plane", m, nrm, p, dmax, R.NONE, 0.0, 6, -1.0)
        b = P.plane_ref(oracle, m, nrm, p, dmax, 6, -1.0)
        for key in ("err", "new_p", "R", "t", "mask"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        assert a["K"] == b["K"] == a["Kpos"] and a["W"] == [float(x) for x in b["K"]] and a["kmargin"] == np.inf
    mg, pg = G.synth(257, 357, 0.25)
    a = R.robust_ref(oracle, "point", mg, None, pg, 1.0, R.NONE, 0.0, 6, -1.0)
    b = G.gated_ref(oracle, mg, pg, 1.0, 6, -1.0)
    for key in ("err", "new_p", "R", "t", "mask"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["K"] == b["K"] == a["Kpos"]


def test_unit_weights_restate_the_oracles_horn(oracle):
    """The weighted point-to-point code with every weight 1 (Huber, k = 1e150) against gated_ref, the
    oracle's own find_alignment: two summation orders of the same arithmetic."""
    m, _nrm, p, _src = P.synth(257, 357, 0.01)
    a = R.robust_ref(oracle, "point", m, None, p, 0.5, R.HUBER, 1e150, 6, -1.0)
    b = G.gated_ref(oracle, m, p, 0.5, 6, -1.0)
    assert a["K"] == b["K"] == a["Kpos"] and a["W"] == [float(x) for x in b["K"]]
    np.testing.assert_allclose(a["err"], b["err"], rtol=1e-13)
    np.testing.assert_allclose(a["new_p"], b["new_p"], atol=1e-14)


def test_weights():
    k = 0.5
    r2 = np.array([0.0, 0.1, 0.25, 0.26, 1.0, np.inf, np.nan])
    np.testing.assert_array_equal(R.weights(R.HUBER, r2, k), [1, 1, 1, k / np.sqrt(0.26), 0.5, 0, 0])
    np.testing.assert_array_equal(R.weights(R.TUKEY, r2, k), [1, (1 - 0.1 / 0.25) ** 2, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(R.weights(R.CAUCHY, r2, k), [1, 1 / (1 + 0.1 / 0.25), 0.5, 1 / (1 + 0.26 / 0.25), 0.2, 0, 0])
    np.testing.assert_array_equal(R.weights(R.NONE, r2, k), np.ones(7))


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("kname", list(R.KINDS))
@pytest.mark.parametrize("metric", R.METRICS)
def test_sizes_fp64_against_longdouble(oracle, metric, kname, n):
    kind = R.KINDS[kname]
    m, _nrm, _p, _dmax, _kind, _k, a = R.reference(oracle, ("size", metric, kind, n))
    b = R.reference(oracle, ("size", metric, kind, n), np.longdouble)[-1]
    check_gap(m, a, b)
    least = 6 if metric == "plane" else 4
    assert a["iterations"] == R.SIZES_ITERS and min(a["Kpos"]) >= least
    if kind != R.CAUCHY:
        assert a["kmargin"] >= 1e-9
    if kind == R.TUKEY and n >= 63:  # (the cases are worth their name: some pairs weigh nothing)
        assert a["Kpos"][0] < n
    if kind == R.HUBER:
        assert a["W"][0] < 0.9 * n


def test_far_fp64_against_longdouble(oracle):
    m, _nrm, _p, _dmax, _kind, _k, a = R.reference(oracle, ("far",))
    b = R.reference(oracle, ("far",), np.longdouble)[-1]
    check_gap(m, a, b)
    assert a["K"] == [R.FAR_N] * R.SIZES_ITERS and a["Kpos"][0] == R.FAR_N and a["W"][0] < 0.5 * R.FAR_N
    assert a["kmargin"] >= 1e-9 and a["margin"] > 1e-6


@pytest.mark.parametrize("metric", R.METRICS)
def test_outlier_shell_halves_the_inliers_displacement(oracle, metric):
    m, _nrm, _p, inlier = R.outlier_shell()
    _m, _n, _p, _d, _kind, _k, plain = R.reference(oracle, ("shell", metric, R.NONE))
    _m, _n, _p, _d, _kind, _k, tukey = R.reference(oracle, ("shell", metric, R.TUKEY))
    check_gap(m, tukey, R.reference(oracle, ("shell", metric, R.TUKEY), np.longdouble)[-1])
    d0, d1 = R.inlier_displacement(plain["new_p"], m, inlier), R.inlier_displacement(tukey["new_p"], m, inlier)
    print(metric, "unweighted %.3e Tukey %.3e ratio %.2f" % (d0, d1, d0 / d1), "K", tukey["K"][0], "K+", tukey["Kpos"][-1])
    assert plain["K"] == tukey["K"] == [R.SHELL_N] * R.SHELL_ITERS[metric]  # the gate removes none of the outliers
    assert d1 <= 0.5 * d0
    assert tukey["kmargin"] >= 1e-9 and tukey["margin"] > 1e-6
