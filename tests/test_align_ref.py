"""tests/align_ref.py, the extended-precision truth of an iteration's arithmetic, checked on the
CPU: exact where the answer is known exactly, against the fp64 oracle where that is well
conditioned, and the conditions the GPU tests (tests/test_gpu_align_accuracy.py) rely on, from the
oracle's own trajectory at small n."""
import numpy as np
import pytest

import align_ref as A
import datasets
import gated_ref as G

LD = A.LD
N_SMALL, N_GATED = 1000, 257
CHECKED = (1, 2, 6)  # the iterations the GPU tests check


def lattice_problem(seed=3, n=300):
    """p on 25 Z^3, y = s R p + t with R = the rotation of the integer quaternion (1, 2, 2, 4) / 5
    (entries k / 25), s a power of two, t dyadic: every y is exact in fp64."""
    rng = np.random.default_rng(seed)
    pi = rng.integers(-9, 10, size=(n, 3))
    pi -= np.round(pi.mean(axis=0)).astype(pi.dtype)
    Rnum = np.array([[-15, 0, 20], [16, -15, 12], [12, 20, 9]])
    assert np.array_equal(Rnum @ Rnum.T, 625 * np.eye(3, dtype=int))
    s, t = 4.0, np.array([1.5, -0.25, 3.0])
    p = 25.0 * pi
    y = s * (pi @ Rnum.T).astype(np.float64) + t
    return p, y, s, LD(1) * Rnum / LD(25), t


def test_truth_is_exact_on_a_lattice():
    p, y, s, R, t = lattice_problem()
    tr = A.truth_alignment(p, y)
    print("ds", float(abs(tr["s"] - s)), "dR", float(np.abs(tr["R"] - R).max()), "dt", float(np.abs(tr["t"] - t).max()),
          "e", float(tr["e"]), "gap", float(tr["gap"]))
    assert abs(tr["s"] - LD(s)) <= LD(1e-18) * s
    assert np.abs(tr["R"] - R).max() <= LD(1e-18)
    assert np.abs(tr["t"] - A._ld(t)).max() <= LD(1e-18) * np.abs(y).max()
    assert tr["e"] <= LD(1e-30) * (A._ld(y) ** 2).sum()
    assert abs(np.linalg.det(np.asarray(tr["R"], dtype=np.float64)) - 1.0) < 1e-15
    it = A.truth_iteration(p, y)
    assert it["K"] == p.shape[0] and it["err"] == 2 * it["e"] / p.shape[0]
    np.testing.assert_array_equal(np.asarray(it["x"], dtype=np.float64), y)  # (x* rounds to y exactly)


def test_truth_negative_control():
    """One point of the exact problem moved by 1e-9 of the extent changes s, R and e by far more
    than the tolerance of the exact test."""
    p, y, s, R, _t = lattice_problem()
    y2 = y.copy()
    y2[17, 0] += 1e-9 * np.abs(y).max()
    tr = A.truth_alignment(p, y2)
    assert abs(tr["s"] - LD(s)) > LD(1e-15) * s
    assert np.abs(tr["R"] - R).max() > LD(1e-15)
    assert tr["e"] > LD(1e-22) * (A._ld(y) ** 2).sum()
    dev = A.deviation(dict(s=s, R=np.asarray(R, dtype=np.float64), t=_t), A.truth_iteration(p, y2))
    assert dev["ds"] > 1e-15 and dev["dR"] > 1e-15


def test_keep_restricts_the_alignment_and_moves_every_point():
    p, y, s, R, t = lattice_problem()
    y2 = y.copy()
    y2[:40] += 1000.0  # outliers
    keep = np.ones(p.shape[0], dtype=bool)
    keep[:40] = False
    it = A.truth_iteration(p, y2, keep)
    assert it["K"] == p.shape[0] - 40
    assert abs(it["s"] - LD(s)) <= LD(1e-18) * s and np.abs(it["R"] - R).max() <= LD(1e-18)
    np.testing.assert_array_equal(np.asarray(it["x"], dtype=np.float64), y)  # (the outliers moved too)
    assert it["err"] <= LD(1e-30) * (A._ld(y) ** 2).sum()


def test_horn_matrix_map_is_a_bijection():
    rng = np.random.default_rng(0)
    S = rng.standard_normal((5, 3, 3))
    N = A.horn_matrix(S)
    np.testing.assert_allclose(N, np.swapaxes(N, -1, -2), atol=0)
    np.testing.assert_allclose(np.trace(N, axis1=-1, axis2=-2), 0.0, atol=1e-15)
    np.testing.assert_allclose(A.horn_matrix_inverse(N), S, atol=1e-15)


def well_conditioned(oracle):
    out = []
    for name in ("plain", "scaled_small", "noisy"):
        c = A.case(name, N_SMALL)
        out.append((name, c["m"], c["p"]))
    m, tr1, tr2 = G.load_cow(oracle)
    out += [("cow_tr1", m, tr1), ("cow_tr2", m, tr2)]
    out.append(("bunny", oracle.load_matrix(datasets.path("bun000")), oracle.load_matrix(datasets.path("bun045"))))
    return out


def test_truth_agrees_with_the_oracle_where_that_is_well_conditioned(oracle):
    for name, m, p in well_conditioned(oracle):
        Y, _ = oracle.closest(p, m)
        tr = A.truth_iteration(p, Y)
        al = oracle.find_alignment(p, Y)
        e, new_p = oracle.err_compute(p, Y, al.s, al.R, al.t)
        err = (al.err + e) / p.shape[0]
        ext = float(np.abs(p).max())
        print(name, "gap", float(tr["gap"]), "ds", abs(al.s - float(tr["s"])), "derr", abs(err / float(tr["err"]) - 1))
        assert tr["gap"] > 0.1
        assert abs(al.s - tr["s"]) <= 1e-13 * tr["s"]
        assert np.abs(A._ld(np.array(al.R).reshape(3, 3)) - tr["R"]).max() <= 1e-13
        assert np.abs(A._ld(np.array(al.t)) - tr["t"]).max() <= 1e-13 * ext
        assert np.abs(A._ld(new_p) - tr["x"]).max() <= 1e-13 * ext
        assert abs(LD(err) - tr["err"]) <= 1e-13 * tr["err"]


@pytest.fixture(scope="module")
def trajectories(oracle):
    """(name, gated) -> list over the checked iterations of (truth, m, margin): the oracle's own
    trajectory at small n, the pairs of iteration k taken on the scene of k - 1."""
    out = {}
    for gated in (False, True):
        n = N_GATED if gated else N_SMALL
        for name in A.CASES:
            c = A.case(name, n, gated=gated)
            m, p = c["m"], c["p"].copy()
            D = None if not gated else np.float64(c["dmax"]) * np.float64(c["dmax"])
            rows = []
            for k in range(1, max(CHECKED) + 1):
                Y, _ = oracle.closest(p, m)
                keep, margin = None, np.inf
                if gated:
                    d2 = G.d2_of(p, Y)
                    keep = d2 <= D
                    margin = float(np.min(np.abs(d2 - D) / D))
                tr = A.truth_iteration(p, Y, keep)
                if k in CHECKED:
                    rows.append((tr, m, margin, c))
                kk = tr["keep"]
                al = oracle.find_alignment(p[kk], Y[kk])
                _, p = oracle.err_compute(p, Y, al.s, al.R, al.t)
            out[(name, gated)] = rows
    return out


def test_yardstick_oracle_deviation_from_truth(oracle, trajectories):
    """The oracle's own distance from the truth on every named input: what the GPU tests measure
    the engine against.  Recorded (pytest -s), and bounded where conditioning allows a bound."""
    for (name, gated), rows in trajectories.items():
        for k, (tr, _m, _margin, c) in zip(CHECKED, rows):
            dev = A.oracle_deviation(oracle, tr)
            print(f"{name:13s} gated={int(gated)} k={k} gap {float(tr['gap']):.3g} dpoly {float(tr['dpoly']):.3g} "
                  + " ".join(f"{m} {dev[m]:.2g}" for m in A.METRICS))
            assert all(np.isfinite(v) for v in dev.values())
            w = float(tr["gap"]) if c["rod"] else 1.0
            assert dev["ds"] <= 1e-13 and dev["dR"] * w <= 1e-13 and dev["dOpt"] <= 1e-12
            # the engine measured against itself must pass (the acceptance is reflexive)
            assert A.acceptance(dev, dev, rod=bool(c["rod"]), gap=tr["gap"], lever=tr["lever"])[0] == []


def test_conditions_on_the_inputs(trajectories):
    for (name, gated), rows in trajectories.items():
        for k, (tr, m, margin, c) in zip(CHECKED, rows):
            y_kept = np.asarray(tr["y"], dtype=np.float64)[tr["keep"]]
            if gated:  # no pair within 1e-6 of the gate; the clump dropped, A kept
                assert margin >= 1e-6, (name, k, margin)
                n = tr["p"].shape[0]
                assert tr["K"] == n - max(1, n // 20), (name, k, tr["K"])
            if c["rod"] is None:
                assert tr["gap"] >= 0.1, (name, k, float(tr["gap"]))
            if name in A.PATCH_RATIOS:
                r = A.d_over_sigma(A.model_centre(m), y_kept)
                assert 0.5 * A.PATCH_RATIOS[name] <= r <= 2.0 * A.PATCH_RATIOS[name], (name, k, r)
            if name == "far":
                r = A.d_over_sigma(np.zeros(3), y_kept)
                assert 0.5 * A.FAR_NOMINAL <= r <= 2.0 * A.FAR_NOMINAL, (name, k, r)
            assert tr["err"] > 1e-7 * c["width"] ** 2 * (c["rod"] or 1.0) ** 2, (name, k)  # (e* far above rounding)


def test_acceptance_rejects_a_defect():
    """A deviation that grows like (D / sigma)^2 eps is refused from D / sigma ~ 10 on."""
    yard = {k: 2e-16 for k in A.METRICS}
    yard["dP"] = 2.0
    ok = dict(yard, ds=20 * A.EPS64)
    assert A.acceptance(ok, yard)[0] == []
    bad = dict(yard, ds=100.0 * A.EPS64 * 8)
    fails, ratios = A.acceptance(bad, yard)
    assert len(fails) == 1 and fails[0].startswith("ds") and ratios["ds"] > 1
    rod = dict(yard, dR=1e-10)  # a rod with gap 1e-6: dR gap = 1e-16, inside the floor
    assert A.acceptance(rod, yard, rod=True, gap=1e-6, lever=1e-3)[0] == [] and A.acceptance(rod, yard)[0] != []
    # ... whose points lie within 1e-3 of the axis: dX up to rounding / gap x lever passes, a
    # displaced centroid (an error of t) of the same size does not
    assert A.acceptance(dict(yard, dX=1e-13), yard, rod=True, gap=1e-6, lever=1e-3)[0] == []
    assert A.acceptance(dict(yard, dX=1e-10), yard, rod=True, gap=1e-6, lever=1e-3)[0] != []
    assert A.acceptance(dict(yard, dC=1e-13), yard, rod=True, gap=1e-6, lever=1e-3)[0] != []
    assert 1e-6 < A.HANDOVER < 1e-1  # (read from icp_horn.h)
