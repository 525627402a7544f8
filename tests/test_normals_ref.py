"""CPU checks that pin the reference of the estimated normals (tests/normals_ref.py) and the inputs
of tests/test_gpu_normals.py before the GPU tests rely on them: the library exports the calls, the
reference's normals are the surface's to the angle a 16-point neighbourhood allows, the fp64
restatement agrees with its extended-precision twin far inside the GPU tolerance, and the inputs
have the conditioning the GPU comparisons assume (clear eigenvalue gaps, clear signs, real ties)."""
import numpy as np
import pytest

import normals_ref as NR
import plane_ref as P


def _load(oracle):
    return oracle.load_matrix


# (a)
def test_library_exports_the_calls(icp_lib):
    names = ("icp_model_knn", "icp_estimate_model_normals", "icp_get_model_normals")
    for name in names:
        assert name in icp_lib.EXPORTED
        assert hasattr(icp_lib.lib(), name), name
    for name in ("model_knn", "estimate_model_normals", "model_normals"):
        assert callable(getattr(icp_lib.Context, name))
    with pytest.raises(ValueError):
        icp_lib.ICP(np.zeros((8, 3)), np.zeros((8, 3)), 1, normals=np.zeros((8, 3)), estimate_normals=4)


# (b) measured at k = 16, n = 4097: largest 7.0 degrees, mean 1.1; the bound is the measured largest
# value plus a quarter for other seeds
def test_estimated_normals_are_the_surfaces():
    m, k, r = NR.reference("ell4097")
    exact = P.ellipsoid(4097, 4197)[1]
    cosang = np.clip(np.abs((r["normals"] * exact).sum(axis=1)), 0, 1)
    ang = np.degrees(np.arccos(cosang))
    print("angle to the exact normal, degrees: largest", ang.max(), "mean", ang.mean())
    assert r["degenerate"] == 0
    assert ang.max() <= 7.0 * 1.25
    assert ang.mean() <= 1.1 * 1.25


# (c) the inputs' conditioning takes under 1 % of the GPU tests' tolerance: a direction within 1e-9
# means |n . n_ref| >= 1 - 1e-9, i.e. an angle of 4.5e-5; here the components agree to 1e-11
@pytest.mark.parametrize("name", ["ell257", "ell4097", "cow", "lattice", "planar", "ell257k64", "ell257k3"])
@pytest.mark.parametrize("view", [None, NR.VIEW])
def test_fp64_reference_against_extended_precision(oracle, name, view):
    _m, _k, a = NR.reference(name, _load(oracle), view)
    _m, _k, b = NR.reference(name, _load(oracle), view, np.longdouble)
    clear = (a["gap"] >= NR.GAP_CLEAR) & (a["sign_margin"] >= NR.SIGN_CLEAR)
    diff = float(np.abs(a["normals"][clear] - np.asarray(b["normals"], dtype=np.float64)[clear]).max())
    dgap = float(np.abs(a["gap"] - b["gap"]).max())
    print(name, view, "points compared", int(clear.sum()), "largest component difference", diff, "gap", dgap)
    assert clear.sum() >= 0.9 * clear.size  # (the lattice's 60 edge points have two equal components: 8 %)
    assert diff <= 1e-11
    assert dgap <= 1e-11
    np.testing.assert_array_equal(a["zero"], b["zero"])


# (d) what the GPU comparisons assume of their inputs: the points their filters leave out are few.
# The gap's cap holds for every input of the direction comparison; the sign's for those inputs'
# points taken together (the lattice's 60 edge points have normals with two components of exactly
# equal magnitude, 8 % of that one small cloud and 0.3 % of all the points compared)
def test_inputs_have_clear_gaps_and_signs(oracle):
    for view in (None, NR.VIEW):
        points = unclear_all = 0
        for name in NR.CLEAR_CASES:
            _m, _k, r = NR.reference(name, _load(oracle), view)
            band = (r["gap"] > NR.GAP_MIN) & (r["gap"] < NR.GAP_CLEAR)
            unclear = ~r["zero"] & (r["sign_margin"] < NR.SIGN_CLEAR)
            print(name, view, "least gap ratio", r["gap"].min(), "in the uncertain band", int(band.sum()),
                  "unclear signs", int(unclear.sum()), "degenerate", r["degenerate"])
            assert band.mean() <= 0.01
            assert r["degenerate"] == 0
            if name == "far":  # exactly its 8 far points sit in the band
                assert band.sum() == 8 and band[-8:].all()
            else:
                assert band.sum() == 0
            points += unclear.size
            unclear_all += int(unclear.sum())
        print(view, "unclear signs", unclear_all, "of", points)
        assert unclear_all <= 0.01 * points


def test_lattice_and_line_have_ties_and_the_line_no_direction():
    _m, _k, lat = NR.reference("lattice")
    _m, _k, lin = NR.reference("line")
    print("lattice ties", int(lat["tie"].sum()), "line ties", int(lin["tie"].sum()), "line gap", lin["gap"].max())
    assert lat["tie"].sum() == 669
    assert lin["tie"].sum() == 52
    assert lin["degenerate"] == 64 and not lin["normals"].any()
    assert lin["gap"].max() < NR.GAP_MIN
    _m, _k, eq = NR.reference("equal")
    assert eq["degenerate"] == 32 and not eq["normals"].any()
    np.testing.assert_array_equal(eq["idx"], np.tile(np.arange(16, dtype=np.int32), (32, 1)))
    _m, _k, dup = NR.reference("duplicates")
    assert (dup["idx"][:, 0] != np.arange(dup["idx"].shape[0])).sum() == 40  # (the later copy is not first in its own row)
    _m, _k, pl = NR.reference("planar")
    np.testing.assert_allclose(np.abs(pl["normals"]), np.tile([0.0, 0.0, 1.0], (400, 1)), atol=1e-12)


# (e) the purpose: point-to-plane on estimated normals lands where it does on exact ones
def test_plane_ref_on_estimated_normals(oracle):
    m, _nrm, p, src = P.synth(4097, 4197, 0.0, other=True)
    _m, _k, r = NR.reference("ell4097")
    np.testing.assert_array_equal(_m, m)
    out = P.plane_ref(oracle, m, r["normals"], p, 0.0, 5, -1.0)
    d = float(np.abs(out["new_p"] - src).max())
    print("max |new_p - src| after 5 plane iterations on estimated normals", d)
    assert out["status"] == "ok" and out["iterations"] == 5
    assert d <= 1.5e-4 * 1.25
