"""CPU checks of the symmetric point-to-plane reference (tests/symm_ref.py) that pin the inputs of
tests/test_gpu_symm.py before the GPU tests rely on them: the fp64 restatement agrees with its
extended-precision twin far inside the GPU tolerances, no pair of the gate cases lies within 1e-6 of
the gate (or of the trim's cut), the pivots are far from the degenerate limit, the degenerate and
too-few inputs are what they claim, the symmetric form lands where point-to-plane's one-sided planes
leave a bias -- and the ABI's argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import plane_ref as P
import symm_ref as S


def err_close(a, b, extent):
    """err within 1e-11 relative, or within the floor of (1e-9 x extent)^2 absolutely: the project's
    position tolerance, squared.  The floor bounds the difference, as the atol of an allclose does: where
    an exactly determined system (n = 6) lets err fall to rounding (6.6e-8, 1.5e-14, 6.6e-21, ... 4e-33),
    the two precisions differ by what one ulp of a coordinate does to residuals of 1e-7 and less --
    2.0e-23 at err = 1.5e-14, 1.3e-9 of it, and 6,400 times the last err -- which no relative bound on an
    fp64 restatement can hold and the floor, 9.2e-19 here, does."""
    floor = (1e-9 * extent) ** 2
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return bool(np.all((np.abs(a - b) <= 1e-11 * np.abs(b)) | (np.abs(a - b) <= floor)))


@pytest.mark.parametrize("n", S.SIZES)
def test_fp64_reference_against_extended_precision(oracle, n):
    m, _N, _p, _U, _d, a = S.reference(oracle, ("size", n))
    _m, _N, _p, _U, _d, b = S.reference(oracle, ("size", n), np.longdouble)
    dp = float(np.max(np.abs(a["new_p"] - b["new_p"])))
    print(n, "err", a["err"], "twin", b["err"], "new_p abs", dp, "smallest pivot", a["min_pivot"])
    assert a["status"] == b["status"] == "ok"
    assert a["iterations"] == b["iterations"] == S.SIZES_ITERS
    assert a["K"] == b["K"] == [n] * S.SIZES_ITERS and a["mask"].all()
    assert err_close(a["err"], b["err"], float(np.abs(m).max())) and dp <= 1e-11
    assert a["min_pivot"] > 1e-3  # (0.037 at n = 6, 0.22 at n = 7, >= 0.67 from n = 63)


@pytest.mark.parametrize("n,dmax", list(S.GATES))
def test_gate_cases(oracle, n, dmax):
    m, _N, _p, _U, _d, a = S.reference(oracle, ("gate", n, dmax))
    _m, _N, _p, _U, _d, b = S.reference(oracle, ("gate", n, dmax), np.longdouble)
    print(n, dmax, a["K"], a["margin"], b["margin"], a["min_pivot"])
    assert a["K"] == b["K"] == S.GATES[(n, dmax)] and len(a["K"]) == S.GATES_ITERS
    np.testing.assert_array_equal(a["mask"], b["mask"])
    assert a["margin"] > 1e-6 and b["margin"] > 1e-6
    assert a["min_pivot"] > 1e-3
    assert err_close(a["err"], b["err"], float(np.abs(m).max()))


@pytest.mark.parametrize("kind", ["trim", "tukey"])
def test_gate_case_with_a_trim_and_with_weights(oracle, kind):
    m, _N, _p, _U, _d, a = S.reference(oracle, (kind, 4097, 0.08))
    _m, _N, _p, _U, _d, b = S.reference(oracle, (kind, 4097, 0.08), np.longdouble)
    print(kind, a["K"], a["Kpos"], a["margin"], b["margin"], a["min_pivot"])
    assert a["status"] == b["status"] == "ok" and a["K"] == b["K"] and len(a["K"]) == S.GATES_ITERS
    assert a["Kpos"] == b["Kpos"]
    np.testing.assert_array_equal(a["mask"], b["mask"])
    assert a["margin"] > 1e-6 and b["margin"] > 1e-6 and a["min_pivot"] > 1e-3
    assert err_close(a["err"], b["err"], float(np.abs(m).max()))
    assert float(np.max(np.abs(a["new_p"] - b["new_p"]))) <= 1e-11


def test_planar_model_is_degenerate(oracle):
    m, nrm, p, U0 = S.planar()
    for dtype in (np.float64, np.longdouble):
        r = S.symm_ref(oracle, m, nrm, p, U0, 0.0, 3, -1.0, dtype)
        assert r["status"] == "degenerate" and r["fail_iter"] == 0 and r["iterations"] == 0
        assert not r["min_pivot"] > P.PIVOT_MIN
        np.testing.assert_array_equal(np.asarray(r["new_p"], dtype=np.float64), p)


def test_five_points_are_too_few(oracle):
    m, nrm, p, U0 = S.five()
    for dtype in (np.float64, np.longdouble):
        r = S.symm_ref(oracle, m, nrm, p, U0, 0.0, 3, -1.0, dtype)
        assert r["status"] == "few" and r["fail_iter"] == 0 and r["K_fail"] == 5 and r["K"] == []
        np.testing.assert_array_equal(np.asarray(r["new_p"], dtype=np.float64), p)


def test_signs_and_zero_normals(oracle):
    """The sign of any normal of either cloud changes no bit; a zero normal drops its pair's terms."""
    m, nrm, p, U0, _d, a = S.reference(oracle, ("size", 257))
    flip = np.where(np.random.default_rng(1).random(257) < 0.5, -1.0, 1.0)[:, None]
    for N2, U2 in ((nrm * flip, U0), (nrm, U0 * flip)):
        b = S.symm_ref(oracle, m, N2, p, U2, 0.0, S.SIZES_ITERS, -1.0)
        np.testing.assert_array_equal(b["err"], a["err"])
        np.testing.assert_array_equal(b["new_p"], a["new_p"])
    N0, U00 = nrm.copy(), U0.copy()
    N0[7] = 0.0
    U00[11] = 0.0
    z = S.symm_ref(oracle, m, N0, p, U00, 0.0, S.SIZES_ITERS, -1.0)
    assert z["status"] == "ok" and z["K"] == [257] * S.SIZES_ITERS and not np.array_equal(z["err"], a["err"])


def test_purpose_inputs(oracle):
    """A different sample of the same curved surface from 15 degrees: the symmetric form lands on the
    pose, point-to-plane stops at the bias of its one-sided planes (tests/test_gpu_symm.py asserts
    the same of the engine)."""
    m, nrm, p, U0, src = S.purpose()
    s = S.symm_ref(oracle, m, nrm, p, U0, 0.0, 5, -1.0)
    o = P.plane_ref(oracle, m, nrm, p, 0.0, 8, -1.0)
    dsymm, dplane = float(np.abs(s["new_p"] - src).max()), float(np.abs(o["new_p"] - src).max())
    print("symmetric, 5 iterations", dsymm, "point-to-plane, 8 iterations", dplane)
    assert dsymm < 2e-5 and dplane > 1e-4


def test_abi_without_a_device(icp_lib):
    amd = icp_lib
    L = amd.lib()
    n = np.zeros((4, 3))
    dp = n.ctypes.data_as(C.POINTER(C.c_double))
    assert L.icp_set_plane_symmetric(None, 1) == amd.ICP_E_ARG
    assert L.icp_set_scene_normals(None, dp, 4) == amd.ICP_E_ARG
    assert L.icp_set_scene_normals_device(None, None, 4) == amd.ICP_E_ARG
    assert L.icp_get_scene_normals(None, dp) == amd.ICP_E_ARG
    assert L.icp_estimate_scene_normals(None, 16, None, None) == amd.ICP_E_ARG
