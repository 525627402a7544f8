"""CPU checks of the point-to-plane reference (tests/plane_ref.py) that pin the inputs of
tests/test_gpu_plane.py before the GPU tests rely on them: the fp64 restatement agrees with its
extended-precision twin far inside the GPU tolerances (so the inputs' conditioning takes under 1 %
of the project's 1e-9), no pair of the gate cases lies within 1e-6 of the gate (so a trajectory
that differs in the last bits cannot flip a gate decision), the degenerate and too-few inputs are
what they claim -- and the ABI's argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import plane_ref as P


@pytest.mark.parametrize("n", P.SIZES)
def test_fp64_reference_against_extended_precision(oracle, n):
    _m, _N, _p, _d, a = P.reference(oracle, ("size", n))
    _m, _N, _p, _d, b = P.reference(oracle, ("size", n), np.longdouble)
    rel = float(np.max(np.abs(a["err"] - b["err"]) / np.abs(b["err"])))
    dp = float(np.max(np.abs(a["new_p"] - b["new_p"])))
    print(n, "err rel", rel, "new_p abs", dp, "smallest pivot", a["min_pivot"])
    assert a["status"] == b["status"] == "ok"
    assert a["iterations"] == b["iterations"] == P.SIZES_ITERS
    assert a["K"] == b["K"] == [n] * P.SIZES_ITERS and a["mask"].all()
    assert rel <= 1e-11 and dp <= 1e-11
    assert a["min_pivot"] > 1e-3  # (0.004 at n = 6, >= 0.25 from n = 7)


@pytest.mark.parametrize("n,dmax", list(P.GATES))
def test_gate_cases(oracle, n, dmax):
    _m, _N, _p, _d, a = P.reference(oracle, ("gate", n, dmax))
    _m, _N, _p, _d, b = P.reference(oracle, ("gate", n, dmax), np.longdouble)
    print(n, dmax, a["K"], a["margin"], b["margin"])
    assert a["K"] == b["K"] == P.GATES[(n, dmax)] and len(a["K"]) == P.GATES_ITERS
    np.testing.assert_array_equal(a["mask"], b["mask"])
    assert a["margin"] > 1e-6 and b["margin"] > 1e-6
    np.testing.assert_allclose(a["err"], np.asarray(b["err"], dtype=np.float64), rtol=1e-11)


def test_planar_model_is_degenerate(oracle):
    m, nrm, p = P.planar()
    for dtype in (np.float64, np.longdouble):
        r = P.plane_ref(oracle, m, nrm, p, 0.0, 3, -1.0, dtype)
        assert r["status"] == "degenerate" and r["fail_iter"] == 0 and r["iterations"] == 0
        assert not r["min_pivot"] > P.PIVOT_MIN
        np.testing.assert_array_equal(np.asarray(r["new_p"], dtype=np.float64), p)


def test_five_points_are_too_few(oracle):
    m, nrm, p = P.five()
    for dtype in (np.float64, np.longdouble):
        r = P.plane_ref(oracle, m, nrm, p, 0.0, 3, -1.0, dtype)
        assert r["status"] == "few" and r["fail_iter"] == 0 and r["K_fail"] == 5 and r["K"] == []
        np.testing.assert_array_equal(np.asarray(r["new_p"], dtype=np.float64), p)


def test_purpose_inputs(oracle):
    """A different sample of the same surface: point-to-plane lands on the pose, point-to-point
    with scale does not (tests/test_gpu_plane.py asserts the same of the engine)."""
    m, nrm, p, src = P.synth(4097, 4197, 0.0, other=True)
    r = P.plane_ref(oracle, m, nrm, p, 0.0, 5, -1.0)
    u = oracle.icp(m, p, 10)
    dplane, dpoint = float(np.abs(r["new_p"] - src).max()), float(np.abs(u["new_p"] - src).max())
    print("plane", dplane, "point", dpoint)
    assert dplane < 1e-3 and dpoint > 1e-2


def test_abi_without_a_device(icp_lib):
    amd = icp_lib
    L = amd.lib()
    n = np.zeros((4, 3))
    assert L.icp_set_metric(None, amd.METRIC_POINT_TO_PLANE) == amd.ICP_E_ARG
    assert L.icp_set_model_normals(None, n.ctypes.data_as(C.POINTER(C.c_double)), 4) == amd.ICP_E_ARG
    assert L.icp_set_model_normals_device(None, None, 4) == amd.ICP_E_ARG
    assert amd.ICP_E_DEGENERATE == -10 and amd.strerror(-10) not in ("", "unknown error")
    assert (amd.METRIC_POINT_TO_POINT, amd.METRIC_POINT_TO_PLANE) == (0, 1)
