"""icp_filter_statistical / icp_filter_radius and their device forms are part of the C ABI: the built
library exports them, include/icp_capi.h declares them, and the binding lists and wraps them (CPU:
nothing here needs a device)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("icp_filter_statistical", "icp_filter_statistical_device", "icp_filter_radius", "icp_filter_radius_device")


def test_filters_are_exported_declared_and_listed(icp_lib):
    with open(os.path.join(ROOT, "include", "icp_capi.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(icp_lib.lib(), name)
        assert re.search(r"^int %s\(icp_ctx \*ctx, const double \*xyz(_dev)?, size_t n, " % name, header, re.M), name
        assert name in icp_lib.EXPORTED
        assert callable(getattr(icp_lib.Context, name[len("icp_"):], None))
    # the rules are stated where the declarations are
    for phrase in ("icp_filter_statistical(k, std_ratio):", "icp_filter_radius(radius, min_neighbors):",
                   "T = mu + std_ratio * sigma", "c_j > min_neighbors"):
        assert phrase in header, phrase


def test_a_null_context_is_an_argument_error(icp_lib):
    L = icp_lib.lib()
    xyz = (C.c_double * 12)(*range(12))
    n_out = C.c_size_t(77)
    assert L.icp_filter_statistical(None, xyz, 4, 2, 1.0, None, None, C.byref(n_out), None, None) == icp_lib.ICP_E_ARG
    assert L.icp_filter_statistical_device(None, None, 4, 2, 1.0, None, None, C.byref(n_out), None,
                                           None) == icp_lib.ICP_E_ARG
    assert L.icp_filter_radius(None, xyz, 4, 1.0, 1, None, None, C.byref(n_out), None) == icp_lib.ICP_E_ARG
    assert L.icp_filter_radius_device(None, None, 4, 1.0, 1, None, None, C.byref(n_out), None) == icp_lib.ICP_E_ARG
    assert n_out.value == 77  # (nothing written)
