"""icp_set_one_to_one is part of the C ABI: the built library exports it, include/icp_capi.h declares
it, and the binding lists it (CPU: nothing here needs a device)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_to_one_is_exported_declared_and_listed(icp_lib):
    assert hasattr(icp_lib.lib(), "icp_set_one_to_one")
    with open(os.path.join(ROOT, "include", "icp_capi.h")) as f:
        header = f.read()
    assert re.search(r"^int icp_set_one_to_one\(icp_ctx \*ctx, int on\);", header, re.M)
    assert "icp_set_one_to_one" in icp_lib.EXPORTED
    assert callable(getattr(icp_lib.Context, "set_one_to_one", None))


def test_null_context_and_bad_values_are_argument_errors(icp_lib):
    L = icp_lib.lib()
    for on in (0, 1, 2, -1):
        assert L.icp_set_one_to_one(None, on) == icp_lib.ICP_E_ARG
