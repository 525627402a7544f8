"""icp_evaluate and its device form are part of the C ABI: the built library exports them,
include/icp_capi.h declares them and states their rules, and the binding lists and wraps them (CPU:
nothing here needs a device)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("icp_evaluate", "icp_evaluate_device")


def test_evaluate_is_exported_declared_and_listed(icp_lib):
    with open(os.path.join(ROOT, "include", "icp_capi.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(icp_lib.lib(), name)
        assert re.search(r"^int %s\(icp_ctx \*ctx, double max_dist, int both, icp_evaluation \*out, " % name, header,
                         re.M), name
        assert name in icp_lib.EXPORTED
        assert callable(getattr(icp_lib.Context, name[len("icp_"):], None))
    assert callable(icp_lib.evaluate_registration)
    assert "typedef struct icp_evaluation {" in header
    # the rules are stated where the declarations are
    for phrase in ("d2_j <= D", "A33 = A44 = A55 = K", "(dx*dx + dy*dy) + dz*dz", "fitness = K / np"):
        assert phrase in header, phrase
    # the binding's structure is the header's: the fields in order, 8 bytes each
    body = header[header.index("typedef struct icp_evaluation {"):header.index("} icp_evaluation;")]
    fields = []
    for line in body.splitlines()[1:]:
        decl = line.split("/*")[0].strip().rstrip(";")
        if decl:
            fields += [w.strip().split("[")[0] for w in decl.split(" ", 2 if decl.startswith("long long") else 1)[-1].split(",")]
    assert fields == [k for k, _ in icp_lib.Evaluation._fields_]
    assert C.sizeof(icp_lib.Evaluation) == 8 * (len(fields) - 1 + 36)


def test_a_null_context_is_an_argument_error(icp_lib):
    L = icp_lib.lib()
    out = icp_lib.Evaluation()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    assert L.icp_evaluate(None, 1.0, 0, C.byref(out), None, None, None, None) == icp_lib.ICP_E_ARG
    assert L.icp_evaluate_device(None, 1.0, 1, C.byref(out), None, None, None, None) == icp_lib.ICP_E_ARG
    assert bytes(out) == before  # (nothing written)
