"""The device memory of the calls on a cloud that is not the resident model (engine::Scratch, icp_engine.h):
the filters take theirs from one block the context keeps, icp_fpfh and the scene's estimator allocate and
free theirs inside the call.  What that can get wrong is an array left over from another call or another
size: on ONE context a sequence of calls of different kinds and sizes -- the first with the block still
empty (every array an allocation of the call's own), the second growing the block, later ones inside it --
must give, bit for bit, what each call gives as the first call on a fresh context; and a refused call in
between writes nothing and changes nothing.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import filter_ref as F
import plane_ref as P

pytestmark = pytest.mark.gpu

SMALL, BIG, MID = F.cloud("ell65"), F.cloud("ell4097"), F.cloud("ell257")
MODEL, SCENE = F.cloud("ell193"), np.ascontiguousarray(P.ellipsoid(193, 294)[0])
RADIUS = 0.05 * float(np.linalg.norm(BIG.max(axis=0) - BIG.min(axis=0)))


def stat_host(c):  # step 1: the host form, every optional output
    return c.filter_statistical(SMALL, 16, 2.0, mask=True, mean_dist=True, stats=True)


def radius_device(c):  # step 2: the device form with the full counts
    n = BIG.shape[0]
    d = torch.from_numpy(BIG).cuda()
    out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    kept = c.filter_radius_device(d.data_ptr(), n, RADIUS, 2, out.data_ptr(), mask.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    return kept, out[:kept].cpu().numpy(), mask.cpu().numpy(), cnt.cpu().numpy()


def stat_device(c):  # step 3
    n = MID.shape[0]
    d = torch.from_numpy(MID).cuda()
    out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mean = torch.zeros(n, dtype=torch.float64, device="cuda")
    kept, stats = c.filter_statistical_device(d.data_ptr(), n, 16, 2.0, out.data_ptr(), mask.data_ptr(), mean.data_ptr())
    torch.cuda.synchronize()
    return kept, stats, out[:kept].cpu().numpy(), mask.cpu().numpy(), mean.cpu().numpy()


def fpfh(c):  # step 4: the normals estimated
    return c.fpfh(MID, 16, k_normals=16, spfh=True, return_normals=True)


def scene_normals(c):  # step 5
    c.set_model(MODEL)
    c.set_scene(SCENE)
    return c.estimate_scene_normals(8), c.scene_normals()


def model_normals(c):  # step 6 (the model of step 5)
    return c.estimate_model_normals(8), c.model_normals()


def fresh_model_normals(c):
    c.set_model(MODEL)
    return model_normals(c)


@pytest.fixture(scope="module")
def fresh(icp_lib):
    """every step as the first call on a context of its own"""
    ref = {}
    for step in (stat_host, radius_device, stat_device, fpfh, scene_normals, fresh_model_normals):
        with icp_lib.Context() as c:
            ref[step.__name__.replace("fresh_", "")] = step(c)
    return ref


def same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert not np.isnan(w.astype(np.float64)).any()
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, i)


def test_a_sequence_on_one_context_is_each_call_on_a_fresh_one(icp_lib, fresh):
    steps = (stat_host, radius_device, stat_device, fpfh, scene_normals, model_normals, stat_host, radius_device,
             radius_device)
    with icp_lib.Context() as c:
        got = [(step.__name__, step(c)) for step in steps]
    for i, (name, outs) in enumerate(got):
        print("step", i + 1, name, "outputs", [np.asarray(o).shape for o in outs])
        same(outs, fresh[name], "step %d (%s)" % (i + 1, name))
    same(got[6][1], got[0][1], "step 7 against step 1")
    same(got[7][1], got[1][1], "step 8 against step 2")
    same(got[8][1], got[1][1], "step 8, again, against step 2")


def test_a_refused_call_between_two_good_ones(icp_lib, fresh):
    amd = icp_lib
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    with amd.Context() as c:
        same(stat_host(c), fresh["stat_host"], "before the refusal")
        n = SMALL.shape[0]
        out, mask, mean, stats = np.full((n, 3), -7.0), np.full(n, 9, dtype=np.uint8), np.full(n, -7.0), np.full(3, -7.0)
        n_out = C.c_size_t(99)
        rc = amd.lib().icp_filter_statistical(c._h, dp(SMALL), n, 0, 2.0, dp(out), mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              C.byref(n_out), dp(mean), dp(stats))
        msg = amd.lib().icp_last_error(c._h).decode()
        print(rc, msg)
        assert rc == amd.ICP_E_ARG and "k = 0" in msg
        assert (out == -7.0).all() and (mask == 9).all() and (mean == -7.0).all() and (stats == -7.0).all()
        assert n_out.value == 99
        same(stat_host(c), fresh["stat_host"], "after the refused filter")
        same(fpfh(c), fresh["fpfh"], "before the refused fpfh")
        x17 = F.cloud("ell17")  # k_fpfh = 32 is in range and above the cloud's size
        outs = [np.full((17, 33), -7.0), np.full((17, 33), -7.0), np.full((17, 3), -7.0)]
        rc = amd.lib().icp_fpfh(c._h, dp(x17), 17, None, 16, None, 32, dp(outs[0]), dp(outs[1]), dp(outs[2]))
        msg = amd.lib().icp_last_error(c._h).decode()
        print(rc, msg)
        assert rc == amd.ICP_E_ARG and "k = 32 exceeds the cloud's 17 points" in msg
        assert all((o == -7.0).all() for o in outs)
        same(fpfh(c), fresh["fpfh"], "after the refused fpfh")
        same(radius_device(c), fresh["radius_device"], "a filter after them")
