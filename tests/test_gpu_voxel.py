"""icp_voxel_downsample / icp_voxel_downsample_device (icp_voxel.hip) against tests/voxel_ref.py.

Cell membership is exact: n_out, every count, and every output point compared with the mean of the
reference partition's cell of the same rank.  A mean must satisfy the any-order bound
|mean - mean_longdouble| <= (L + 1) 2^-53 max_i |x_i| per axis (voxel_ref.mean_bound), which holds for
any summation order plus the division: no measured tolerance.

The bits are the header's too (item 4, the order of the sum): every mean equals voxel_ref.rule_means, a
plain numpy restatement of the rule, as uint64 -- whichever of the kernel's three forms took the cell.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the first HIP call of the session: torch then sees the device)

import datasets
import voxel_ref as V

pytestmark = pytest.mark.gpu

_REF = {}


def ref(name):
    """(xyz, voxel, origin, means longdouble, counts, bound, the order rule's means): computed once, shared,
    never changed."""
    if name not in _REF:
        xyz, voxel, origin = V.case(name)
        mean, counts, rank = V.downsample_ref(xyz, voxel, origin)
        _REF[name] = (xyz, voxel, origin, mean, counts, V.mean_bound(xyz, rank, counts),
                      V.rule_means(xyz, rank, counts.size))
    return _REF[name]


@pytest.fixture(scope="module")
def ctx(icp_lib):
    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as c:
        yield c


def device_form(ctx, xyz, voxel, origin):
    d = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    out = torch.full((xyz.shape[0], 3), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((xyz.shape[0],), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    k = ctx.voxel_downsample_device(d.data_ptr(), xyz.shape[0], voxel, out.data_ptr(), origin, cnt.data_ptr())
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    assert (out[k:] == -7.0).all() and (cnt[k:] == -7).all()  # (nothing past the outputs)
    return out[:k], cnt[:k]


@pytest.mark.parametrize("name", V.CASES + V.BIG_CASES)
def test_matches_reference(ctx, name):
    xyz, voxel, origin, mean, counts, bound = ref(name)[:6]
    got, got_counts = ctx.voxel_downsample(xyz, voxel, origin, counts=True)
    assert got.shape[0] == counts.size
    assert np.array_equal(got_counts, counts)
    gap = np.abs(got.astype(np.longdouble) - mean).astype(np.float64)
    print(f"{name}: {counts.size} cells, largest {counts.max()}, worst gap / bound "
          f"{np.max(gap / np.maximum(bound, 1e-300)):.3f}")
    assert (gap <= bound).all()
    # without the counts: the same points
    assert np.array_equal(ctx.voxel_downsample(xyz, voxel, origin).view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("name", V.CASES + V.BIG_CASES)
def test_means_follow_the_order_rule(ctx, name):
    """The promised bits: chunks of 1,024, 64 lane sums from +0, the xor butterfly, the chunk sums in
    order from +0, one division -- not merely some order inside the any-order bound."""
    xyz, voxel, origin, _, counts, _, rule = ref(name)
    got, got_counts = ctx.voxel_downsample(xyz, voxel, origin, counts=True)
    assert got.shape[0] == counts.size
    assert np.array_equal(got_counts, counts)
    differ = (got.view(np.uint64) != rule.view(np.uint64)).any(axis=1)
    print(f"{name}: n_out {got.shape[0]}, largest cell {got_counts.max()}, {int(differ.sum())} cells differ from the rule"
          + (f" (lengths {sorted(set(counts[differ].tolist()))[:20]})" if differ.any() else ""))
    assert not differ.any()


@pytest.mark.parametrize("name", ["lengths", "wide48"])
def test_device_form_writes_nothing_past_the_outputs(ctx, name):
    """Rows n_out .. n - 1 of xyz_out and count_out keep their fill (device_form checks it), and the
    rows before them are the rule's."""
    xyz, voxel, origin, _, counts, _, rule = ref(name)
    d, cd = device_form(ctx, xyz, voxel, origin)
    assert d.shape[0] == counts.size < xyz.shape[0]
    assert np.array_equal(cd, counts) and np.array_equal(d.view(np.uint64), rule.view(np.uint64))


def test_sums_start_from_plus_zero(ctx):
    """A cell of three points (the eight-lane form) and one of 70 (the whole wave), x = -0.0 throughout:
    the mean's x has the bits of +0.0."""
    xyz, voxel, origin = V.negative_zero_case()
    _, counts, rank = V.downsample_ref(xyz, voxel, origin)
    got, got_counts = ctx.voxel_downsample(xyz, voxel, origin, counts=True)
    assert got_counts.tolist() == counts.tolist() == [3, 70]
    assert got[:, 0].view(np.uint64).tolist() == [0, 0]
    assert np.array_equal(got.view(np.uint64), V.rule_means(xyz, rank, 2).view(np.uint64))
    d, _ = device_form(ctx, xyz, voxel, origin)
    assert np.array_equal(d.view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("name", ["n1", "n4097", "one_cell4097", "one_cell70000", "mixed", "wide", "shared_a", "cow",
                                  "lengths", "long_many", "wide63"])
def test_forms_and_calls_give_the_same_bits(ctx, name):
    xyz, voxel, origin = ref(name)[:3]
    a, ca = ctx.voxel_downsample(xyz, voxel, origin, counts=True)
    b, cb = ctx.voxel_downsample(xyz, voxel, origin, counts=True)
    d, cd = device_form(ctx, xyz, voxel, origin)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(ca, cb)
    assert np.array_equal(a.view(np.uint64), d.view(np.uint64)) and np.array_equal(ca, cd)


def test_shared_origin_is_one_lattice(ctx):
    (xa, voxel, origin), (xb, _, _) = ref("shared_a")[:3], ref("shared_b")[:3]
    a = ctx.voxel_downsample(xa, voxel, origin)
    b = ctx.voxel_downsample(xb, voxel, origin)
    both = ctx.voxel_downsample(np.concatenate([xa, xb]), voxel, origin, counts=True)[1]
    # a cell occupied in both clouds is one cell of the union: the lattices coincide
    ka = {tuple(c) for c in np.floor((a - np.asarray(origin)) / voxel).astype(np.int64)}
    kb = {tuple(c) for c in np.floor((b - np.asarray(origin)) / voxel).astype(np.int64)}
    assert len(ka) == a.shape[0] and len(kb) == b.shape[0]
    assert both.size == len(ka | kb) and both.sum() == xa.shape[0] + xb.shape[0]


def test_run_is_unchanged_by_a_downsample(icp_lib):
    m = icp_lib.load_matrix(datasets.path("cow_ref"))
    p = icp_lib.load_matrix(datasets.path("cow_tr2"))
    with icp_lib.Context(0, icp_lib.NN_CERTIFIED) as c:
        c.set_model(m)
        c.set_scene(p)
        r1, e1 = c.run(6)
        s1, i1 = c.get_scene(), c.get_indices()
        c.voxel_downsample(m, V.extent(m) / 16)
        c.set_scene(p)
        c.voxel_downsample(p, V.extent(m) / 16)
        r2, e2 = c.run(6)
        s2, i2 = c.get_scene(), c.get_indices()
    assert r1.iterations == r2.iterations == 6
    assert np.array_equal(e1.view(np.uint64), e2.view(np.uint64))
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64)) and np.array_equal(i1, i2)


# ---- errors: every row of the header's list; nothing is written to the outputs ------------------

def raw_call(icp_lib, ctx, xyz, n, voxel, origin, out, n_out):
    dp = C.POINTER(C.c_double)
    return icp_lib.lib().icp_voxel_downsample(
        ctx._h, None if xyz is None else xyz.ctypes.data_as(dp), n, voxel,
        None if origin is None else np.asarray(origin, dtype=np.float64).ctypes.data_as(dp),
        None if out is None else out.ctypes.data_as(dp), None, None if n_out is None else C.byref(n_out))


def test_errors(icp_lib, ctx):
    E_ARG, E_RANGE = icp_lib.ICP_E_ARG, icp_lib.ICP_E_RANGE
    xyz = np.ascontiguousarray(V.case("n65")[0])
    bad = xyz.copy()
    bad[17, 1] = np.nan
    inf = xyz.copy()
    inf[3, 2] = np.inf
    rows = [
        ("xyz null", E_ARG, dict(xyz=None)),
        ("xyz_out null", E_ARG, dict(out=None)),
        ("n_out null", E_ARG, dict(n_out=None)),
        ("n == 0", E_ARG, dict(n=0)),
        ("n > INT_MAX", E_ARG, dict(n=2 ** 31)),  # (refused before anything is read)
        ("voxel 0", E_ARG, dict(voxel=0.0)),
        ("voxel < 0", E_ARG, dict(voxel=-0.5)),
        ("voxel nan", E_ARG, dict(voxel=float("nan"))),
        ("voxel inf", E_ARG, dict(voxel=float("inf"))),
        ("origin nan", E_ARG, dict(origin=(0.0, float("nan"), 0.0))),
        ("origin inf", E_ARG, dict(origin=(float("-inf"), 0.0, 0.0))),
        ("coordinate nan", E_ARG, dict(xyz=bad)),
        ("coordinate inf", E_ARG, dict(xyz=inf)),
        ("below the origin", E_RANGE, dict(origin=(0.0, 0.5, 0.0))),
        ("g > 2^21", E_RANGE, dict(voxel=2.0 ** -22)),
    ]
    for what, code, change in rows:
        out = np.full((65, 3), -7.0)
        n_out = C.c_size_t(12345)
        args = dict(xyz=xyz, n=65, voxel=0.25, origin=None, out=out, n_out=n_out)
        args.update(change)
        rc = raw_call(icp_lib, ctx, **args)
        assert rc == code, (what, rc, icp_lib.lib().icp_last_error(ctx._h))
        assert (out == -7.0).all() and n_out.value == 12345, what
    msg = icp_lib.lib().icp_last_error(ctx._h).decode()
    assert "x axis" in msg and "2^21" in msg, msg
    raw_call(icp_lib, ctx, xyz=xyz, n=65, voxel=0.25, origin=(0.0, 0.5, 0.0), out=np.empty((65, 3)), n_out=C.c_size_t(0))
    assert " y = " in icp_lib.lib().icp_last_error(ctx._h).decode()
    # g = 2^21 an axis is still inside
    line = np.zeros((2, 3))
    line[1, 0] = 1.0 - 2.0 ** -30
    assert ctx.voxel_downsample(line, 2.0 ** -21).shape[0] == 2
    # the device form: a non-finite coordinate is ICP_E_RANGE, as icp_set_model_device's; the outputs stay
    d = torch.from_numpy(bad).cuda()
    o = torch.full((65, 3), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(icp_lib.ICPError) as e:
        ctx.voxel_downsample_device(d.data_ptr(), 65, 0.25, o.data_ptr())
    assert e.value.code == E_RANGE
    assert bool((o == -7.0).all())
    with pytest.raises(icp_lib.ICPError) as e:
        ctx.voxel_downsample_device(d.data_ptr(), 65, 0.25, 0)
    assert e.value.code == E_ARG
    # the context still works
    assert ctx.voxel_downsample(xyz, 0.25).shape[0] == V.downsample_ref(xyz, 0.25)[1].size
