"""voxel_ref — numpy restatements for the coarse-to-fine pieces (include/icp_capi.h: icp_voxel_downsample,
icp_get_transform, icp_transform_scene).  TEST INFRASTRUCTURE ONLY.

* partition / downsample_ref: the voxel downsample's contract.  The cells are fp64 exactly as the
  header writes them (floor((x - lo) / voxel), IEEE division); the means are np.longdouble.
* mean_bound: the any-order bound a mean must satisfy, (L + 1) 2^-53 max_i |x_i| per axis -- L - 1
  additions in any order lose at most (L - 1) u sum |x_i| <= (L - 1) u L max |x_i| of the sum, that is
  (L - 1) u max |x_i| of the mean, and the division one more u |mean| (u = 2^-53); the rest of the
  margin covers the second-order terms.
* rule_means: the header's order of the sum (chunks, lanes, butterfly), whose bits the engine promises;
  sequential_means: a plain sum in input order, which it is not.
* case(name): the named clouds of tests/test_gpu_voxel.py, generated from seeds (CASES, and BIG_CASES
  for the kernels' strided loops, length switches and wide keys).
* icp_steps / compose / pyramid_twin: numpy_twin's loop (its closest and find_alignment) keeping
  every iteration's step, the engine's composition rule in a chosen precision, and the coarse-to-fine
  twin built on them.
* G_REL: the measured gap between a composed total and the moved scene (test_voxel_ref.py).
"""
from __future__ import annotations

import numpy as np

import numpy_twin

U = 2.0 ** -53

# The largest gap, over the scene's points and axes, between the fp64 twin's composed total applied
# to the original scene and the twin's own moved scene, on cow_ref / cow_tr2 (12 iterations), divided
# by the scene's largest |coordinate|: measured by tests/test_voxel_ref.py::test_total_against_moved_scene,
# which prints it and checks it against this constant.  The device tests allow 8 x G_REL x max |p|.
G_REL = 1.2e-15  # (measured 1.15e-15: G = 3.55e-15 at max |p| = 3.10)

# the voxel of the cow pair's coarse level as a fraction of the model's extent (test_voxel_ref.py
# checks that the twin then needs at most half the plain run's iterations)
COW_VOXEL_DIV = 16
# the cow pair's pyramids that tests/test_gpu_pyramid.py runs against pyramid_twin (voxel = extent / d per
# level), each level PYRAMID_LEVEL_ITERS and the full clouds PYRAMID_FINE_ITERS iterations, threshold -1.
# Two fine iterations are what the default threshold takes after either pyramid (test_voxel_ref.py); from
# the third on err sits at its floor of 2.3e-11, where an ulp in the points is 2e-12 of it (residuals of
# 5e-6 between coordinates of 3) and a bound of a hundredth of rtol 1e-9 would rest on chance
COW_PYRAMIDS = ([16], [8, 16])
PYRAMID_LEVEL_ITERS = 10
PYRAMID_FINE_ITERS = 2


def extent(xyz: np.ndarray) -> float:
    return float((xyz.max(axis=0) - xyz.min(axis=0)).max())


def partition(xyz: np.ndarray, voxel: float, origin=None):
    """-> (lo (3,), g (3,) int64, key (n,) int64 per point, keys: the occupied cells' keys ascending,
    rank (n,): each point's cell as its index into keys)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    lo = xyz.min(axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
    c = np.floor((xyz - lo) / np.float64(voxel))
    assert (c >= 0).all() and (c < 2 ** 21).all()
    c = c.astype(np.int64)
    g = 1 + c.max(axis=0)
    key = (c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0]
    keys, rank = np.unique(key, return_inverse=True)
    return lo, g, key, keys, rank.reshape(-1)


def downsample_ref(xyz: np.ndarray, voxel: float, origin=None):
    """-> (means (n_out, 3) np.longdouble, counts (n_out,) int32, rank (n,))."""
    xyz = np.asarray(xyz, dtype=np.float64)
    _, _, _, keys, rank = partition(xyz, voxel, origin)
    counts = np.bincount(rank, minlength=keys.size).astype(np.int32)
    sums = np.zeros((keys.size, 3), dtype=np.longdouble)
    np.add.at(sums, rank, xyz.astype(np.longdouble))
    return sums / counts[:, None].astype(np.longdouble), counts, rank


def sequential_means(xyz: np.ndarray, rank: np.ndarray, n_out: int) -> np.ndarray:
    """A plain fp64 sum of each cell's points in input order, divided by the count (np.add.at adds
    one element at a time, in order)."""
    sums = np.zeros((n_out, 3))
    np.add.at(sums, rank, np.asarray(xyz, dtype=np.float64))
    return sums / np.bincount(rank, minlength=n_out)[:, None].astype(np.float64)


def rule_means(xyz: np.ndarray, rank: np.ndarray, n_out: int) -> np.ndarray:
    """The order of the sum as include/icp_capi.h states it (icp_voxel_downsample, item 4), in fp64:
    a cell's points in input order are cut into chunks of 1,024; in a chunk 64 partial sums start
    from +0 and take the points l, l + 64, ... in order and are combined by the butterfly
    a_l += a_(l xor 32), 16, 8, 4, 2, 1; the chunk sums are added, from +0, in chunk order; one
    division by the count.  Vectorised across the cells (rows of one chunk each, a block at a time)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    by_cell = np.argsort(rank, kind="stable")  # (a cell's points in input order)
    pts, cell = xyz[by_cell], rank[by_cell]
    counts = np.bincount(rank, minlength=n_out)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    pos = np.arange(pts.shape[0]) - first[cell]  # a point's position in its cell
    chunks = (counts + 1023) // 1024
    row0 = np.concatenate([[0], np.cumsum(chunks)[:-1]])
    row = row0[cell] + pos // 1024  # one row per (cell, chunk), ascending along pts
    lane, turn = pos % 64, (pos % 1024) // 64  # the lane's turn-th point of the chunk
    n_rows = int(chunks.sum())
    chunk_sums = np.empty((n_rows, 3))
    xor = np.arange(64)
    for r0 in range(0, n_rows, 8192):
        r1 = min(n_rows, r0 + 8192)
        a, b = np.searchsorted(row, [r0, r1])
        lanes = np.zeros((r1 - r0, 64, 3))  # +0
        # (a row and a lane at most once a turn: a plain indexed add, in turn order)
        for k in range(int(turn[a:b].max()) + 1):
            sel = np.flatnonzero(turn[a:b] == k) + a
            lanes[row[sel] - r0, lane[sel]] += pts[sel]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, xor ^ o]
        chunk_sums[r0:r1] = lanes[:, 0]
    sums = np.zeros((n_out, 3))  # +0
    row_cell = np.repeat(np.arange(n_out), chunks)
    row_chunk = np.arange(n_rows) - row0[row_cell]
    for c in range(int(chunks.max())):  # (a cell at most once a chunk index)
        sel = np.flatnonzero(row_chunk == c)
        sums[row_cell[sel]] += chunk_sums[sel]
    return sums / counts[:, None].astype(np.float64)


def mean_bound(xyz: np.ndarray, rank: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """(n_out, 3): (L + 1) 2^-53 max_i |x_i| per cell and axis."""
    mx = np.zeros((counts.size, 3))
    np.maximum.at(mx, rank, np.abs(np.asarray(xyz, dtype=np.float64)))
    return (counts[:, None].astype(np.float64) + 1.0) * U * mx


# ---- the named cases ---------------------------------------------------------------------------

SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 12289]

# "lengths": a cell on either side of every switch of icp_voxel.hip -- eight lanes / the whole wave (8 | 9),
# one turn a lane / two (64 | 65), one chunk / two (1,024 | 1,025), the means kernel / the listed cells'
# kernel (4,096 | 4,097), its one round of 16 chunks / two (16,384 | 16,385)
LENGTHS = [1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 16383, 16384, 16385, 32769]


def _uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def case(name: str):
    """-> (xyz, voxel, origin or None)"""
    if name.startswith("n"):  # n<size>: uniform points, about eight a cell from 4,095 points on
        n = int(name[1:])
        return _uniform(n, 100 + n), (0.5 if n < 100 else 0.125 if n < 5000 else 0.1), None
    if name.startswith("one_cell"):  # all points in one cell (the extent is below the voxel)
        n = int(name[len("one_cell"):])
        return _uniform(n, 200 + n) - 0.5, 2.0, None
    if name == "own_cell":  # every point in its own cell: a jittered 10 x 10 x 10 lattice, shuffled
        rng = np.random.default_rng(301)
        i = rng.permutation(1000)
        base = np.stack([i % 10, (i // 10) % 10, i // 100], axis=1).astype(np.float64)
        return base + 0.25 + 0.5 * rng.random((1000, 3)), 1.0, (0.0, 0.0, 0.0)
    if name == "mixed":  # 200 singletons, a cell of 65 points and a cell of 4,097 points, shuffled
        rng = np.random.default_rng(302)
        single = np.stack([np.arange(200.0), np.zeros(200), np.zeros(200)], axis=1) + rng.random((200, 3))
        a = np.array([3.0, 1.0, 0.0]) + rng.random((65, 3))
        b = np.array([5.0, 2.0, 1.0]) + rng.random((4097, 3))
        xyz = np.concatenate([single, a, b])
        return xyz[rng.permutation(xyz.shape[0])], 1.0, (0.0, 0.0, 0.0)
    if name in ("boundary_tenth", "boundary_eighth"):  # points on cell faces: coordinates k * voxel
        voxel = 0.1 if name == "boundary_tenth" else 2.0 ** -3
        rng = np.random.default_rng(303)
        k = rng.integers(0, 16, size=(600, 3)).astype(np.float64)
        on_face = rng.random((600, 3)) < 0.6
        xyz = np.where(on_face, k * voxel, (k + rng.random((600, 3))) * voxel)
        return xyz, voxel, (0.0, 0.0, 0.0)
    if name == "duplicates":  # every point three times
        rng = np.random.default_rng(304)
        xyz = np.repeat(rng.random((500, 3)), 3, axis=0)
        return xyz[rng.permutation(1500)], 0.2, None
    if name in ("shared_a", "shared_b"):  # two clouds on one lattice: an explicit origin below both
        rng = np.random.default_rng(305 if name == "shared_a" else 306)
        return rng.random((700, 3)) + (0.0 if name == "shared_a" else 0.3), 0.15, (-0.05, -0.05, -0.05)
    if name == "wide":  # extent 1, voxel 2^-12: g = 4,097 an axis, the key past 32 bits
        rng = np.random.default_rng(307)
        xyz = rng.random((257, 3))
        xyz[0] = 0.0
        xyz[1] = 1.0
        xyz[200:257] = xyz[100:157]  # (runs of two, apart in input order)
        return xyz, 2.0 ** -12, None
    if name == "lengths":  # one cell of each length of LENGTHS, consecutive along x in a shuffled order
        rng = np.random.default_rng(308)
        cell_len = rng.permutation(LENGTHS)
        xyz = rng.random((int(cell_len.sum()), 3))
        xyz[:, 0] += np.repeat(np.arange(cell_len.size, dtype=np.float64), cell_len)
        return xyz[rng.permutation(xyz.shape[0])], 1.0, (0.0, 0.0, 0.0)
    if name == "many_cells":  # more than two trips of the means kernel's 65,536 cells, all of them small
        return _uniform(200000, 309), 2.0 ** -6, (0.0, 0.0, 0.0)
    if name == "long_many":  # 260 cells of 4,097 points on a 20 x 13 lattice; the box from the cloud
        rng = np.random.default_rng(310)
        n = 260 * 4097
        c = np.repeat(np.arange(260), 4097)[rng.permutation(n)]
        base = np.stack([c % 20, c // 20, np.zeros(n, dtype=np.int64)], axis=1).astype(np.float64)
        xyz = base + 2.0 ** -12 + (1.0 - 2.0 ** -11) * rng.random((n, 3))
        # the two points that alone set the box's corners come last, past input position 2^20
        i_lo, i_hi = np.flatnonzero(c == 0)[-1], np.flatnonzero(c == 259)[-1]
        xyz[i_lo] = 0.0
        xyz[i_hi] = np.array([20.0, 13.0, 1.0]) - 2.0 ** -20
        rest = np.setdiff1d(np.arange(n), [i_lo, i_hi])
        return xyz[np.concatenate([rest, [i_lo, i_hi]])], 1.0, None
    if name in ("wide48", "wide63"):  # g = 2^16 / 2^21 an axis: the key's high word 16 / 31 bits
        b = 16 if name == "wide48" else 21
        rng = np.random.default_rng(311 if name == "wide48" else 312)
        c = rng.integers(0, 2 ** b, size=(9001, 3))
        c[0] = 0
        c[1] = 2 ** b - 1
        c[2000:3000, :2] = c[1000:2000, :2]  # x and y again, another z: equal low words, other high words
        # z again, another x (wide48: the high word is z; wide63: it is z and y's upper ten bits, so y too)
        c[4000:5000, (2 if b == 16 else 1):] = c[3000:4000, (2 if b == 16 else 1):]
        c[6000:6500] = c[5000:5500]  # whole cells again, 1,000 input positions on: runs of two over two tiles
        frac = rng.integers(0, 2 ** 20, size=(9001, 3))
        # dyadic coordinates: (x - 0) / voxel is exact
        return (c.astype(np.float64) + frac.astype(np.float64) * 2.0 ** -20) * 2.0 ** -b, 2.0 ** -b, (0.0, 0.0, 0.0)
    if name == "cow":
        import datasets
        import icp_amd
        m = icp_amd.load_matrix(datasets.path("cow_ref"))
        return m, extent(m) / COW_VOXEL_DIV, None
    raise KeyError(name)


CASES = (["n%d" % n for n in SIZES] + ["one_cell4097", "one_cell70000", "own_cell", "mixed", "boundary_tenth",
                                       "boundary_eighth", "duplicates", "shared_a", "shared_b", "wide", "cow"])
# the branches the cases above do not reach: the strided loops over cells, tiles and listed cells,
# every length switch in one call, a wide key over several tiles
BIG_CASES = ["lengths", "many_cells", "long_many", "wide48", "wide63"]


def negative_zero_case():
    """A cell of three points and a cell of 70, x = -0.0 throughout: the rule's sums start from +0, so
    both means' x is +0.0.  -> (xyz, voxel, origin)"""
    rng = np.random.default_rng(313)
    xyz = rng.random((73, 3))
    xyz[3:, 1] += 1.0  # (the second cell: one further along y)
    xyz[:, 0] = -0.0
    return xyz[rng.permutation(73)], 1.0, (-1.0, -1.0, -1.0)


# ---- the total transform and the coarse-to-fine twin ----------------------------------------------

def closest(p: np.ndarray, m: np.ndarray):
    """numpy_twin.closest over blocks of queries (its n x m x 3 temporaries stay small)."""
    idx = np.concatenate([numpy_twin.closest(p[i:i + 256], m)[1] for i in range(0, p.shape[0], 256)])
    return m[idx], idx


def icp_steps(m, p, max_iter: int, threshold: float = 1e-5):
    """numpy_twin.icp keeping every applied step -> (moved scene, errs, [(s, R, t), ...])."""
    new_p = p.copy()
    errs, steps = [], []
    for _ in range(max_iter):
        Y, _ = closest(new_p, m)
        s, R, t, e = numpy_twin.find_alignment(new_p, Y)
        new_p = new_p @ (s * R).T + t
        steps.append((s, R, t))
        err = (e + float(((Y - new_p) ** 2).sum())) / p.shape[0]
        errs.append(err)
        if err < threshold:
            break
    return new_p, np.array(errs), steps


def compose(steps, dtype=np.float64):
    """(s2, R2, t2) o (s1, R1, t1) = (s2 s1, R2 R1, s2 R2 t1 + t2) over the steps, first to last."""
    s, R, t = dtype(1.0), np.eye(3, dtype=dtype), np.zeros(3, dtype=dtype)
    for s2, R2, t2 in steps:
        s2, R2, t2 = dtype(s2), np.asarray(R2, dtype=dtype), np.asarray(t2, dtype=dtype)
        s, R, t = s2 * s, R2 @ R, (s2 * R2) @ t + t2
    return s, R, t


def apply(total, p):
    s, R, t = total
    return p.astype(R.dtype) @ (s * R).T + t


def coarse_longdouble(xyz, voxel):
    """The coarse cloud as the longdouble means rounded to fp64."""
    return downsample_ref(xyz, voxel)[0].astype(np.float64)


def coarse_rule(xyz, voxel):
    """The coarse cloud as the header's order rule gives it: the engine's bits."""
    _, _, _, keys, rank = partition(xyz, voxel)
    return rule_means(xyz, rank, keys.size)


def pyramid_twin(m, p, voxels, max_iter: int, level_iter: int, threshold: float = 1e-5, coarse=coarse_longdouble):
    """Coarse to fine: each level registers the downsampled clouds (coarse(cloud, voxel)) from the pose so far.
    -> (moved full scene, the fine run's errs, the total, [(model points, scene points, iterations, errs)])."""
    total = compose([])
    levels = []
    for h in voxels:
        mc = coarse(m, h)
        pc = coarse(p, h)
        _, errs, steps = icp_steps(mc, apply(total, pc), level_iter, threshold)
        total = compose([total] + steps)
        levels.append((mc.shape[0], pc.shape[0], len(errs), errs))
    moved, errs, steps = icp_steps(m, apply(total, p), max_iter, threshold)
    return moved, errs, compose([total] + steps), levels


def too_few_case():
    """A gated pair whose run stops with too few pairs AFTER two completed iterations (K = 4, 5, then
    3; tests/test_voxel_ref.py checks it with the gated reference loop): 7 model points, the scene
    the model with noise, the gate just above the fourth nearest pair.  -> (m, p, dmax, completed)"""
    r = np.random.default_rng(2099)
    m = r.uniform(-1, 1, size=(7, 3))
    p = m + 0.15 * r.standard_normal((7, 3))
    return m, p, 0.2532, 2
