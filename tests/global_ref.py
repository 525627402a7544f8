"""The reference of global registration (icp_fpfh, icp_match_features, icp_ransac_pose; icp_global.hip),
restated in numpy in the header's operation order, and the named inputs of its tests
(tests/test_global_ref.py on the CPU, tests/test_gpu_global.py, tests/test_gpu_global_cli.py).

Every dot product and 3-term sum is ((a + b) + c); numpy evaluates each +, -, *, /, sqrt and floor in
IEEE fp64, so everything but atan2 has the engine's bits.  f1 = atan2(...) only chooses a bin: a row is
compared on the GPU when every f1 it depends on (its own pairs' and its listed neighbours') lies at least
EDGE_CLEAR of a bin from an edge.  The 3-point pose calls icp_amd.horn_solve: the engine's own Horn code
on the host; a hypothesis's count is reported at max_dist (1 - BRACKET) and max_dist (1 + BRACKET).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import normals_ref as N
import plane_ref as P
import voxel_ref as V

DIM = 33
EDGE_CLEAR = 1e-9   # of a bin: the f1 filter
BRACKET = 1e-9      # relative, on max_dist: the count's bracket
FILTER_MAX = 0.01   # the filter may leave out at most this share of a case's rows
BRACKET_MAX = 0.01  # the bracket may be open for at most this share of a case's hypotheses
GAMMA = np.uint64(0x9E3779B97F4A7C15)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def bins(u):
    """clamp(floor(11 u), 0, 10); a NaN goes to bin 0"""
    with np.errstate(invalid="ignore"):
        f = np.floor(11.0 * u)
        return np.where(f >= 0.0, np.minimum(f, 10.0), 0.0).astype(np.int64)


def fpfh_ref(x, normals, k):
    """-> dict(idx, d2 (n, k): the lists; spfh, fpfh (n, 33); counted (n,): c_i; spfh_ok, fpfh_ok (n,) bool:
    the rows the f1 filter lets a GPU test compare)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nr = np.ascontiguousarray(normals, dtype=np.float64)
    n = x.shape[0]
    idx, d2, _ = N.knn(x, k)
    me = np.arange(n)[:, None]
    xi, ni = x[:, None, :], np.broadcast_to(nr[:, None, :], (n, k, 3))
    xj, nj = x[idx], nr[idx]
    d = xj - xi
    L2 = dot(d, d)
    zero_i = (ni == 0.0).all(axis=-1)
    zero_j = (nj == 0.0).all(axis=-1)
    ok = (idx != me) & (L2 != 0.0) & ~zero_i & ~zero_j
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.sqrt(L2)
        a1 = dot(ni, d) / L
        a2 = dot(nj, d) / L
        swap = (np.abs(a1) < np.abs(a2))[..., None]
        n1 = np.where(swap, nj, ni)
        n2 = np.where(swap, ni, nj)
        e = np.where(swap, -d, d)
        f3 = np.where(swap[..., 0], -a2, a1)
        v = cross(e, n1)
        vl2 = dot(v, v)
        ok = ok & (vl2 != 0.0)
        v = v / np.sqrt(vl2)[..., None]
        w = cross(n1, v)
        f2 = dot(v, n2)
        f1 = np.arctan2(dot(w, n2), dot(n1, n2))
        u1 = (f1 + np.pi) / (2.0 * np.pi)
        b1, b2, b3 = bins(u1), bins((f2 + 1.0) / 2.0), bins((f3 + 1.0) / 2.0)
        s1 = 11.0 * u1
        clear = np.abs(s1 - np.round(s1)) >= EDGE_CLEAR
    cnt = np.zeros(n * DIM, dtype=np.int64)
    rows = np.broadcast_to(me, (n, k))
    for b, off in ((b1, 0), (b2, 11), (b3, 22)):
        cnt += np.bincount((rows * DIM + off + b)[ok], minlength=n * DIM)
    cnt = cnt.reshape(n, DIM)
    c = ok.sum(axis=1)
    with np.errstate(divide="ignore"):
        scale = np.where(c > 0, 100.0 / c.astype(np.float64), 0.0)
    spfh = np.where((c > 0)[:, None], cnt.astype(np.float64) * scale[:, None], 0.0)
    A = np.zeros((n, DIM))
    for s in range(k):  # (the list's order)
        j, dd = idx[:, s], d2[:, s]
        use = (j != me[:, 0]) & (dd > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = (1.0 / dd)[:, None] * spfh[j]
        A = np.where(use[:, None], A + term, A)
    for t0 in (0, 11, 22):
        T = np.zeros(n)
        for b in range(11):
            T = T + A[:, t0 + b]
        with np.errstate(divide="ignore", invalid="ignore"):
            A[:, t0:t0 + 11] = np.where((T > 0.0)[:, None], A[:, t0:t0 + 11] * (100.0 / T)[:, None], 0.0)
    spfh_ok = (clear | ~ok).all(axis=1)
    return dict(idx=idx, d2=d2, spfh=spfh, fpfh=A + spfh, counted=c, spfh_ok=spfh_ok,
                fpfh_ok=spfh_ok & spfh_ok[idx].all(axis=1))


def match_ref(fa, fb, chunk=256):
    """-> (idx (na,) int32: the lowest minimiser, -1 when every D is a NaN; D (na,): its distance, NaN at -1)"""
    fa = np.ascontiguousarray(fa, dtype=np.float64)
    fb = np.ascontiguousarray(fb, dtype=np.float64)
    idx = np.empty(fa.shape[0], dtype=np.int32)
    dist = np.empty(fa.shape[0])
    for a0 in range(0, fa.shape[0], chunk):
        q = fa[a0:a0 + chunk]
        D = np.zeros((q.shape[0], fb.shape[0]))
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(DIM):  # (from +0 in ascending c, the difference before the product)
                d = q[:, c][:, None] - fb[:, c][None, :]
                D = D + d * d
        valid = ~np.isnan(D)
        lo = np.where(valid, D, np.inf).min(axis=1)
        first = np.argmax(valid & (D == lo[:, None]), axis=1)
        some = valid.any(axis=1)
        idx[a0:a0 + chunk] = np.where(some, first, -1)
        dist[a0:a0 + chunk] = np.where(some, lo, np.nan)
    return idx, dist


def mutual(idx_ab, idx_ba):
    """the rows a of the first set that the mutual filter keeps"""
    a = np.arange(idx_ab.size)
    ok = idx_ab >= 0
    keep = np.zeros(idx_ab.size, dtype=bool)
    keep[ok] = idx_ba[idx_ab[ok]] == a[ok]
    return np.nonzero(keep)[0]


def splitmix64(x):
    x = x.astype(np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw(seed, H, C):
    """-> (H, 3) int64: the three pair indices of the hypotheses 0 .. H - 1"""
    h = np.arange(H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = [splitmix64(np.uint64(seed) + (np.uint64(3) * h + np.uint64(r + 1)) * GAMMA) for r in range(3)]
    i0 = (z[0] % np.uint64(C)).astype(np.int64)
    i1 = (z[1] % np.uint64(C - 1)).astype(np.int64)
    i1 = i1 + (i1 >= i0)
    i2 = (z[2] % np.uint64(C - 2)).astype(np.int64)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.stack([i0, i1, i2], axis=1)


def rows3(R, x):
    """((R0 x0 + R1 x1) + R2 x2) per row, x (n, 3) -> (n, 3)"""
    return np.stack([(R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1]) + R[r, 2] * x[:, 2] for r in range(3)], axis=1)


def ransac_ref(p, q, H, seed, max_dist, edge_ratio, horn_solve):
    """-> dict(ids (H, 3), kept (H,) bool, lo, hi (H,) int: the count's bracket (-1 where rejected), mid: the
    count at max_dist itself, poses {h: (R, t)}, open (how many kept hypotheses have lo != hi)); horn_solve =
    None: the draw and the edge check alone (ids, kept)"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    C = p.shape[0]
    ids = draw(seed, H, C)
    P3, Q3 = p[ids], q[ids]  # (H, 3, 3)
    e2 = edge_ratio * edge_ratio
    kept = np.ones(H, dtype=bool)
    for r in range(3):
        dp, dq = P3[:, r] - P3[:, (r + 1) % 3], Q3[:, r] - Q3[:, (r + 1) % 3]
        lp, lq = dot(dp, dp), dot(dq, dq)
        kept &= np.minimum(lp, lq) >= e2 * np.maximum(lp, lq)
    if horn_solve is None:
        return dict(ids=ids, kept=kept)
    mp = ((P3[:, 0] + P3[:, 1]) + P3[:, 2]) / 3.0
    mq = ((Q3[:, 0] + Q3[:, 1]) + Q3[:, 2]) / 3.0
    S = np.zeros((H, 3, 3))
    d_caps, sp = np.zeros(H), np.zeros(H)
    for r in range(3):
        pc, qc = P3[:, r] - mp, Q3[:, r] - mq
        S = S + pc[:, :, None] * qc[:, None, :]
        d_caps = d_caps + dot(qc, qc)
        sp = sp + dot(pc, pc)
    lo = np.full(H, -1, dtype=np.int64)
    hi = np.full(H, -1, dtype=np.int64)
    mid = np.full(H, -1, dtype=np.int64)
    d_lo, d_hi = max_dist * (1.0 - BRACKET), max_dist * (1.0 + BRACKET)
    poses = {}
    for h in np.nonzero(kept)[0]:
        with np.errstate(all="ignore"):
            _, R, _ = horn_solve(S[h].reshape(-1), mp[h], mq[h], float(d_caps[h]), float(sp[h]))
            t = mq[h] - rows3(R, mp[h][None, :])[0]
            dd = (rows3(R, p) + t[None, :]) - q
            r2 = dot(dd, dd)
            lo[h] = int((r2 <= d_lo * d_lo).sum())
            hi[h] = int((r2 <= d_hi * d_hi).sum())
            mid[h] = int((r2 <= max_dist * max_dist).sum())
        poses[int(h)] = (R, t)
    return dict(ids=ids, kept=kept, lo=lo, hi=hi, mid=mid, poses=poses, open=int((lo != hi).sum()))


def winner(counts):
    """the rule on a counts array: the largest count, ties to the lowest h -> (h, count)"""
    h = int(np.argmax(counts))  # (the first maximum)
    return h, int(counts[h])


def angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


# ---- inputs -----------------------------------------------------------------------------------------

COW_VOXEL = 0.12
COW_ANGLE, COW_AXIS, COW_SHIFT = 120.0, (1.0, 2.0, 3.0), (0.5, -0.3, 0.8)
PURPOSE_SEED = 1  # (tests/test_global_ref.py: the reference's own pose for this seed is inside 5 degrees)


def lattice_plane():
    g = np.arange(12, dtype=np.float64)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    # (a tilt: the unit normal has three non-zero components)
    R = P.rot((1.0, -2.0, 0.5), 33.0)
    return np.concatenate([xy, np.zeros((xy.shape[0], 1))], axis=1) @ R.T


def cow(load):
    import datasets
    return load(datasets.path("cow_ref"))


def cow_pair(load):
    """-> (m, p, R_true, t_true) with m = R_true p + t_true: the cow against itself turned and shifted"""
    m = cow(load)
    Rt = P.rot(COW_AXIS, COW_ANGLE)
    p = m @ Rt.T + np.asarray(COW_SHIFT)
    return m, p, Rt.T, -(Rt.T @ np.asarray(COW_SHIFT))


def cloud(name, load=None):
    """The named descriptor input -> (x, k)."""
    if name.startswith("ell"):  # "ell<n>k<k>"
        n, _, k = name[3:].partition("k")
        return P.ellipsoid(int(n), 300 + int(n))[0], int(k)
    if name == "cow":
        return V.coarse_rule(cow(load), COW_VOXEL), 32
    if name == "plane":
        return lattice_plane(), 16
    if name == "duplicates":
        m = P.ellipsoid(257, 557)[0]
        return np.concatenate([m, m[:40]]), 32
    if name == "line":
        return N.line(), 8
    raise KeyError(name)


FPFH_CASES = ("ell5k3", "ell5k5", "ell63k32", "ell64k32", "ell65k32", "ell64k64", "ell257k32", "ell4096k32",
              "ell4097k32", "cow", "plane", "duplicates", "line")
K_NORMALS = 16  # (min(K_NORMALS, n) for the clouds of fewer points)


def planted(C=200, good=120, seed=77):
    """C pairs, the first `good` exact pairs of a known pose, the rest random -> (p, q, R, t)"""
    r = np.random.default_rng(seed)
    p = r.uniform(-1.0, 1.0, (C, 3))
    R = P.rot((0.3, -1.0, 0.6), 70.0)
    t = np.array([0.4, -0.2, 0.9])
    q = p @ R.T + t
    q[good:] = r.uniform(-1.0, 1.0, (C - good, 3)) + t
    return p, q, R, t


def noisy_pairs(C, seed, sigma=0.02, outliers=0.3):
    """C pairs of a pose with noise and a share of random ones: counts that differ between hypotheses"""
    r = np.random.default_rng(seed)
    p = r.uniform(-1.0, 1.0, (C, 3))
    R = P.rot((1.0, 0.2, -0.4), 40.0)
    q = p @ R.T + np.array([0.1, 0.2, -0.3]) + sigma * r.standard_normal((C, 3))
    bad = r.uniform(size=C) < outliers
    q[bad] = r.uniform(-1.0, 1.0, (int(bad.sum()), 3))
    return p, q


# (C, H, seed, max_dist, edge_ratio)
RANSAC_CASES = {"c3h1": (3, 1, 5, 0.1, 0.0), "c4": (4, 64, 6, 0.1, 0.5), "c64": (64, 63, 7, 0.08, 0.7),
                "c65": (65, 65, 8, 0.08, 0.7), "h64": (40, 64, 9, 0.08, 0.6), "h4000": (65, 4000, 10, 0.08, 0.8)}


def ransac_case(name):
    C, H, seed, max_dist, edge = RANSAC_CASES[name]
    p, q = noisy_pairs(C, 900 + C + H)
    return p, q, H, seed, max_dist, edge
