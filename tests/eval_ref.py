"""The reference of icp_evaluate (icp_eval.hip): include/icp_capi.h's rules restated in numpy, and the
inputs of its tests (tests/test_eval_ref.py on the CPU, tests/test_gpu_eval.py).

  d2(a, b) = (dx*dx + dy*dy) + dz*dz in fp64 (numpy does not contract); the pair of a query is the FIRST
  minimum over the target in index order (np.argmin); kept iff d2 <= D = max_dist * max_dist; a point
  that is not kept has index -1 and d2 +inf.  Every sum is math.fsum, the exactly rounded sum, so that
  the reference takes no side on the device's sum order S; the tests allow S's rounding.
A helper module, not a conftest: no fixtures, no hooks.
"""
import math

import numpy as np

import datasets
import gated_ref as G
import normals_ref as NR
import plane_ref as P

CHUNK = 512  # queries a block of the brute force (CHUNK x n doubles, three at a time)


def nearest(q, m):
    """-> (the first-minimum index of every q in m, its d2)"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    m = np.ascontiguousarray(m, dtype=np.float64)
    idx = np.empty(q.shape[0], dtype=np.int32)
    d2 = np.empty(q.shape[0])
    for b in range(0, q.shape[0], CHUNK):
        e = min(b + CHUNK, q.shape[0])
        dx = q[b:e, None, 0] - m[None, :, 0]
        dy = q[b:e, None, 1] - m[None, :, 1]
        dz = q[b:e, None, 2] - m[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        i = np.argmin(d, axis=1)
        idx[b:e] = i
        d2[b:e] = d[np.arange(e - b), i]
    return idx, d2


def gate(idx, d2, max_dist):
    """rule 2 -> (idx, d2) with (-1, +inf) where the pair is not kept"""
    D = np.float64(max_dist) * np.float64(max_dist)
    keep = d2 <= D
    return np.where(keep, idx, -1).astype(np.int32), np.where(keep, d2, np.inf)


def summary(idx, d2):
    """rule 3 -> (K, fitness, rmse, max d2)"""
    keep = idx >= 0
    K = int(keep.sum())
    n = idx.shape[0]
    if K == 0:
        return 0, 0.0 / n, 0.0, 0.0
    return K, K / n, math.sqrt(math.fsum(d2[keep]) / K), float(d2[keep].max())


TERMS = ("x", "y", "z", "xx", "yy", "zz", "xy", "xz", "yz")


def term_columns(y):
    x, yy, z = y[:, 0], y[:, 1], y[:, 2]
    return dict(x=x, y=yy, z=z, xx=x * x, yy=yy * yy, zz=z * z, xy=x * yy, xz=x * z, yz=yy * z)


def information(m, idx):
    """rule 4 from the nine sums -> (A (6, 6), B (6, 6): per entry the sum of the |terms| it is made of)"""
    keep = idx >= 0
    K = int(keep.sum())
    cols = term_columns(m[idx[keep]])
    S = {k: math.fsum(v) for k, v in cols.items()}
    T = {k: math.fsum(np.abs(v)) for k, v in cols.items()}
    A, B = np.zeros((6, 6)), np.zeros((6, 6))

    def put(r, c, v, b):
        A[r, c] = A[c, r] = v
        B[r, c] = B[c, r] = b

    put(0, 0, S["yy"] + S["zz"], T["yy"] + T["zz"])
    put(1, 1, S["xx"] + S["zz"], T["xx"] + T["zz"])
    put(2, 2, S["xx"] + S["yy"], T["xx"] + T["yy"])
    put(0, 1, -S["xy"], T["xy"])
    put(0, 2, -S["xz"], T["xz"])
    put(1, 2, -S["yz"], T["yz"])
    put(0, 4, -S["z"], T["z"])
    put(0, 5, S["y"], T["y"])
    put(1, 3, S["z"], T["z"])
    put(1, 5, -S["x"], T["x"])
    put(2, 3, -S["y"], T["y"])
    put(2, 4, S["x"], T["x"])
    for d in (3, 4, 5):
        put(d, d, float(K), float(K))
    return A, B


def information_pairwise(m, idx):
    """the same matrix as the sum of G^T G pair by pair (Open3D's loop), each entry by math.fsum"""
    y = m[idx[idx >= 0]]
    K = y.shape[0]
    G_ = np.zeros((K, 3, 6))
    G_[:, 0, 1], G_[:, 0, 2], G_[:, 0, 3] = y[:, 2], -y[:, 1], 1.0
    G_[:, 1, 0], G_[:, 1, 2], G_[:, 1, 4] = -y[:, 2], y[:, 0], 1.0
    G_[:, 2, 0], G_[:, 2, 1], G_[:, 2, 5] = y[:, 1], -y[:, 0], 1.0
    A = np.zeros((6, 6))
    for r in range(6):
        for c in range(6):
            A[r, c] = math.fsum((G_[:, :, r] * G_[:, :, c]).reshape(-1))
    return A


def evaluate(m, p, max_dist, both=False, raw=None):
    """The whole call -> a dict with icp_evaluation's fields, idx / d2 (and model_idx / model_d2), and
    information_bound (the per-entry sum of |terms|).  raw: a cached (nearest(p, m), nearest(m, p))."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    fwd = raw[0] if raw else nearest(p, m)
    idx, d2 = gate(fwd[0], fwd[1], max_dist)
    K, fit, rmse, mx = summary(idx, d2)
    A, B = information(m, idx)
    out = dict(scene_points=p.shape[0], correspondences=K, fitness=fit, inlier_rmse=rmse, max_inlier_d2=mx,
               information=A, information_bound=B, idx=idx, d2=d2, model_points=0, model_correspondences=0,
               model_fitness=0.0, model_rmse=0.0, model_max_inlier_d2=0.0)
    if both:
        rev = raw[1] if raw else nearest(m, p)
        midx, md2 = gate(rev[0], rev[1], max_dist)
        Km, mfit, mrmse, mmx = summary(midx, md2)
        out.update(model_points=m.shape[0], model_correspondences=Km, model_fitness=mfit, model_rmse=mrmse,
                   model_max_inlier_d2=mmx, model_idx=midx, model_d2=md2)
    return out


# ---- inputs ---------------------------------------------------------------------------------

SYNTH_SIZES = (5, 63, 64, 65, 257, 1025, 4097, 9001)
SYNTH_DISTS = (0.08, 0.12)
# name -> ((max_dist, K, K_m | None), ...): the issue's table, checked on the CPU by tests/test_eval_ref.py
COUNTS = {
    "synth5": ((0.08, 1, 1), (0.12, 3, 3)),
    "synth63": ((0.08, 14, 14), (0.12, 34, 34)),
    "synth64": ((0.08, 13, 14), (0.12, 33, 34)),
    "synth65": ((0.08, 18, 18), (0.12, 36, 36)),
    "synth257": ((0.08, 50, 53), (0.12, 126, 136)),
    "synth1025": ((0.08, 339, 362), (0.12, 629, 729)),
    "synth4097": ((0.08, 2229, 2557), (0.12, 2959, 3881)),
    "synth9001": ((0.08, 5994, 7530), (0.12, 6649, 8900)),
    "cow_partial": (("0.05ext", 712, 755), ("0.2ext", 1777, 1839), (float("inf"), 2177, 2177)),
    "far": ((0.05, 3718, 3627), (0.2, 4089, 4089)),
    "shell": ((0.3, 155, 243),),
    "lattice_tie": ((1.0, 729, None),),
    "lattice_edge": ((0.5, 729, None), (0.49, 0, None)),
}
CASES = tuple(COUNTS)

_clouds, _raw = {}, {}


def clouds(name, load=None):
    """-> (model, scene) of a named case; load: the oracle's load_matrix, for the cow"""
    if name in _clouds:
        return _clouds[name]
    if name.startswith("synth"):
        n = int(name[5:])
        m, p = G.synth(n, 100 + n, 0.25, sigma=0.05)
    elif name == "cow_partial":
        m, p = G.cow_partial(load(datasets.path("cow_ref")), load(datasets.path("cow_tr2")))
    elif name == "far":
        m = NR.far_points()
        p = m @ P.rot((1, 2, 3), 5).T + np.array([0.02, -0.03, 0.01])
    elif name == "shell":
        m = P.ellipsoid(257, 357)[0]
        p = np.concatenate([3 * m, 0.5 * m, m[:40]])
    elif name == "lattice_tie":
        m = NR.lattice()
        p = m + np.array([0.5, 0.5, 0.5])
    elif name == "lattice_edge":
        m = NR.lattice()
        p = m + np.array([0.5, 0.0, 0.0])
    else:
        raise KeyError(name)
    _clouds[name] = (np.ascontiguousarray(m, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64))
    return _clouds[name]


def distance(name, d, load=None):
    """a table entry's max_dist as a number ("0.05ext": that share of the cow's extent)"""
    if isinstance(d, str):
        return float(d[:-3]) * G.cow_ext(load(datasets.path("cow_ref")))
    return d


def reference(name, d, load=None):
    """-> (m, p, max_dist, evaluate(m, p, max_dist, both)): the brute force once a case and session,
    shared and never modified"""
    m, p = clouds(name, load)
    if name not in _raw:
        _raw[name] = (nearest(p, m), nearest(m, p))
    md = distance(name, d, load)
    return m, p, md, evaluate(m, p, md, both=True, raw=_raw[name])
