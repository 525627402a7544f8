"""The reference of the two outlier filters (icp_filter_statistical, icp_filter_radius; icp_filter.hip),
restated in numpy from include/icp_capi.h, and the inputs of their tests (tests/test_filter_ref.py on
the CPU, tests/test_gpu_filter.py).

Statistical, for point j:
  1. L_j = normals_ref.knn(m, k + 1): the first k + 1 indices in ascending (d2, i) order, the point
     itself a candidate
  2. dbar_j = (sum of sqrt(d2) over the list, column by column from +0) / k
  3. mu = fsum(dbar) / n, sigma = sqrt(fsum((dbar - mu)^2) / (n - 1)): math.fsum is the correctly rounded
     sum, so the reference takes no side on the engine's order; the GPU test allows n 2^-53 for it
  4. T = mu + ratio * sigma; keep j iff dbar_j <= T
Radius: c_j = #{ i : (dx*dx + dy*dy) + dz*dz <= radius * radius } by chunked brute force (the point
itself counted); keep j iff c_j > min_neighbors.
A helper module, not a conftest: no fixtures, no hooks.
"""
import math

import numpy as np

import normals_ref as NR
import plane_ref as P

MARGIN = 1e-9  # the least |dbar_j - T| / T of a statistical case (tests/test_filter_ref.py)


def statistical(m, k, ratio):
    """-> dict(mean (n,), mu, sigma, T, mask (n,) bool, margin: min |dbar - T| / T)"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    n = m.shape[0]
    _idx, d2, _tie = NR.knn(m, k + 1)
    s = np.zeros(n)
    for e in range(k + 1):
        s = s + np.sqrt(d2[:, e])
    mean = s / float(k)
    mu = math.fsum(mean) / n
    dev = mean - mu
    sigma = math.sqrt(math.fsum(dev * dev) / (n - 1))
    return dict(mean=mean, mu=mu, sigma=sigma, **threshold(mean, mu, sigma, ratio))


def threshold(mean, mu, sigma, ratio):
    """rule 4 -> dict(T, mask, margin)"""
    T = mu + ratio * sigma
    margin = float(np.min(np.abs(mean - T)) / T) if T > 0 else 0.0
    return dict(T=T, mask=mean <= T, margin=margin)


def radius_counts(m, radius, chunk=512):
    """-> c (n,) int32"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    r2 = float(radius) * float(radius)
    c = np.empty(m.shape[0], dtype=np.int32)
    for b in range(0, m.shape[0], chunk):
        q = m[b:b + chunk]
        dx = q[:, None, 0] - m[None, :, 0]
        dy = q[:, None, 1] - m[None, :, 1]
        dz = q[:, None, 2] - m[None, :, 2]
        c[b:b + chunk] = ((dx * dx + dy * dy) + dz * dz <= r2).sum(axis=1)
    return c


# ---- inputs ---------------------------------------------------------------------------------

K = 16
ELLIPSOIDS = (K + 1, 64, 65, 257, 4097, 9001)  # normals_ref's ellipsoids ("ell<n>")
CLUTTER_SEED = 20


def duplicates():
    """an ellipsoid and one of its points 19 more times: 20 >= k + 2 equal points, whose dbar is 0"""
    m = P.ellipsoid(257, 357)[0]
    return np.concatenate([m[:100], np.tile(m[5], (19, 1)), m[100:]])


def cow_clutter(load, name="cow_ref"):
    """cow_ref (or another bundled cloud) plus n / 50 points uniform in its box scaled by 1.5 about the
    centre, rows shuffled -> (cloud, planted (bool, per row))"""
    import datasets
    cow = np.ascontiguousarray(load(datasets.path(name)), dtype=np.float64)
    rng = np.random.default_rng(CLUTTER_SEED)
    lo, hi = cow.min(axis=0), cow.max(axis=0)
    c, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    extra = c + half * rng.uniform(-1.0, 1.0, (cow.shape[0] // 50, 3))
    cloud = np.concatenate([cow, extra])
    planted = np.concatenate([np.zeros(cow.shape[0], dtype=bool), np.ones(extra.shape[0], dtype=bool)])
    perm = rng.permutation(cloud.shape[0])
    return np.ascontiguousarray(cloud[perm]), planted[perm]


def cloud(name, load=None):
    """The named input; "cow_clutter" needs load (a cloud's loader)."""
    if name.startswith("ell"):
        return NR.model(name)[0]
    if name == "cow_clutter":
        return cow_clutter(load)[0]
    return {"lattice": NR.lattice, "far": NR.far_points, "duplicates": duplicates}[name]()


CASES = tuple("ell%d" % n for n in ELLIPSOIDS) + ("lattice", "duplicates", "far", "cow_clutter")
# (k, ratio) of every statistical case the GPU test runs
STAT_PARAMS = {name: ((K, 2.0), (K, 1.0)) for name in CASES}
STAT_PARAMS["ell257"] = ((K, 2.0), (K, 1.0), (2, 2.0), (63, 0.5), (8, 0.0), (K, 1e6))
STAT_PARAMS["ell17"] = ((K, 2.0), (K, 1.0), (K, 0.0))


def radius_params(name, m):
    """(radius, min_neighbors) of every radius case the GPU test runs.  The lattice at exactly 1.0: the six
    neighbours at d2 == r2 count.  ell257 at its diameter: every count is n."""
    if name == "lattice":
        return ((1.0, 5), (1.0, 6), (1.5, 18))
    spread = float(np.linalg.norm(m.max(axis=0) - m.min(axis=0)))
    out = ((0.05 * spread, 2), (0.15 * spread, 8))
    if name == "ell257":
        out += ((spread, 256), (spread, 257))
    if name == "far":
        out += ((40.0, 8),)  # the cluster at x = 40 comes within reach: the boxes go over the cell budget
    return out


_cache = {}


def reference(kind, name, params, load=None):
    """The reference of a named input, computed once a session and shared (never modified):
    kind "stat", params (k, ratio) -> (m, statistical(...)); kind "radius", params radius -> (m, counts)"""
    if ("cloud", name) not in _cache:
        _cache[("cloud", name)] = cloud(name, load)
    m = _cache[("cloud", name)]
    key = (kind, name, params)
    if key not in _cache:
        if kind == "stat":
            # (the lists are the costly half: shared by the ratios of one k)
            lk = ("lists", name, params[0])
            if lk not in _cache:
                _cache[lk] = statistical(m, params[0], 0.0)
            base = _cache[lk]
            _cache[key] = dict(base, **threshold(base["mean"], base["mu"], base["sigma"], params[1]))
        else:
            _cache[key] = radius_counts(m, params)
    return m, _cache[key]
