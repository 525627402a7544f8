"""The reference of the gated ICP loop (icp_set_max_distance), from the oracle's own pieces, and
the inputs of the gated tests (tests/test_gated_ref.py on the CPU, tests/test_gpu_gated.py).

One gated iteration on the current scene p (all n points), D = dmax * dmax in fp64:
  Y = closest(p, m);  d2_j = (dx*dx + dy*dy) + dz*dz, dx = p_j.x - Y_j.x ...;  keep_j = d2_j <= D
  K = #keep; K < 4: stop before the iteration changes anything ("few")
  Horn's closed form over the kept pairs (N = K); EVERY point moves: p_j <- sR p_j + t
  e = sum over the kept j of ||Y_j - p_j(new)||^2;  err = (align.err + e) / K
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import datasets


def d2_of(p, Y):
    """(dx*dx + dy*dy) + dz*dz in fp64, the engine's NN arithmetic (numpy does not contract)."""
    dx = p[:, 0] - Y[:, 0]
    dy = p[:, 1] - Y[:, 1]
    dz = p[:, 2] - Y[:, 2]
    return (dx * dx + dy * dy) + dz * dz


def gated_ref(oracle, m, p, dmax, max_iter, threshold=1e-5):
    """-> dict(new_p, K (list), err (array), mask (last gate evaluated), status ('ok' | 'few'),
    margin (min over iterations and points of |d2 - D| / D; inf without a finite gate),
    s, R, t (the last completed iteration's), iterations)."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64).copy()
    D = np.float64(dmax) * np.float64(dmax)
    Ks, errs = [], []
    mask = np.zeros(p.shape[0], dtype=bool)
    margin = np.inf
    status = "ok"
    s, R, t = 1.0, np.eye(3), np.zeros(3)
    for _ in range(max_iter):
        Y, _idx = oracle.closest(p, m)
        d2 = d2_of(p, Y)
        with np.errstate(invalid="ignore"):
            keep = d2 <= D
        mask = keep
        if np.isfinite(D):
            margin = min(margin, float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        if K < 4:
            status = "few"
            Ks_fail = K
            return dict(new_p=p, K=Ks, err=np.array(errs), mask=mask, status=status, margin=margin, s=s, R=R, t=t,
                        iterations=len(errs), K_fail=Ks_fail)
        al = oracle.find_alignment(p[keep], Y[keep])
        s, R, t = al.s, np.array(al.R).reshape(3, 3), np.array(al.t)
        e, kept_new = oracle.err_compute(p[keep], Y[keep], al.s, al.R, al.t)
        new_p = np.empty_like(p)
        new_p[keep] = kept_new
        if K < p.shape[0]:
            _e, rest_new = oracle.err_compute(p[~keep], Y[~keep], al.s, al.R, al.t)
            new_p[~keep] = rest_new
        p = new_p
        err = (al.err + e) / K
        Ks.append(K)
        errs.append(err)
        if err < threshold:
            break
    return dict(new_p=p, K=Ks, err=np.array(errs), mask=mask, status=status, margin=margin, s=s, R=R, t=t,
                iterations=len(errs))


# ---- inputs ---------------------------------------------------------------------------------

def synth(n, seed, frac_out, sigma=0.01):
    r = np.random.default_rng(seed); m = r.uniform(-1, 1, size=(n, 3))
    ax = np.array([1., 2., 3.]); ax /= np.linalg.norm(ax); a = np.deg2rad(5.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    p = m @ R.T + np.array([0.02, -0.03, 0.01]) + sigma * r.standard_normal((n, 3))
    k = int(round(frac_out * n))
    if k: p[r.choice(n, k, replace=False)] = np.array([4., 0, 0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    return m, p


def cow_ext(cow_ref):
    return float(np.abs(cow_ref).max())  # 2.81976


def cow_clump(cow_ref, cow_tr2):
    ext = cow_ext(cow_ref)
    r = np.random.default_rng(7); sc = cow_tr2.copy()
    sc[-700:] = cow_ref.mean(0) + np.array([3 * ext, 0, 0]) + r.uniform(-0.05 * ext, 0.05 * ext, size=(700, 3))
    return sc


def cow_partial(cow_ref, cow_tr2):
    """Partial overlap: model = the cow_ref points with x above its 0.25 quantile, scene = the
    cow_tr2 points whose cow_ref x is below the 0.75 quantile (2177 x 2177)."""
    x = cow_ref[:, 0]
    return cow_ref[x > np.quantile(x, 0.25)], cow_tr2[x < np.quantile(x, 0.75)]


def load_cow(oracle):
    return (oracle.load_matrix(datasets.path("cow_ref")), oracle.load_matrix(datasets.path("cow_tr1")),
            oracle.load_matrix(datasets.path("cow_tr2")))


# The cases of tests/test_gpu_gated.py with the reference K the issue quotes; each is checked on
# the CPU by tests/test_gated_ref.py (margin > 1e-6, the K list) before the GPU tests rely on it.
SIZES = {5: 4, 63: 47, 64: 48, 65: 49, 257: 193, 4096: 3072, 4097: 3073, 9001: 6751}  # n -> K, every iteration
SIZES_DMAX, SIZES_ITERS = 1.0, 6
BITES = {(257, 0.08): (50, 109), (257, 0.12): (126, 175), (4097, 0.08): (2229, 2481), (4097, 0.12): (2959, 3047)}
BITES_ITERS = 8  # (n, dmax) -> (K first, K last); synth(n, 100 + n, 0.25, sigma=0.05)

_cache = {}


def reference(oracle, key):
    """The reference of a named case, computed once a session and shared (never modified).
    key: ("size", n) | ("bite", n, dmax) | ("partial",) | ("clump",) | ("clump", iters) -> (m, p, dmax, ref)"""
    if key in _cache:
        return _cache[key]
    if key[0] == "size":
        m, p = synth(key[1], 100 + key[1], 0.25)
        out = (m, p, SIZES_DMAX, gated_ref(oracle, m, p, SIZES_DMAX, SIZES_ITERS, -1.0))
    elif key[0] == "bite":
        m, p = synth(key[1], 100 + key[1], 0.25, sigma=0.05)
        out = (m, p, key[2], gated_ref(oracle, m, p, key[2], BITES_ITERS, -1.0))
    elif key[0] == "partial":
        ref_, _tr1, tr2 = load_cow(oracle)
        m, p = cow_partial(ref_, tr2)
        dmax = 0.05 * cow_ext(ref_)
        out = (m, p, dmax, gated_ref(oracle, m, p, dmax, 20, -1.0))
    elif key[0] == "clump":
        ref_, _tr1, tr2 = load_cow(oracle)
        p = cow_clump(ref_, tr2)
        dmax = 0.25 * cow_ext(ref_)
        if len(key) == 1:
            out = (ref_, p, dmax, gated_ref(oracle, ref_, p, dmax, 30, 1e-5))
        else:
            out = (ref_, p, dmax, gated_ref(oracle, ref_, p, dmax, key[1], -1.0))
    else:
        raise KeyError(key)
    _cache[key] = out
    return out
