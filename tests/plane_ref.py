"""The reference of the point-to-plane ICP loop (icp_set_metric, icp_plane.hip), restated with the
oracle's nearest-neighbour search and numpy, and the inputs of its tests (tests/test_plane_ref.py
on the CPU, tests/test_gpu_plane.py).

One iteration on the current scene p (all n points); N = the model's normals as given, c = the
model's centroid, D = dmax * dmax (+inf without a gate):
  1. Y, idx = closest(p, m);  n_j = N[idx_j]
  2. d = p - Y;  d2_j = (dx*dx + dy*dy) + dz*dz;  keep_j = d2_j <= D;  K = #keep
  3. K < 6: stop before the iteration changes anything ("few")
  4. over the kept pairs a_j = [(p_j - c) x n_j ; n_j], r_j = d_j . n_j:  A = sum a_j a_j^T, b = -sum a_j r_j
  5. g = sqrt(diag A) (an A_kk not > 0: "degenerate");  A^ = A / (g g^T), b^ = b / g;  Cholesky of A^
     (a pivot not > 1e-12: "degenerate");  x = solve(A^, b^) / g
  6. omega = x[:3], tau = x[3:];  R = exp([omega]x) (Rodrigues), s = 1, t = (c + tau) - R c
  7. every point moves, q = R p + t;  e = sum over the kept j of ((q_j - Y_j) . n_j)^2;  err = (e + e) / K
dtype = np.float64 restates the engine's arithmetic; dtype = np.longdouble is the extended-precision
truth (the searches stay the oracle's fp64 ones; the solve is plain elimination).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

from gated_ref import d2_of

PIVOT_MIN = 1e-12
AXES = np.array([1.0, 0.7, 0.45])


def rot(axis, deg):
    """The rotation of gated_ref.synth: Rodrigues about `axis` by `deg` degrees."""
    ax = np.array(axis, dtype=np.float64)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _solve(A, b, dtype):
    """-> (x | None, smallest pivot).  fp64: Cholesky by rows, as the kernel; longdouble: elimination."""
    diag = np.diag(A)
    if not np.all(diag > 0):
        return None, dtype(0)
    g = np.sqrt(diag)
    Ah = A / np.outer(g, g)
    bh = b / g
    pmin = dtype(np.inf)
    if dtype is np.float64:
        L = np.zeros((6, 6))
        for r in range(6):
            for c in range(r):
                L[r, c] = (Ah[r, c] - np.dot(L[r, :c], L[c, :c])) / L[c, c]
            d = Ah[r, r] - np.dot(L[r, :r], L[r, :r])
            pmin = min(pmin, d) if d == d else d
            if not d > PIVOT_MIN:
                return None, pmin
            L[r, r] = np.sqrt(d)
        z = np.zeros(6)
        for r in range(6):
            z[r] = (bh[r] - np.dot(L[r, :r], z[:r])) / L[r, r]
        x = np.zeros(6)
        for r in range(5, -1, -1):
            x[r] = (z[r] - np.dot(L[r + 1:, r], x[r + 1:])) / L[r, r]
        return x / g, pmin
    M = np.concatenate([Ah, bh[:, None]], axis=1).astype(dtype)
    for r in range(6):
        d = M[r, r]
        pmin = min(pmin, d) if d == d else d
        if not d > PIVOT_MIN:
            return None, pmin
        for k in range(r + 1, 6):
            M[k] = M[k] - (M[k, r] / d) * M[r]
    x = np.zeros(6, dtype=dtype)
    for r in range(5, -1, -1):
        x[r] = (M[r, 6] - np.dot(M[r, r + 1:6], x[r + 1:])) / M[r, r]
    return x / g, pmin


def _rodrigues(w, dtype):
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if not th2 > 0:
        return np.eye(3, dtype=dtype)
    th = np.sqrt(th2)
    sa = np.sin(th) / th
    h = np.sin(th / 2) / th
    sb = 2 * (h * h)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=dtype)
    return np.eye(3, dtype=dtype) + sa * W + sb * (W @ W)


def plane_ref(oracle, m, N, p, dmax, max_iter, threshold=1e-5, dtype=np.float64):
    """-> dict(new_p, err (array), K (list), mask (last gate evaluated), s, R, t (the last completed
    iteration's), iterations, status ('ok' | 'few' | 'degenerate'), fail_iter, K_fail, min_pivot (the
    smallest pivot of any solve), margin (min over iterations and points of |d2 - D| / D; inf
    without a finite gate))."""
    m64 = np.ascontiguousarray(m, dtype=np.float64)
    mx = m64.astype(dtype)
    Nx = np.ascontiguousarray(N, dtype=np.float64).astype(dtype)
    p = np.ascontiguousarray(p, dtype=np.float64).astype(dtype)
    c = mx.sum(axis=0) / dtype(mx.shape[0])
    D = np.float64(dmax) * np.float64(dmax) if dmax is not None and dmax > 0 and np.isfinite(dmax) else np.inf
    Ks, errs = [], []
    out = dict(status="ok", margin=np.inf, min_pivot=np.inf, s=1.0, R=np.eye(3, dtype=dtype), t=np.zeros(3, dtype=dtype),
               mask=np.zeros(p.shape[0], dtype=bool), fail_iter=-1, K_fail=-1)
    for it in range(max_iter):
        p64 = np.ascontiguousarray(p, dtype=np.float64)
        _Y, idx = oracle.closest(p64, m64)
        Y, n = mx[idx], Nx[idx]
        d2 = d2_of(p, Y)
        with np.errstate(invalid="ignore"):
            keep = d2 <= D
        out["mask"] = np.asarray(keep, dtype=bool)
        if np.isfinite(D):
            out["margin"] = min(out["margin"], float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        if K < 6:
            out.update(status="few", fail_iter=it, K_fail=K)
            break
        pk, Yk, nk = p[keep], Y[keep], n[keep]
        a = np.concatenate([np.cross(pk - c, nk), nk], axis=1)
        d = pk - Yk
        r = (d[:, 0] * nk[:, 0] + d[:, 1] * nk[:, 1]) + d[:, 2] * nk[:, 2]
        A = a.T @ a
        b = -(a * r[:, None]).sum(axis=0)
        x, piv = _solve(A, b, dtype)
        out["min_pivot"] = min(out["min_pivot"], float(piv))
        if x is None:
            out.update(status="degenerate", fail_iter=it, K_fail=K, min_pivot=float(piv))
            break
        R = _rodrigues(x[:3], dtype)
        t = (c + x[3:]) - R @ c
        p = p @ R.T + t
        q = p[keep] - Yk
        rn = (q[:, 0] * nk[:, 0] + q[:, 1] * nk[:, 1]) + q[:, 2] * nk[:, 2]
        e = (rn * rn).sum()
        err = (e + e) / dtype(K)
        out.update(R=R, t=t)
        Ks.append(K)
        errs.append(err)
        if err < threshold:
            break
    out.update(new_p=p, K=Ks, err=np.array(errs, dtype=dtype), iterations=len(errs))
    return out


# ---- inputs ---------------------------------------------------------------------------------

def ellipsoid(n, seed):
    """n points of the tri-axial ellipsoid with semi-axes (1, 0.7, 0.45) and their unit normals."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    m = v * AXES
    nrm = m / (AXES * AXES)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return m, nrm


def synth(n, seed, sigma, other=False):
    """-> (model, normals, scene, src): the scene is src (the model, or with `other` a different
    sample of the same surface) turned 5 degrees about (1, 2, 3), shifted, with noise sigma."""
    m, nrm = ellipsoid(n, seed)
    src = ellipsoid(n, seed + 1000)[0] if other else m
    p = src @ rot((1, 2, 3), 5.0).T + np.array([0.02, -0.03, 0.01])
    p = p + sigma * np.random.default_rng(seed + 5).standard_normal((n, 3))
    return m, nrm, p, src


def gate_case(n):
    """synth(n, 100 + n, 0.05) with a quarter of the scene moved far away, to (4, 0, 0) + U(-0.2, 0.2)."""
    m, nrm, p, _src = synth(n, 100 + n, 0.05)
    r = np.random.default_rng(n)
    k = n // 4
    p[r.choice(n, k, replace=False)] = np.array([4.0, 0.0, 0.0]) + r.uniform(-0.2, 0.2, size=(k, 3))
    return m, nrm, p


def planar(n=400, seed=3):
    """A planar model (z = 0, normals (0, 0, 1)) and a scene beside it: degenerate at iteration 0."""
    r = np.random.default_rng(seed)
    m = np.concatenate([r.uniform(-1, 1, size=(n, 2)), np.zeros((n, 1))], axis=1)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    p = m @ rot((1, 2, 3), 2.0).T + np.array([0.01, 0.02, 0.03])
    return m, nrm, p


def five():
    """A 5-point pair: too few for the 6 x 6 system."""
    m, nrm, p, _src = synth(5, 105, 0.01)
    return m, nrm, p


SIZES = (6, 7, 63, 64, 65, 257, 4096, 4097, 9001)  # synth(n, 100 + n, 0.01), no gate
SIZES_ITERS = 6
GATES = {(257, 0.08): [104, 128, 135, 130, 126, 125, 115, 115],  # (n, dmax) -> K of each iteration
         (4097, 0.08): [2543, 2670, 2707, 2709, 2712, 2711, 2713, 2713]}
GATES_ITERS = 8

_cache = {}


def reference(oracle, key, dtype=np.float64):
    """The reference of a named case, computed once a session and shared (never modified).
    key: ("size", n) | ("gate", n, dmax) -> (m, normals, p, dmax, ref)"""
    ck = (key, dtype)
    if ck in _cache:
        return _cache[ck]
    if key[0] == "size":
        m, nrm, p, _src = synth(key[1], 100 + key[1], 0.01)
        out = (m, nrm, p, 0.0, plane_ref(oracle, m, nrm, p, 0.0, SIZES_ITERS, -1.0, dtype))
    elif key[0] == "gate":
        m, nrm, p = gate_case(key[1])
        out = (m, nrm, p, key[2], plane_ref(oracle, m, nrm, p, key[2], GATES_ITERS, -1.0, dtype))
    else:
        raise KeyError(key)
    _cache[ck] = out
    return out
