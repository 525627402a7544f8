"""The reference of icp_run with robust weights (icp_set_robust), restated with the oracle's
nearest-neighbour search, its symmetric 4 x 4 eigen-solve (Horn) and numpy, on top of gated_ref.py and
plane_ref.py, and the inputs of its tests (tests/test_robust_ref.py on the CPU,
tests/test_gpu_robust.py).

One iteration on the current scene p (all n points); D = dmax * dmax (+inf without a gate), k2 = k * k
in fp64, c = the model's centroid:
  1. Y, idx = closest(p, m);  d = p - Y;  d2_j = (dx*dx + dy*dy) + dz*dz;  keep_j = d2_j <= D;  K = #keep
  2. residual of a kept pair: point-to-point r2_j = d2_j;  point-to-plane r_j = (dx*nx + dy*ny) + dz*nz,
     r2_j = r_j * r_j
  3. w_j:  Huber r2 <= k2 ? 1 : k / sqrt(r2);  Tukey r2 < k2 ? (1 - r2/k2)^2 : 0;  Cauchy 1 / (1 + r2/k2);
     a NaN residual weighs 0.  W = sum w, K+ = #{w > 0}
  4. K or K+ below the metric's least count (4 / 6): stop before the iteration changes anything ("few")
  5. point-to-point: Horn's closed form on the weighted sums -- mu_p = sum w p / W, mu_y = sum w y / W,
     S = sum w p' y'^T, d_caps = sum w |y'|^2, sp = sum w |p'|^2, the quaternion of the largest
     eigenvalue (the oracle's eig_sym4 and max_element_index), s = sqrt(d_caps / sp), t = mu_y - s R mu_p;
     point-to-plane: (sum w a a^T) x = -sum w a r with plane_ref's solve, Rodrigues, t = (c + tau) - R c
  6. every point moves;  e = the kept pairs' UNWEIGHTED residual after the move;  err = (e + e) / K
With ROBUST_NONE the point-to-point iteration is gated_ref's own (the oracle's find_alignment and
err_compute) and the point-to-plane one is the weighted code with w = 1, which multiplies exactly: both
equal gated_ref / plane_ref bit for bit.
dtype = np.float64 restates the engine's arithmetic; dtype = np.longdouble is the extended-precision
truth (the searches stay the oracle's fp64 ones, k2 stays the fp64 product, the eigenvector of the
fp64 solve is refined by Rayleigh-quotient iteration in longdouble).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import gated_ref as G
import plane_ref as P
from gated_ref import d2_of

NONE, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3
KINDS = {"huber": HUBER, "tukey": TUKEY, "cauchy": CAUCHY}


def weights(kind, r2, k, dtype=np.float64):
    """-> w (dtype) of the squared residuals r2; k2 = k * k is the fp64 product, as on the host."""
    k2 = dtype(np.float64(k) * np.float64(k))
    kk = dtype(np.float64(k))
    r2 = np.asarray(r2, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == NONE:
            return np.ones(r2.shape, dtype=dtype)
        if kind == HUBER:
            w = np.where(r2 <= k2, dtype(1), np.where(r2 > k2, kk / np.sqrt(r2), dtype(0)))
        elif kind == TUKEY:
            u = dtype(1) - r2 / k2
            w = np.where(r2 < k2, u * u, dtype(0))
        elif kind == CAUCHY:
            w = np.where(r2 == r2, dtype(1) / (dtype(1) + r2 / k2), dtype(0))
        else:
            raise ValueError(kind)
    return np.asarray(w, dtype=dtype)


def _solve4(M, b, dtype):
    """Gaussian elimination with partial pivoting, 4 x 4 (numpy has no longdouble solver)."""
    A = np.concatenate([M, b[:, None]], axis=1).astype(dtype)
    for r in range(4):
        piv = r + int(np.argmax(np.abs(A[r:, r])))
        if A[piv, r] == 0:
            return None
        A[[r, piv]] = A[[piv, r]]
        for i in range(r + 1, 4):
            A[i] = A[i] - (A[i, r] / A[r, r]) * A[r]
    x = np.zeros(4, dtype=dtype)
    for r in range(3, -1, -1):
        x[r] = (A[r, 4] - np.dot(A[r, r + 1:4], x[r + 1:])) / A[r, r]
    return x


def _top_quaternion(oracle, Nm, dtype):
    """The unit eigenvector of Nm's largest eigenvalue: the oracle's Jacobi solve in fp64, refined by
    Rayleigh-quotient iteration in `dtype` when that is wider."""
    N64 = np.asarray(Nm, dtype=np.float64)
    ev, V = oracle.eig_sym4(N64)
    q = V[:, oracle.max_element_index(ev)].astype(dtype)
    if dtype is np.float64:
        return q
    for _ in range(3):
        lam = q @ (Nm @ q) / (q @ q)
        x = _solve4(Nm - lam * np.eye(4, dtype=dtype), q, dtype)
        if x is None or not np.all(np.isfinite(x)):
            break
        q = x / np.sqrt(x @ x)
    return q


def weighted_horn(oracle, pk, Yk, w, dtype):
    """Horn's closed form on the weighted sums with N = W -> (s, R, t), as oracle_find_alignment
    builds them (cpu.cc:113-167)."""
    W = w.sum()
    mu_p = (w[:, None] * pk).sum(axis=0) / W
    mu_y = (w[:, None] * Yk).sum(axis=0) / W
    pp, yp = pk - mu_p, Yk - mu_y
    S = (w[:, None] * pp).T @ yp
    d_caps = (w * ((yp[:, 0] * yp[:, 0] + yp[:, 1] * yp[:, 1]) + yp[:, 2] * yp[:, 2])).sum()
    sp = (w * ((pp[:, 0] * pp[:, 0] + pp[:, 1] * pp[:, 1]) + pp[:, 2] * pp[:, 2])).sum()
    s = S
    Nm = np.array([
        [s[0, 0] + s[1, 1] + s[2, 2], s[1, 2] - s[2, 1], -s[0, 2] + s[2, 0], s[0, 1] - s[1, 0]],
        [-s[2, 1] + s[1, 2], s[0, 0] - s[2, 2] - s[1, 1], s[0, 1] + s[1, 0], s[0, 2] + s[2, 0]],
        [s[2, 0] - s[0, 2], s[1, 0] + s[0, 1], s[1, 1] - s[2, 2] - s[0, 0], s[1, 2] + s[2, 1]],
        [-s[1, 0] + s[0, 1], s[2, 0] + s[0, 2], s[2, 1] + s[1, 2], s[2, 2] - s[1, 1] - s[0, 0]],
    ], dtype=dtype)
    q0, q1, q2, q3 = _top_quaternion(oracle, Nm, dtype)
    qbar = np.array([[q0, -q1, -q2, -q3], [q1, q0, q3, -q2], [q2, -q3, q0, q1], [q3, q2, -q1, q0]], dtype=dtype)
    qcap = np.array([[q0, -q1, -q2, -q3], [q1, q0, -q3, q2], [q2, q3, q0, -q1], [q3, -q2, q1, q0]], dtype=dtype)
    R = (qbar.T @ qcap)[1:, 1:]
    sc = np.sqrt(d_caps / sp)
    t = mu_y - (sc * R) @ mu_p
    return sc, R, t


def robust_ref(oracle, metric, m, N, p, dmax, kind, k, max_iter, threshold=1e-5, dtype=np.float64):
    """metric: "point" | "plane" (N: the model's normals, unused for "point").
    -> dict(new_p, err (array), K, W, Kpos (lists, one entry a recorded iteration), mask (last gate
    evaluated), s, R, t (the last completed iteration's), iterations, status ('ok' | 'few' |
    'degenerate'), fail_iter, K_fail, Kpos_fail, margin (min |d2 - D| / D; inf without a finite gate),
    kmargin (min over iterations and kept pairs of |r2 - k2| / k2; inf with ROBUST_NONE))."""
    plane = metric == "plane"
    least = 6 if plane else 4
    if kind == NONE and not plane and dtype is np.float64:  # gated_ref's own iteration (the oracle's Horn)
        g = G.gated_ref(oracle, m, p, dmax if dmax and np.isfinite(dmax) else np.inf, max_iter, threshold)
        out = dict(g, W=[float(x) for x in g["K"]], Kpos=list(g["K"]), kmargin=np.inf, fail_iter=-1, Kpos_fail=-1)
        if g["status"] == "few":
            out.update(fail_iter=g["iterations"], Kpos_fail=g["K_fail"])
        return out
    m64 = np.ascontiguousarray(m, dtype=np.float64)
    mx = m64.astype(dtype)
    Nx = np.ascontiguousarray(N, dtype=np.float64).astype(dtype) if plane else None
    p = np.ascontiguousarray(p, dtype=np.float64).astype(dtype)
    c = mx.sum(axis=0) / dtype(mx.shape[0])
    D = np.float64(dmax) * np.float64(dmax) if dmax is not None and dmax > 0 and np.isfinite(dmax) else np.inf
    k2 = np.float64(k) * np.float64(k)
    Ks, Ws, Kps, errs = [], [], [], []
    out = dict(status="ok", margin=np.inf, kmargin=np.inf, s=1.0, R=np.eye(3, dtype=dtype), t=np.zeros(3, dtype=dtype),
               mask=np.zeros(p.shape[0], dtype=bool), fail_iter=-1, K_fail=-1, Kpos_fail=-1)
    for it in range(max_iter):
        p64 = np.ascontiguousarray(p, dtype=np.float64)
        _Y, idx = oracle.closest(p64, m64)
        Y = mx[idx]
        d2 = d2_of(p, Y)
        with np.errstate(invalid="ignore"):
            keep = d2 <= D
        out["mask"] = np.asarray(keep, dtype=bool)
        if np.isfinite(D):
            out["margin"] = min(out["margin"], float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        pk, Yk = p[keep], Y[keep]
        d = pk - Yk
        if plane:
            nk = Nx[idx][keep]
            r = (d[:, 0] * nk[:, 0] + d[:, 1] * nk[:, 1]) + d[:, 2] * nk[:, 2]
            r2 = r * r
        else:
            r2 = d2[keep]
        w = weights(kind, r2, k, dtype)
        Kpos = int((w > 0).sum())
        W = w.sum() if K else dtype(0)
        if kind != NONE and K:
            out["kmargin"] = min(out["kmargin"], float(np.min(np.abs(r2 - dtype(k2)) / dtype(k2))))
        if K < least or Kpos < least:
            out.update(status="few", fail_iter=it, K_fail=K, Kpos_fail=Kpos)
            break
        if plane:
            a = np.concatenate([np.cross(pk - c, nk), nk], axis=1)
            A = (a * w[:, None]).T @ a
            b = -(a * (w * r)[:, None]).sum(axis=0)
            x, piv = P._solve(A, b, dtype)
            if x is None:
                out.update(status="degenerate", fail_iter=it, K_fail=K, Kpos_fail=Kpos, min_pivot=float(piv))
                break
            s, R = dtype(1), P._rodrigues(x[:3], dtype)
            t = (c + x[3:]) - R @ c
        else:
            s, R, t = weighted_horn(oracle, pk, Yk, w, dtype)
        p = p @ (s * R).T + t
        q = p[keep] - Yk
        if plane:
            rn = (q[:, 0] * nk[:, 0] + q[:, 1] * nk[:, 1]) + q[:, 2] * nk[:, 2]
            e = (rn * rn).sum()
        else:
            e = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]).sum()
        err = (e + e) / dtype(K)
        out.update(s=s, R=R, t=t)
        Ks.append(K)
        Ws.append(W)
        Kps.append(Kpos)
        errs.append(err)
        if err < threshold:
            break
    out.update(new_p=p, K=Ks, W=Ws, Kpos=Kps, err=np.array(errs, dtype=dtype), iterations=len(errs))
    return out


# ---- inputs ---------------------------------------------------------------------------------

SIZES = (6, 7, 63, 64, 65, 257, 4097)  # plane_ref.synth(n, 100 + n, 0.01): both metrics, no gate
SIZES_ITERS = 6
METRICS = ("point", "plane")


def k_of(metric, kind, n):
    """The scale of a sizes case.  The residuals start near 0.05 (point-to-point: the 5 degree turn and
    the shift) or 0.03 (along the normal) and end at the noise, 0.01 a coordinate: these k put pairs
    on both sides of Huber's and Tukey's k while leaving every iteration at least the metric's least
    count of positive weights, down to n = 6 (tests/test_robust_ref.py checks that, and kmargin)."""
    if metric == "point":
        return {HUBER: 0.03, TUKEY: 0.2 if n < 63 else 0.08, CAUCHY: 0.05}[kind]
    return {HUBER: 0.01, TUKEY: 0.3 if n < 63 else 0.04, CAUCHY: 0.02}[kind]


FAR_N, FAR_SHIFT, FAR_DMAX, FAR_K = 4097, 10.0, 20.0, 15.0  # the model's extent is 1.0 (the ellipsoid's x axis)


def far_case():
    """Point-to-point, Tukey: the sizes scene at 4097 points shifted by 10 x the model's extent along
    (1, 1, 1) / sqrt 3, under a gate that keeps every pair, so that the first iteration's sums depend on
    the pre-pass's shifts (around the model's centre they would cancel (10 / 0.5)^2 of their precision).
    At 100 x the extent the iteration itself is ill-posed: every scene point pairs with the one or the
    few model points that face it, Horn's scale collapses the scene, and fp64 and longdouble part ways
    by 2e-2 (30 x at 257 points: the same); at 10 x and 4097 points they agree to 2e-15."""
    m, nrm, p, _src = P.synth(FAR_N, 100 + FAR_N, 0.01)
    return m, nrm, p + FAR_SHIFT * np.ones(3) / np.sqrt(3.0)


SHELL_N, SHELL_SEED, SHELL_DMAX, SHELL_K = 2048, 2148, 0.25, 0.06
SHELL_ITERS = {"point": 20, "plane": 12}


def outlier_shell(n=SHELL_N, seed=SHELL_SEED):
    """-> (model, normals, scene, inlier (bool)): the model's own sample with 0.002 noise; a fifth of it
    pushed outward by 5-15 % of its radius and shifted 0.075 along x (a second shell near the surface,
    inside any useful gate); everything turned 5 degrees about (1, 2, 3) and shifted.  An inlier's true
    place is its model point."""
    m, nrm = P.ellipsoid(n, seed)
    r = np.random.default_rng(seed + 7)
    src = m + 0.002 * r.standard_normal((n, 3))
    out = np.zeros(n, dtype=bool)
    out[r.choice(n, n // 5, replace=False)] = True
    src[out] = src[out] * (1.0 + r.uniform(0.05, 0.15, size=(int(out.sum()), 1))) + np.array([0.075, 0.0, 0.0])
    p = src @ P.rot((1, 2, 3), 5.0).T + np.array([0.02, -0.03, 0.01])
    return m, nrm, p, ~out


def inlier_displacement(new_p, m, inlier):
    """The largest distance of an inlier from its true place."""
    return float(np.linalg.norm(np.asarray(new_p, dtype=np.float64)[inlier] - m[inlier], axis=1).max())


_cache = {}


def reference(oracle, key, dtype=np.float64):
    """The reference of a named case, computed once a session and shared (never modified).
    key: ("size", metric, kind, n) | ("far",) | ("shell", metric, kind) -> (m, normals, p, dmax, kind, k, ref)"""
    ck = (key, dtype)
    if ck in _cache:
        return _cache[ck]
    if key[0] == "size":
        _tag, metric, kind, n = key
        m, nrm, p, _src = P.synth(n, 100 + n, 0.01)
        k = k_of(metric, kind, n)
        out = (m, nrm, p, 0.0, kind, k, robust_ref(oracle, metric, m, nrm, p, 0.0, kind, k, SIZES_ITERS, -1.0, dtype))
    elif key[0] == "far":
        m, nrm, p = far_case()
        out = (m, nrm, p, FAR_DMAX, TUKEY, FAR_K,
               robust_ref(oracle, "point", m, nrm, p, FAR_DMAX, TUKEY, FAR_K, SIZES_ITERS, -1.0, dtype))
    elif key[0] == "shell":
        _tag, metric, kind = key
        m, nrm, p, _inl = outlier_shell()
        k = SHELL_K if kind != NONE else 0.0
        out = (m, nrm, p, SHELL_DMAX, kind, k,
               robust_ref(oracle, metric, m, nrm, p, SHELL_DMAX, kind, k, SHELL_ITERS[metric], -1.0, dtype))
    else:
        raise KeyError(key)
    _cache[ck] = out
    return out
