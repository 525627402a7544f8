"""The reference of the plane-to-plane ICP loop (icp_set_plane_to_plane, icp_gicp.hip: generalised ICP
in the regularised form of PCL and Open3D), restated with the oracle's nearest-neighbour search and
numpy, and the inputs of its tests (tests/test_gicp_ref.py on the CPU, tests/test_gpu_gicp.py).

A point's covariance has the eigenvalues (eps, 1, 1), eps along its normal: C = I - (1 - eps) n n^T.
One iteration on the current scene p (all n points); N = the model's normals, U0 = the scene's normals
as given (the frame of the scene as given), c = the model's centroid, D = dmax * dmax (+inf without a
gate), Q = the rotation of the total transform at the iteration's start (the identity at first),
k1 = 1 - eps:
  1. Y, idx = closest(p, m);  d = p - Y;  d2_j = (dx*dx + dy*dy) + dz*dz;  keep_j = d2_j <= min(D, C), C
     the T-th smallest d2 with a trim (trim_ref's rule), else +inf;  K = #keep
  2. N_j = N[idx_j], u_j = Q u0_j (rows ((Q0 u0 + Q1 u1) + Q2 u2));  S = 2 I - k1 (N_j N_j^T + u_j u_j^T), six
     entries s_ab = [a == b ? 2 : 0] - k1 * (N_a * N_b + u_a * u_b); positive definite when s00 > 0,
     s00 s11 - s01 s01 > 0 and det S > 0 (false for a NaN), else the pair counts in K and adds nothing
     else;  M_j = adj(S) * (1 / det S) (longdouble: plain elimination)
  3. v = p_j - c, g = M_j d (rows summed as above), r2 = (dx g0 + dy g1) + dz g2, w = the robust weight of
     r2 (robust_ref.weights; 1 without); with weights M and g are scaled by w.  H = [v]x M; with
     J = [-[v]x | I]: A = sum w J^T M J = [[H [v]x^T, H], [H^T, M]], b = -sum w [v x g ; g];  W = sum w,
     K+ = #{w > 0}
  4. K < 6 (with a trim T < 6; with weights K+ < 6): stop before the iteration changes anything ("few");
     plane_ref's scaled Cholesky and pivot rule ("degenerate"); R = exp([omega]x), t = (c + tau) - R c, s = 1;
     Q' = R Q
  5. every point moves, q = R p + t;  M'_j by rule 2 from N_j and Q' u0_j;  e = sum over the kept j of
     (q_j - Y_j)^T M'_j (q_j - Y_j) (0 for a pair whose S' is not positive definite);  err = (e + e) / K
dtype = np.float64 restates the engine's arithmetic; dtype = np.longdouble is the extended-precision
truth (the searches stay the oracle's fp64 ones; the inverse and the solve are plain elimination).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import plane_ref as P
import robust_ref as RB
import symm_ref as S
import trim_ref as T
from gated_ref import d2_of

EPS = 1e-3  # PCL's and Open3D's default


def _row3(a0, a1, a2, x):
    return (a0 * x[:, 0] + a1 * x[:, 1]) + a2 * x[:, 2]


def information(Nj, U0, Q, k1, dtype):
    """Rule 2 -> (M (k, 3, 3), live (k,): False where S is not positive definite, M = 0 there)."""
    u = np.stack([_row3(Q[r, 0], Q[r, 1], Q[r, 2], U0) for r in range(3)], axis=1)
    two, zero = dtype(2), dtype(0)
    s = {}
    for a in range(3):
        for b in range(a, 3):
            s[a, b] = (two if a == b else zero) - k1 * (Nj[:, a] * Nj[:, b] + u[:, a] * u[:, b])
    s00, s01, s02, s11, s12, s22 = s[0, 0], s[0, 1], s[0, 2], s[1, 1], s[1, 2], s[2, 2]
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    with np.errstate(invalid="ignore"):
        live = (s00 > 0) & (c22 > 0) & (det > 0)
    k = Nj.shape[0]
    M = np.zeros((k, 3, 3), dtype=dtype)
    if dtype is np.float64:
        with np.errstate(all="ignore"):
            inv = dtype(1) / det
        for (a, b), c in (((0, 0), c00), ((0, 1), c01), ((0, 2), c02), ((1, 1), c11), ((1, 2), c12), ((2, 2), c22)):
            M[:, a, b] = M[:, b, a] = c * inv
    else:  # Gauss-Jordan on [S | I], no pivoting (S is positive definite where it is used)
        A = np.zeros((k, 3, 6), dtype=dtype)
        for a in range(3):
            for b in range(3):
                A[:, a, b] = s[min(a, b), max(a, b)]
            A[:, a, 3 + a] = 1
        with np.errstate(all="ignore"):
            for r in range(3):
                A[:, r, :] = A[:, r, :] / A[:, r, r][:, None]
                for q in range(3):
                    if q != r:
                        A[:, q, :] = A[:, q, :] - A[:, q, r][:, None] * A[:, r, :]
        M = A[:, :, 3:].copy()
    M[~live] = 0
    return M, live


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def mahalanobis(M, d):
    """-> (g = M d (k, 3), r2 = d . g (k,)), each three-term sum as ((a + b) + c)."""
    g = np.stack([_row3(M[:, r, 0], M[:, r, 1], M[:, r, 2], d) for r in range(3)], axis=1)
    return g, (d[:, 0] * g[:, 0] + d[:, 1] * g[:, 1]) + d[:, 2] * g[:, 2]


def pair_sums(v, M, d, w=None):
    """Rule 3 -> (A (6, 6), b (6,)): the plane metric's columns, [rotation; translation]."""
    g, _r2 = mahalanobis(M, d)
    Mw, gw = (M, g) if w is None else (M * w[:, None, None], g * w[:, None])
    H = np.stack([_cross(v, Mw[:, :, k]) for k in range(3)], axis=2)  # H[:, r, k] = (v x M_k)_r
    TL = np.stack([_cross(v, H[:, r, :]) for r in range(3)], axis=1)  # TL[:, r, c] = (v x H_r)_c
    A = np.zeros((6, 6), dtype=v.dtype)
    A[:3, :3] = TL.sum(axis=0)
    A[:3, :3] = np.triu(A[:3, :3]) + np.triu(A[:3, :3], 1).T  # (the upper triangle is what is summed)
    A[:3, 3:] = H.sum(axis=0)
    A[3:, :3] = A[:3, 3:].T
    A[3:, 3:] = Mw.sum(axis=0)
    b = -np.concatenate([_cross(v, gw), gw], axis=1).sum(axis=0)
    return A, b


def gicp_ref(oracle, m, N, p, U0, eps, dmax, max_iter, threshold=1e-5, dtype=np.float64, trim=None, robust=None):
    """-> plane_ref's dict, and Q (the total's rotation), W, Kpos (lists, with robust = (kind, k)), C (list,
    with trim = the fraction), wmargin (with Tukey weights: min |r2 - k2| / k2 over the kept pairs)."""
    m64 = np.ascontiguousarray(m, dtype=np.float64)
    mx = m64.astype(dtype)
    Nx = np.ascontiguousarray(N, dtype=np.float64).astype(dtype)
    Ux = np.ascontiguousarray(U0, dtype=np.float64).astype(dtype)
    p = np.ascontiguousarray(p, dtype=np.float64).astype(dtype)
    npts = p.shape[0]
    c = mx.sum(axis=0) / dtype(mx.shape[0])
    k1 = dtype(np.float64(1.0) - np.float64(eps))  # (fp64, once, as the host forms it)
    D = np.float64(dmax) * np.float64(dmax) if dmax is not None and dmax > 0 and np.isfinite(dmax) else np.inf
    Tn = T.trim_count(trim, npts) if trim is not None else None
    Q = np.eye(3, dtype=dtype)
    Ks, errs, Ws, Kps, Cs = [], [], [], [], []
    out = dict(status="ok", margin=np.inf, wmargin=np.inf, min_pivot=np.inf, s=1.0, R=np.eye(3, dtype=dtype),
               t=np.zeros(3, dtype=dtype), mask=np.zeros(npts, dtype=bool), fail_iter=-1, K_fail=-1)
    for it in range(max_iter):
        p64 = np.ascontiguousarray(p, dtype=np.float64)
        _Y, idx = oracle.closest(p64, m64)
        Y = mx[idx]
        d2 = d2_of(p, Y)
        cut = D
        if Tn is not None:
            srt = np.sort(d2)
            C = srt[Tn - 1]
            cut = min(D, C)
            if Tn < npts and C > 0:
                out["margin"] = min(out["margin"], float((srt[Tn] - C) / C))
        with np.errstate(invalid="ignore"):
            keep = d2 <= cut
        out["mask"] = np.asarray(keep, dtype=bool)
        if np.isfinite(D):
            out["margin"] = min(out["margin"], float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        pk, Yk, Nk, Uk = p[keep], Y[keep], Nx[idx][keep], Ux[keep]
        M, live = information(Nk, Uk, Q, k1, dtype)
        d = pk - Yk
        _g, r2 = mahalanobis(M, d)
        w = RB.weights(robust[0], r2, robust[1], dtype) if robust else np.ones(K, dtype=dtype)
        w = np.where(live, w, dtype(0))
        if robust:
            k2 = dtype(robust[1]) * dtype(robust[1])
            out["wmargin"] = min(out["wmargin"], float(np.min(np.abs(r2[live] - k2) / k2)) if live.any() else np.inf)
        Kpos = int((w > 0).sum())
        if K < 6 or (Tn is not None and Tn < 6) or (robust and Kpos < 6):
            out.update(status="few", fail_iter=it, K_fail=K)
            break
        A, b = pair_sums(pk - c, M, d, w if robust else None)
        x, piv = P._solve(A, b, dtype)
        out["min_pivot"] = min(out["min_pivot"], float(piv))
        if x is None:
            out.update(status="degenerate", fail_iter=it, K_fail=K, min_pivot=float(piv))
            break
        R = P._rodrigues(x[:3], dtype)
        t = (c + x[3:]) - R @ c
        Q = R @ Q
        p = p @ R.T + t
        M2, _live = information(Nk, Uk, Q, k1, dtype)
        q = p[keep] - Yk
        e = mahalanobis(M2, q)[1].sum()
        err = (e + e) / dtype(K)
        out.update(R=R, t=t)
        Ks.append(K)
        errs.append(err)
        if robust:
            Ws.append(float(w.sum()))
            Kps.append(Kpos)
        if Tn is not None:
            Cs.append(float(C))
        if err < threshold:
            break
    out.update(new_p=p, K=Ks, err=np.array(errs, dtype=dtype), iterations=len(errs), Q=Q, W=Ws, Kpos=Kps, C=Cs)
    return out


# ---- inputs ---------------------------------------------------------------------------------

SIZES = (6, 7, 63, 65, 257, 2049)  # plane_ref.synth(n, 100 + n, 0.01) with U0 = symm_ref.scene_normals_of(N), no gate
SIZES_ITERS = 4
GATE = (2049, 0.08)  # plane_ref.gate_case(n) under dmax
GATE_ITERS = 4
TRIM = 0.5  # ... with icp_set_trim: T = 1024, below the gate's K (1196 at first)
TUKEY_K = 1.2  # ... with Tukey weights of the Mahalanobis residual: k2 = 1.44 gives part of the gated pairs weight 0


# symm_ref.purpose(): max |new_p - src| is 2.78e-5 after 5 iterations of this reference and 2.01e-4 at
# point-to-plane's fixed point (8 iterations of plane_ref), a factor of 7.2: asserted with a margin of two
PURPOSE_FACTOR = 3.6


def planar_L(n=498, seed=7):
    """A planar L-shaped patch (z = 0, the square [-1, 1]^2 without its quadrant x, y > 0; normals (0, 0, 1))
    and the same points turned 3 degrees about (1, 2, 3) and shifted, with their exact normals:
    -> (model, normals, scene, scene normals, R, t)."""
    xy = np.random.default_rng(seed).uniform(-1, 1, size=(4 * n, 2))
    xy = xy[~((xy[:, 0] > 0) & (xy[:, 1] > 0))][:n]
    assert xy.shape[0] == n
    m = np.concatenate([xy, np.zeros((n, 1))], axis=1)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    R, t = P.rot((1, 2, 3), 3.0), np.array([0.01, 0.02, 0.03])
    return m, nrm, m @ R.T + t, nrm @ R.T, R, t


_cache = {}


def reference(oracle, key, dtype=np.float64):
    """The reference of a named case, computed once a session and shared (never modified).
    key: ("size", n) | ("trim",) | ("tukey",) -> (m, normals, p, scene normals, dmax, ref)"""
    ck = (key, dtype)
    if ck in _cache:
        return _cache[ck]
    if key[0] == "size":
        m, nrm, p, _src = P.synth(key[1], 100 + key[1], 0.01)
        U0 = S.scene_normals_of(nrm)
        out = (m, nrm, p, U0, 0.0, gicp_ref(oracle, m, nrm, p, U0, EPS, 0.0, SIZES_ITERS, -1.0, dtype))
    elif key[0] in ("trim", "tukey"):
        m, nrm, p = P.gate_case(GATE[0])
        U0 = S.scene_normals_of(nrm)
        more = dict(trim=TRIM) if key[0] == "trim" else dict(robust=(RB.TUKEY, TUKEY_K))
        out = (m, nrm, p, U0, GATE[1], gicp_ref(oracle, m, nrm, p, U0, EPS, GATE[1], GATE_ITERS, -1.0, dtype, **more))
    else:
        raise KeyError(key)
    _cache[ck] = out
    return out
