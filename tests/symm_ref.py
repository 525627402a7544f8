"""The reference of the symmetric point-to-plane ICP loop (icp_set_plane_symmetric, icp_plane.hip's
symm_* kernels), restated with the oracle's nearest-neighbour search and numpy, and the inputs of its
tests (tests/test_symm_ref.py on the CPU, tests/test_gpu_symm.py).

One iteration on the current scene p (all n points); N = the model's normals, U0 = the scene's normals
as given (the frame of the scene as given), c = the model's centroid, D = dmax * dmax (+inf without a
gate), Q = the rotation of the total transform at the iteration's start (the identity at first):
  1. Y, idx = closest(p, m);  d = p - Y;  d2_j = (dx*dx + dy*dy) + dz*dz;  keep_j = d2_j <= min(D, C), C
     the T-th smallest d2 with a trim (trim_ref's rule), else +inf;  K = #keep
  2. N_j = N[idx_j], u_j = Q u0_j (rows ((Q0 u0 + Q1 u1) + Q2 u2)), h = (Nx ux + Ny uy) + Nz uz;
     n_j = 0 when N_j or u0_j is all zero, else h < 0 ? N_j - u_j : N_j + u_j
  3. K < 6 (with a trim T < 6; with weights K+ < 6): stop before the iteration changes anything ("few")
  4. over the kept pairs with n_j != 0: v_j = (p_j - c) + (Y_j - c), a_j = [v_j x n_j ; n_j],
     r_j = (dx nx + dy ny) + dz nz, w_j = the robust weight of r_j * r_j (robust_ref.weights; 1 without):
     A = sum w a a^T, b = -sum w a r; W = sum w, K+ = #{w > 0} (a pair with n_j = 0 counts in K alone)
  5. plane_ref's scaled Cholesky and pivot rule ("degenerate")
  6. a~ = x[:3], t~ = x[3:]: aa = (a0^2 + a1^2) + a2^2, g = 1 / sqrt(1 + aa), k2 = g g / (1 + g),
     R_h = I + g [a~]x + k2 [a~]x^2, R = R_h R_h, t = ((R_h (g t~)) + c) - R c, s = 1;  Q' = R Q
  7. every point moves, q = R p + t;  n'_j by rule 2 from N_j and Q' u0_j;  e = sum over the kept j of
     ((q_j - Y_j) . n'_j)^2;  err = (e + e) / K
dtype = np.float64 restates the engine's arithmetic; dtype = np.longdouble is the extended-precision
truth (the searches stay the oracle's fp64 ones; the solve is plain elimination).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import plane_ref as P
import robust_ref as RB
import trim_ref as T
from gated_ref import d2_of


def pair_normals(Nj, U0, Q):
    """Rule 2 -> (n (k, 3), live (k,): False where n_j = 0 by the zero rule)."""
    u = np.stack([(Q[r, 0] * U0[:, 0] + Q[r, 1] * U0[:, 1]) + Q[r, 2] * U0[:, 2] for r in range(3)], axis=1)
    h = (Nj[:, 0] * u[:, 0] + Nj[:, 1] * u[:, 1]) + Nj[:, 2] * u[:, 2]
    live = ~(np.all(Nj == 0, axis=1) | np.all(U0 == 0, axis=1))
    n = np.where((h < 0)[:, None], Nj - u, Nj + u)
    n[~live] = 0
    return n, live


def half_step(x, c, dtype):
    """Rule 6 -> (R, t)."""
    a0, a1, a2 = x[0], x[1], x[2]
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    g = dtype(1) / np.sqrt(dtype(1) + aa)
    k2 = g * g / (dtype(1) + g)
    H = np.array([[1 - k2 * (a1 * a1 + a2 * a2), k2 * (a0 * a1) - g * a2, k2 * (a0 * a2) + g * a1],
                  [k2 * (a0 * a1) + g * a2, 1 - k2 * (a0 * a0 + a2 * a2), k2 * (a1 * a2) - g * a0],
                  [k2 * (a0 * a2) - g * a1, k2 * (a1 * a2) + g * a0, 1 - k2 * (a0 * a0 + a1 * a1)]], dtype=dtype)
    tau = g * x[3:]
    R = H @ H
    return R, (H @ tau + c) - R @ c


def symm_ref(oracle, m, N, p, U0, dmax, max_iter, threshold=1e-5, dtype=np.float64, trim=None, robust=None):
    """-> plane_ref's dict, and Q (the total's rotation), W, Kpos (lists, with robust = (kind, k)), C (list,
    with trim = the fraction)."""
    m64 = np.ascontiguousarray(m, dtype=np.float64)
    mx = m64.astype(dtype)
    Nx = np.ascontiguousarray(N, dtype=np.float64).astype(dtype)
    Ux = np.ascontiguousarray(U0, dtype=np.float64).astype(dtype)
    p = np.ascontiguousarray(p, dtype=np.float64).astype(dtype)
    npts = p.shape[0]
    c = mx.sum(axis=0) / dtype(mx.shape[0])
    D = np.float64(dmax) * np.float64(dmax) if dmax is not None and dmax > 0 and np.isfinite(dmax) else np.inf
    Tn = T.trim_count(trim, npts) if trim is not None else None
    Q = np.eye(3, dtype=dtype)
    Ks, errs, Ws, Kps, Cs = [], [], [], [], []
    out = dict(status="ok", margin=np.inf, min_pivot=np.inf, s=1.0, R=np.eye(3, dtype=dtype), t=np.zeros(3, dtype=dtype),
               mask=np.zeros(npts, dtype=bool), fail_iter=-1, K_fail=-1)
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
        n, live = pair_normals(Nk, Uk, Q)
        d = pk - Yk
        r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        w = RB.weights(robust[0], r * r, robust[1], dtype) if robust else np.ones(K, dtype=dtype)
        w = np.where(live, w, dtype(0))
        Kpos = int((w > 0).sum())
        if K < 6 or (Tn is not None and Tn < 6) or (robust and Kpos < 6):
            out.update(status="few", fail_iter=it, K_fail=K)
            break
        v = (pk - c) + (Yk - c)
        a = np.concatenate([np.cross(v, n), n], axis=1)
        A = (a * w[:, None]).T @ a
        b = -(a * (w * r)[:, None]).sum(axis=0)
        x, piv = P._solve(A, b, dtype)
        out["min_pivot"] = min(out["min_pivot"], float(piv))
        if x is None:
            out.update(status="degenerate", fail_iter=it, K_fail=K, min_pivot=float(piv))
            break
        R, t = half_step(x, c, dtype)
        Q = R @ Q
        p = p @ R.T + t
        n2, _live = pair_normals(Nk, Uk, Q)
        q = p[keep] - Yk
        rn = (q[:, 0] * n2[:, 0] + q[:, 1] * n2[:, 1]) + q[:, 2] * n2[:, 2]
        e = (rn * rn).sum()
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

TURN = P.rot((1, 2, 3), 5.0)  # the scene of plane_ref.synth is its source turned by this


def scene_normals_of(nrm):
    """The exact normals of plane_ref.synth's scene when the scene is the model moved: N turned with it."""
    return nrm @ TURN.T


SIZES = P.SIZES  # plane_ref.synth(n, 100 + n, 0.01) with U0 = N @ rot((1, 2, 3), 5).T, no gate
SIZES_ITERS = 6
GATES = {(257, 0.08): [104, 128, 137, 137, 128, 124, 127, 123],  # (n, dmax) -> K of each iteration
         (4097, 0.08): [2543, 2663, 2708, 2712, 2711, 2713, 2714, 2714]}
GATES_ITERS = 8
TRIM = 0.75  # the gate case (4097, 0.08) with icp_set_trim(0.75)
TUKEY_K = 0.2  # ... and with Tukey weights: k well above the gated pairs' residual along n (|n| <= 2)


def planar():
    """plane_ref.planar with the scene's exact normals: degenerate at iteration 0."""
    m, nrm, p = P.planar()
    return m, nrm, p, nrm @ P.rot((1, 2, 3), 2.0).T


def five():
    """plane_ref.five with scene normals: too few for the 6 x 6 system."""
    m, nrm, p = P.five()
    return m, nrm, p, scene_normals_of(nrm)


def purpose():
    """-> (model, its normals, scene, the scene's exact normals, src): a different sample of the same
    ellipsoid, turned 15 degrees about (1, 2, 3) and shifted, no noise."""
    m, nrm = P.ellipsoid(2049, 4197)
    src, snrm = P.ellipsoid(2049, 5197)
    R = P.rot((1, 2, 3), 15.0)
    return m, nrm, src @ R.T + np.array([0.02, -0.03, 0.01]), snrm @ R.T, src


_cache = {}


def reference(oracle, key, dtype=np.float64):
    """The reference of a named case, computed once a session and shared (never modified).
    key: ("size", n) | ("gate", n, dmax) | ("trim", n, dmax) | ("tukey", n, dmax)
    -> (m, normals, p, scene normals, dmax, ref)"""
    ck = (key, dtype)
    if ck in _cache:
        return _cache[ck]
    if key[0] == "size":
        m, nrm, p, _src = P.synth(key[1], 100 + key[1], 0.01)
        U0 = scene_normals_of(nrm)
        out = (m, nrm, p, U0, 0.0, symm_ref(oracle, m, nrm, p, U0, 0.0, SIZES_ITERS, -1.0, dtype))
    elif key[0] in ("gate", "trim", "tukey"):
        m, nrm, p = P.gate_case(key[1])
        U0 = scene_normals_of(nrm)
        more = dict(trim=TRIM) if key[0] == "trim" else dict(robust=(RB.TUKEY, TUKEY_K)) if key[0] == "tukey" else {}
        out = (m, nrm, p, U0, key[2], symm_ref(oracle, m, nrm, p, U0, key[2], GATES_ITERS, -1.0, dtype, **more))
    else:
        raise KeyError(key)
    _cache[ck] = out
    return out
