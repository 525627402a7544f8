"""The composed reference of the kept-pairs loop (run_kept in icp_run.hip): every combination of the
metric, the max-distance gate, the trim, the robust weights and one-to-one in ONE restatement, built
from the pieces of the seven feature references (gated_ref, trim_ref, unique_ref, plane_ref, robust_ref,
symm_ref, gicp_ref), and the inputs of the option matrix (tests/test_kept_ref.py on the CPU,
tests/test_gpu_kept_matrix.py).

One iteration on the current scene p (all n points); D = dmax * dmax (+inf without a gate),
T = trim_ref.trim_count(f, n) with a trim, k2 = k * k in fp64 with weights, c = the model's centroid,
Q = the rotation of the total transform at the iteration's start (the identity at first), least = 4
(point) or 6 (plane, symm, gicp):
  1. every metric, in the engine's order: Y, idx = closest(p, m) (the oracle's fp64 search);
     d2_i = (dx*dx + dy*dy) + dz*dz (gated_ref.d2_of);  C = the T-th smallest d2 over ALL pairs (+inf
     without a trim);  B_j = min{ d2_i : idx_i = j } (unique_ref.unique_mask: a NaN never wins, ties are
     kept whole);  keep_i = d2_i <= min(D, C) and (not one_to_one or d2_i == B[idx_i]);  K = #keep
  2. the kept pairs' squared residual r2 and whether the pair is live:
       point  r2 = d2
       plane  r = d . N[idx], r2 = r * r
       symm   n by symm_ref.pair_normals(N[idx], U0, Q), r = d . n, r2 = r * r; live: n != 0
       gicp   M by gicp_ref.information(N[idx], U0, Q, 1 - eps), r2 = d^T M d (gicp_ref.mahalanobis);
              live: S positive definite
  3. w = robust_ref.weights(kind, r2, k) (1 without weights; 0 for a pair not live);  W = sum w,
     K+ = #{w > 0}
  4. K < least, T < least with a trim, K+ < least with weights: stop before the iteration changes
     anything ("few")
  5. the metric's step on the kept pairs:
       point  Horn's closed form: robust_ref.weighted_horn on the weighted sums (unweighted in fp64: the
              oracle's find_alignment, as gated_ref, trim_ref and unique_ref)
       plane  a = [(p - c) x n ; n]: (sum w a a^T) x = -sum w a r, plane_ref._solve ("degenerate"),
              R = plane_ref._rodrigues, t = (c + tau) - R c, s = 1
       symm   a = [((p - c) + (Y - c)) x n ; n], the same system, symm_ref.half_step;  Q' = R Q
       gicp   gicp_ref.pair_sums, plane_ref._solve, R = plane_ref._rodrigues, t = (c + tau) - R c;  Q' = R Q
  6. every point moves, q = s R p + t;  e = the kept pairs' UNWEIGHTED residual of rule 2 after the move
     (symm and gicp: with Q');  err = (e + e) / K (unweighted point in fp64: (align.err + e) / K with the
     oracle's err_compute)
dtype = np.float64 restates the engine's arithmetic; dtype = np.longdouble is the extended-precision
truth (the searches stay the oracle's fp64 ones; k2 and 1 - eps stay the fp64 values).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import gicp_ref as GI
import plane_ref as P
import symm_ref as S
import trim_ref as TR
import unique_ref as U
from gated_ref import d2_of
from gicp_ref import information, mahalanobis, pair_sums
from plane_ref import _rodrigues, _solve
from robust_ref import CAUCHY, HUBER, NONE, TUKEY, weighted_horn, weights
from symm_ref import half_step, pair_normals

METRICS = ("point", "plane", "symm", "gicp")
KINDS = {"none": NONE, "huber": HUBER, "tukey": TUKEY, "cauchy": CAUCHY}


def _unique(idx, d2, nm, dtype):
    """unique_ref.unique_mask; its table is fp64, so a wider d2 enters as its ranks (the same order, the
    same ties; a NaN stays a NaN)."""
    if dtype is np.float64:
        return U.unique_mask(idx, d2, nm)
    rank = np.unique(d2, return_inverse=True)[1].reshape(-1).astype(np.float64)
    rank[np.isnan(d2)] = np.nan
    return U.unique_mask(idx, rank, nm)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def kept_ref(oracle, m, p, *, metric, N=None, U0=None, eps=None, dmax=0.0, trim=None, robust=None, one_to_one=False,
             max_iter, threshold=-1.0, dtype=np.float64):
    """metric: "point" | "plane" | "symm" | "gicp" (N: the model's normals, U0: the scene's, eps: gicp's);
    dmax: 0, None or inf: no gate; trim: the fraction or None; robust: (kind, k) or None.
    -> dict(new_p, err (array), K (list), mask (the last one evaluated), s, R, t (the last completed
    iteration's), Q (the total's rotation), iterations, status ('ok' | 'few' | 'degenerate'), fail_iter,
    K_fail, Kpos_fail, min_pivot, T (None without a trim);
    W, Kpos, Kover (#{live kept pairs with r2 > k2}) (lists, empty without weights), C (list, empty
    without a trim);
    gate_margin (min |d2 - D| / D over the iterations and ALL pairs), trim_margin (min (d2_(T+1) - C) / C),
    unique_margin (min unique_ref.unique_margin), k_margin (min |r2 - k2| / k2 over the kept live pairs,
    Huber and Tukey): each inf where its option is off)."""
    if metric not in METRICS:
        raise ValueError(metric)
    plane = metric != "point"
    least = 6 if plane else 4
    kind, k = robust if robust else (NONE, 0.0)
    weighted = kind != NONE
    oracle_horn = metric == "point" and not weighted and dtype is np.float64
    m64 = np.ascontiguousarray(m, dtype=np.float64)
    mx = m64.astype(dtype)
    Nx = np.ascontiguousarray(N, dtype=np.float64).astype(dtype) if plane else None
    Ux = np.ascontiguousarray(U0, dtype=np.float64).astype(dtype) if metric in ("symm", "gicp") else None
    p = np.ascontiguousarray(p, dtype=np.float64).astype(dtype)
    n, nm = p.shape[0], mx.shape[0]
    c = mx.sum(axis=0) / dtype(nm)
    D = np.float64(dmax) * np.float64(dmax) if dmax is not None and dmax > 0 and np.isfinite(dmax) else np.float64(np.inf)
    T = TR.trim_count(trim, n) if trim is not None else None
    k2 = dtype(np.float64(k) * np.float64(k))
    k1 = dtype(np.float64(1.0) - np.float64(eps)) if metric == "gicp" else None  # (fp64, once, as the host forms it)
    Q = np.eye(3, dtype=dtype)
    Ks, errs, Ws, Kps, Kos, Cs = [], [], [], [], [], []
    out = dict(status="ok", gate_margin=np.inf, trim_margin=np.inf, unique_margin=np.inf, k_margin=np.inf, min_pivot=np.inf,
               s=1.0, R=np.eye(3, dtype=dtype), t=np.zeros(3, dtype=dtype), mask=np.zeros(n, dtype=bool), fail_iter=-1,
               K_fail=-1, Kpos_fail=-1, T=T)
    for it in range(max_iter):
        # 1. the kept set
        p64 = np.ascontiguousarray(p, dtype=np.float64)
        _Y, idx = oracle.closest(p64, m64)
        idx = np.asarray(idx).astype(np.int64)
        Y = mx[idx]
        d2 = d2_of(p, Y)
        cut = D
        if T is not None:
            srt = np.sort(d2)
            C = srt[T - 1]
            cut = min(D, C)
            if T < n and C > 0:
                out["trim_margin"] = min(out["trim_margin"], float((srt[T] - C) / C))
        with np.errstate(invalid="ignore"):
            keep = d2 <= cut
            if one_to_one:
                keep = _unique(idx, d2, nm, dtype) & keep
                out["unique_margin"] = min(out["unique_margin"], U.unique_margin(idx, d2))
        keep = np.asarray(keep, dtype=bool)
        out["mask"] = keep
        if np.isfinite(D):
            out["gate_margin"] = min(out["gate_margin"], float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        pk, Yk = p[keep], Y[keep]
        d = pk - Yk
        # 2. the residual
        live = np.ones(K, dtype=bool)
        if metric == "point":
            r2 = d2[keep]
        elif metric == "plane":
            nk = Nx[idx][keep]
            r = _dot3(d, nk)
            r2 = r * r
        elif metric == "symm":
            Nk, Uk = Nx[idx][keep], Ux[keep]
            nk, live = pair_normals(Nk, Uk, Q)
            r = _dot3(d, nk)
            r2 = r * r
        else:
            Nk, Uk = Nx[idx][keep], Ux[keep]
            M, live = information(Nk, Uk, Q, k1, dtype)
            _g, r2 = mahalanobis(M, d)
        # 3. the weights
        w = weights(kind, r2, k, dtype) if weighted else np.ones(K, dtype=dtype)
        if metric in ("symm", "gicp"):
            w = np.where(live, w, dtype(0))
        Kpos = int((w > 0).sum())
        W = w.sum() if K else dtype(0)
        if kind in (HUBER, TUKEY) and live.any():
            out["k_margin"] = min(out["k_margin"], float(np.min(np.abs(r2[live] - k2) / k2)))
        # 4. too few
        if K < least or (T is not None and T < least) or (weighted and Kpos < least):
            out.update(status="few", fail_iter=it, K_fail=K, Kpos_fail=Kpos)
            break
        # 5. the step, 6. the move and the residual after it
        if oracle_horn:
            al = oracle.find_alignment(p[keep], Y[keep])
            s, R, t = al.s, np.array(al.R).reshape(3, 3), np.array(al.t)
            e, kept_new = oracle.err_compute(p[keep], Y[keep], al.s, al.R, al.t)
            new_p = np.empty_like(p)
            new_p[keep] = kept_new
            if K < n:
                _e, rest_new = oracle.err_compute(p[~keep], Y[~keep], al.s, al.R, al.t)
                new_p[~keep] = rest_new
            p = new_p
            err = (al.err + e) / K
        elif metric == "point":
            s, R, t = weighted_horn(oracle, pk, Yk, w, dtype)
            p = p @ (s * R).T + t
            e = _dot3(p[keep] - Yk, p[keep] - Yk).sum()
            err = (e + e) / dtype(K)
        else:
            if metric == "gicp":
                A, b = pair_sums(pk - c, M, d, w if weighted else None)
            else:
                v = (pk - c) + (Yk - c) if metric == "symm" else pk - c
                a = np.concatenate([np.cross(v, nk), nk], axis=1)
                if metric == "plane" and not weighted:  # (plane_ref's own expression: the same sums)
                    A = a.T @ a
                    b = -(a * r[:, None]).sum(axis=0)
                else:
                    A = (a * w[:, None]).T @ a
                    b = -(a * (w * r)[:, None]).sum(axis=0)
            x, piv = _solve(A, b, dtype)
            out["min_pivot"] = min(out["min_pivot"], float(piv))
            if x is None:
                out.update(status="degenerate", fail_iter=it, K_fail=K, Kpos_fail=Kpos, min_pivot=float(piv))
                break
            s = dtype(1)
            if metric == "symm":
                R, t = half_step(x, c, dtype)
            else:
                R = _rodrigues(x[:3], dtype)
                t = (c + x[3:]) - R @ c
            Q = R @ Q
            p = p @ R.T + t
            q = p[keep] - Yk
            if metric == "plane":
                rn = _dot3(q, nk)
                e = (rn * rn).sum()
            elif metric == "symm":
                rn = _dot3(q, pair_normals(Nk, Uk, Q)[0])
                e = (rn * rn).sum()
            else:
                e = mahalanobis(information(Nk, Uk, Q, k1, dtype)[0], q)[1].sum()
            err = (e + e) / dtype(K)
        out.update(s=s, R=R, t=t)
        Ks.append(K)
        errs.append(err)
        if weighted:
            Ws.append(W)
            Kps.append(Kpos)
            with np.errstate(invalid="ignore"):
                Kos.append(int((r2[live] > k2).sum()))
        if T is not None:
            Cs.append(float(C))
        if err < threshold:
            break
    out.update(new_p=p, K=Ks, err=np.array(errs, dtype=dtype), iterations=len(errs), Q=Q, W=Ws, Kpos=Kps, Kover=Kos, C=Cs)
    return out


# ---- the option matrix ------------------------------------------------------------------------
# A cell is (metric, gate, trim, kind name, one_to_one); its case is plane_ref.gate_case(n) with the
# scene's exact normals and gicp_ref.EPS.  tests/test_kept_ref.py checks every cell on the CPU (status,
# margins > 1e-6, the weights and both cuts bite, fp64 against longdouble, the K lists below) before
# tests/test_gpu_kept_matrix.py compares masks and counts exactly.

MATRIX_N, MATRIX_ITERS = 257, 4
ROW_N = 4097  # the "everything on" row: one point past kRedSingle
DMAX = 0.08
TRIM = {MATRIX_N: 0.414, ROW_N: 0.627}
# the robust scale by size, metric and kind: the residual is a distance (point), a distance along one
# normal (plane), along the sum of two (symm, |n| <= 2) or a Mahalanobis length with 1 / eps along the
# normals (gicp)
SCALE = {
    MATRIX_N: {"point": {"huber": 0.031, "tukey": 0.06, "cauchy": 0.05},
               "plane": {"huber": 0.01, "tukey": 0.04, "cauchy": 0.02},
               "symm": {"huber": 0.02, "tukey": 0.08, "cauchy": 0.04},
               "gicp": {"huber": 0.6, "tukey": 1.2, "cauchy": 0.8}},
    ROW_N: {"point": {"huber": 0.03, "tukey": 0.06, "cauchy": 0.05},
            "plane": {"huber": 0.012, "tukey": 0.04, "cauchy": 0.02},
            "symm": {"huber": 0.02, "tukey": 0.08, "cauchy": 0.04},
            "gicp": {"huber": 0.6, "tukey": 1.2, "cauchy": 0.8}},
}

# cell -> K of each iteration, this reference's own (fp64 and longdouble alike)
MATRIX_K = {
    ("point", False, False, "none", False): [257, 257, 257, 257],
    ("point", False, False, "none", True): [143, 148, 149, 146],
    ("point", False, False, "huber", False): [257, 257, 257, 257],
    ("point", False, False, "huber", True): [143, 150, 152, 153],
    ("point", False, False, "tukey", False): [257, 257, 257, 257],
    ("point", False, False, "tukey", True): [143, 146, 144, 147],
    ("point", False, False, "cauchy", False): [257, 257, 257, 257],
    ("point", False, False, "cauchy", True): [143, 149, 152, 153],
    ("point", False, True, "none", False): [106, 106, 106, 106],
    ("point", False, True, "none", True): [91, 92, 94, 94],
    ("point", False, True, "huber", False): [106, 106, 106, 106],
    ("point", False, True, "huber", True): [91, 92, 92, 95],
    ("point", False, True, "tukey", False): [106, 106, 106, 106],
    ("point", False, True, "tukey", True): [91, 93, 91, 91],
    ("point", False, True, "cauchy", False): [106, 106, 106, 106],
    ("point", False, True, "cauchy", True): [91, 92, 92, 95],
    ("point", True, False, "none", False): [104, 118, 125, 131],
    ("point", True, False, "none", True): [89, 101, 103, 105],
    ("point", True, False, "huber", False): [104, 117, 118, 126],
    ("point", True, False, "huber", True): [89, 99, 100, 102],
    ("point", True, False, "tukey", False): [104, 112, 118, 119],
    ("point", True, False, "tukey", True): [89, 97, 101, 102],
    ("point", True, False, "cauchy", False): [104, 117, 118, 127],
    ("point", True, False, "cauchy", True): [89, 99, 100, 102],
    ("point", True, True, "none", False): [104, 106, 106, 106],
    ("point", True, True, "none", True): [89, 93, 93, 94],
    ("point", True, True, "huber", False): [104, 106, 106, 106],
    ("point", True, True, "huber", True): [89, 91, 93, 93],
    ("point", True, True, "tukey", False): [104, 106, 106, 106],
    ("point", True, True, "tukey", True): [89, 93, 91, 91],
    ("point", True, True, "cauchy", False): [104, 106, 106, 106],
    ("point", True, True, "cauchy", True): [89, 91, 92, 93],
    ("plane", False, False, "none", False): [257, 257, 257, 257],
    ("plane", False, False, "none", True): [143, 116, 140, 129],
    ("plane", False, False, "huber", False): [257, 257, 257, 257],
    ("plane", False, False, "huber", True): [143, 150, 153, 154],
    ("plane", False, False, "tukey", False): [257, 257, 257, 257],
    ("plane", False, False, "tukey", True): [143, 145, 151, 150],
    ("plane", False, False, "cauchy", False): [257, 257, 257, 257],
    ("plane", False, False, "cauchy", True): [143, 148, 153, 157],
    ("plane", False, True, "none", False): [106, 106, 106, 106],
    ("plane", False, True, "none", True): [91, 89, 90, 93],
    ("plane", False, True, "huber", False): [106, 106, 106, 106],
    ("plane", False, True, "huber", True): [91, 94, 92, 90],
    ("plane", False, True, "tukey", False): [106, 106, 106, 106],
    ("plane", False, True, "tukey", True): [91, 94, 95, 91],
    ("plane", False, True, "cauchy", False): [106, 106, 106, 106],
    ("plane", False, True, "cauchy", True): [91, 94, 93, 93],
    ("plane", True, False, "none", False): [104, 128, 135, 130],
    ("plane", True, False, "none", True): [89, 106, 110, 118],
    ("plane", True, False, "huber", False): [104, 120, 131, 139],
    ("plane", True, False, "huber", True): [89, 105, 110, 113],
    ("plane", True, False, "tukey", False): [104, 106, 103, 100],
    ("plane", True, False, "tukey", True): [89, 95, 90, 92],
    ("plane", True, False, "cauchy", False): [104, 119, 127, 132],
    ("plane", True, False, "cauchy", True): [89, 100, 109, 110],
    ("plane", True, True, "none", False): [104, 106, 106, 106],
    ("plane", True, True, "none", True): [89, 90, 90, 97],
    ("plane", True, True, "huber", False): [104, 106, 106, 106],
    ("plane", True, True, "huber", True): [89, 93, 93, 91],
    ("plane", True, True, "tukey", False): [104, 106, 103, 100],
    ("plane", True, True, "tukey", True): [89, 94, 90, 92],
    ("plane", True, True, "cauchy", False): [104, 106, 106, 106],
    ("plane", True, True, "cauchy", True): [89, 93, 93, 93],
    ("symm", False, False, "none", False): [257, 257, 257, 257],
    ("symm", False, False, "none", True): [143, 131, 129, 118],
    ("symm", False, False, "huber", False): [257, 257, 257, 257],
    ("symm", False, False, "huber", True): [143, 150, 156, 154],
    ("symm", False, False, "tukey", False): [257, 257, 257, 257],
    ("symm", False, False, "tukey", True): [143, 147, 152, 155],
    ("symm", False, False, "cauchy", False): [257, 257, 257, 257],
    ("symm", False, False, "cauchy", True): [143, 148, 152, 158],
    ("symm", False, True, "none", False): [106, 106, 106, 106],
    ("symm", False, True, "none", True): [91, 90, 89, 87],
    ("symm", False, True, "huber", False): [106, 106, 106, 106],
    ("symm", False, True, "huber", True): [91, 93, 90, 93],
    ("symm", False, True, "tukey", False): [106, 106, 106, 106],
    ("symm", False, True, "tukey", True): [91, 93, 95, 92],
    ("symm", False, True, "cauchy", False): [106, 106, 106, 106],
    ("symm", False, True, "cauchy", True): [91, 94, 89, 92],
    ("symm", True, False, "none", False): [104, 128, 137, 137],
    ("symm", True, False, "none", True): [89, 105, 107, 116],
    ("symm", True, False, "huber", False): [104, 123, 136, 138],
    ("symm", True, False, "huber", True): [89, 103, 111, 115],
    ("symm", True, False, "tukey", False): [104, 109, 113, 105],
    ("symm", True, False, "tukey", True): [89, 95, 100, 93],
    ("symm", True, False, "cauchy", False): [104, 122, 132, 136],
    ("symm", True, False, "cauchy", True): [89, 101, 107, 112],
    ("symm", True, True, "none", False): [104, 106, 106, 106],
    ("symm", True, True, "none", True): [89, 90, 87, 87],
    ("symm", True, True, "huber", False): [104, 106, 106, 106],
    ("symm", True, True, "huber", True): [89, 95, 92, 90],
    ("symm", True, True, "tukey", False): [104, 106, 106, 106],
    ("symm", True, True, "tukey", True): [89, 95, 93, 92],
    ("symm", True, True, "cauchy", False): [104, 106, 106, 106],
    ("symm", True, True, "cauchy", True): [89, 96, 90, 92],
    ("gicp", False, False, "none", False): [257, 257, 257, 257],
    ("gicp", False, False, "none", True): [143, 150, 152, 155],
    ("gicp", False, False, "huber", False): [257, 257, 257, 257],
    ("gicp", False, False, "huber", True): [143, 155, 157, 151],
    ("gicp", False, False, "tukey", False): [257, 257, 257, 257],
    ("gicp", False, False, "tukey", True): [143, 150, 160, 156],
    ("gicp", False, False, "cauchy", False): [257, 257, 257, 257],
    ("gicp", False, False, "cauchy", True): [143, 153, 157, 152],
    ("gicp", False, True, "none", False): [106, 106, 106, 106],
    ("gicp", False, True, "none", True): [91, 92, 92, 97],
    ("gicp", False, True, "huber", False): [106, 106, 106, 106],
    ("gicp", False, True, "huber", True): [91, 91, 95, 92],
    ("gicp", False, True, "tukey", False): [106, 106, 106, 106],
    ("gicp", False, True, "tukey", True): [91, 92, 93, 95],
    ("gicp", False, True, "cauchy", False): [106, 106, 106, 106],
    ("gicp", False, True, "cauchy", True): [91, 91, 94, 96],
    ("gicp", True, False, "none", False): [104, 129, 132, 132],
    ("gicp", True, False, "none", True): [89, 112, 111, 115],
    ("gicp", True, False, "huber", False): [104, 129, 133, 124],
    ("gicp", True, False, "huber", True): [89, 108, 115, 118],
    ("gicp", True, False, "tukey", False): [104, 121, 135, 128],
    ("gicp", True, False, "tukey", True): [89, 100, 107, 113],
    ("gicp", True, False, "cauchy", False): [104, 125, 134, 131],
    ("gicp", True, False, "cauchy", True): [89, 106, 112, 119],
    ("gicp", True, True, "none", False): [104, 106, 106, 106],
    ("gicp", True, True, "none", True): [89, 91, 90, 99],
    ("gicp", True, True, "huber", False): [104, 106, 106, 106],
    ("gicp", True, True, "huber", True): [89, 92, 94, 95],
    ("gicp", True, True, "tukey", False): [104, 106, 106, 106],
    ("gicp", True, True, "tukey", True): [89, 91, 92, 95],
    ("gicp", True, True, "cauchy", False): [104, 106, 106, 106],
    ("gicp", True, True, "cauchy", True): [89, 92, 94, 96],
}
ROW_K = {
    ("point", True, True, "none", True): [1824, 1833, 1829, 1833],
    ("point", True, True, "huber", True): [1824, 1832, 1841, 1833],
    ("point", True, True, "tukey", True): [1824, 1838, 1837, 1839],
    ("point", True, True, "cauchy", True): [1824, 1832, 1835, 1832],
    ("plane", True, True, "none", True): [1824, 1877, 1840, 1859],
    ("plane", True, True, "huber", True): [1824, 1849, 1842, 1848],
    ("plane", True, True, "tukey", True): [1824, 1841, 1847, 1856],
    ("plane", True, True, "cauchy", True): [1824, 1857, 1849, 1847],
    ("symm", True, True, "none", True): [1824, 1869, 1857, 1864],
    ("symm", True, True, "huber", True): [1824, 1839, 1847, 1864],
    ("symm", True, True, "tukey", True): [1824, 1840, 1860, 1841],
    ("symm", True, True, "cauchy", True): [1824, 1861, 1846, 1857],
    ("gicp", True, True, "none", True): [1824, 1851, 1830, 1830],
    ("gicp", True, True, "huber", True): [1824, 1841, 1864, 1851],
    ("gicp", True, True, "tukey", True): [1824, 1858, 1865, 1860],
    ("gicp", True, True, "cauchy", True): [1824, 1860, 1858, 1858],
}


def cells(metric=None):
    """The 128 cells (the 32 of one metric), in the order of the tables."""
    return [(mt, gate, trim, kname, uniq) for mt in METRICS if metric in (None, mt) for gate in (False, True)
            for trim in (False, True) for kname in KINDS for uniq in (False, True)]


def row_cells():
    """The 16 cells with the gate, the trim and one-to-one on."""
    return [(mt, True, True, kname, True) for mt in METRICS for kname in KINDS]


def cell_id(cell):
    mt, gate, trim, kname, uniq = cell
    return f"{mt}-gate{int(gate)}-trim{int(trim)}-{kname}-uniq{int(uniq)}"


_cases = {}


def matrix_case(n):
    """-> (model, its normals, scene, the scene's normals), shared (never modified)."""
    if n not in _cases:
        m, nrm, p = P.gate_case(n)
        _cases[n] = (m, nrm, p, S.scene_normals_of(nrm))
    return _cases[n]


def cell_options(cell, n):
    """-> dict(dmax, trim, robust, one_to_one): kept_ref's keywords, and what the setters take."""
    mt, gate, trim, kname, uniq = cell
    return dict(dmax=DMAX if gate else 0.0, trim=TRIM[n] if trim else None,
                robust=(KINDS[kname], SCALE[n][mt][kname]) if kname != "none" else None, one_to_one=uniq)


_cache = {}


def reference(oracle, n, cell, dtype=np.float64):
    """The reference of a cell at n points, computed once a session and shared (never modified)."""
    ck = (n, cell, dtype)
    if ck not in _cache:
        m, nrm, p, U0 = matrix_case(n)
        _cache[ck] = kept_ref(oracle, m, p, metric=cell[0], N=nrm, U0=U0, eps=GI.EPS, max_iter=MATRIX_ITERS, threshold=-1.0,
                              dtype=dtype, **cell_options(cell, n))
    return _cache[ck]
