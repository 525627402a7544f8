"""Extended-precision truth of one ICP iteration's arithmetic (moments, Horn's step, transform,
error), the metrics that compare an implementation with it, and the named inputs of
tests/test_align_ref.py, tests/test_horn_accuracy.py (CPU) and tests/test_gpu_align_accuracy.py.

Everything here is numpy in np.longdouble (x87 extended: 64-bit mantissa).  The moments are the
two-pass form (centroids, then centred sums), Horn's 4x4 is written as gpu.cc:106-111 writes it,
its eigenvector comes from this module's own cyclic Jacobi.  A helper module, not a conftest: no
fixtures, no hooks.

Metrics (deviation()), chosen so that conditioning does not turn them into noise:
  ds    |s - s*| / s*
  dR    max |R - R*|
  dX    max_j ||(s R p_j + t) - x*_j|| / extent, (s, R, t) under test applied in longdouble to the
        iteration's input scene, extent = max_j ||p_j - mu_p||  (t's inherent |mu| eps lands on
        the cloud's own scale)
  dP    max |scene_out - x*| / (eps64 max |x*|): the stored cloud in ulps of the coordinates
  dE    |err - err*| / err*
  dOpt  |e(s, R, t) - e*| / e*: the residual the transform under test leaves, against the optimum's
        (meaningful where R is not unique)
  dC    ||(s R mu_p* + t) - mu_y*|| / extent: where the transform puts the pairs' centroid (the truth
        puts it on mu_y*); free of R's indeterminacy on rods, so it checks t there
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "align_ref needs an extended-precision np.longdouble"
EPS64 = float(np.finfo(np.float64).eps)



def _handover():
    """icp_horn.h: the polynomial eigen path hands over to Jacobi at P'(l) <= HANDOVER |N|^3; read
    from the header, so that the tests' windows follow the constant."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "iterative-closest-point_amd", "csrc", "icp_horn.h")).read()
    m = re.search(r"if \(!\(dp > ([0-9.eE+-]+) \* nrm \* nrm \* nrm\)\) return false;", src)
    assert m, "icp_horn.h: the hand-over test of largest_eigvec_sym4_poly was not found"
    return float(m.group(1))


HANDOVER = _handover()


def _ld(a):
    return np.asarray(a, dtype=LD)


def psum(a):
    """Sum over axis 0 of a longdouble array by a balanced binary tree (error ~ eps log2 n)."""
    a = _ld(a)
    while a.shape[0] > 1:
        if a.shape[0] & 1:
            a = np.concatenate([a, np.zeros((1,) + a.shape[1:], dtype=LD)])
        a = a[0::2] + a[1::2]
    return a[0]


def jacobi_sym4(A):
    """Cyclic Jacobi on symmetric 4x4 matrices (..., 4, 4) in longdouble, run until the
    off-diagonal mass is below 1e-36 of the total (and one sweep more).
    -> (evals (..., 4), V (..., 4, 4) with the eigenvectors in its columns)."""
    A = _ld(A).copy()
    A = (A + np.swapaxes(A, -1, -2)) / LD(2)
    V = np.zeros_like(A)
    for k in range(4):
        V[..., k, k] = 1
    extra = 1
    with np.errstate(all="ignore"):
        for _sweep in range(100):
            sq = A * A
            tot = sq.sum(axis=(-1, -2))
            off = tot - sum(sq[..., k, k] for k in range(4))
            if np.all(off <= LD(1e-36) * tot):
                if extra == 0:
                    break
                extra -= 1
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = A[..., p, q]
                    nz = apq != 0
                    theta = np.where(nz, (A[..., q, q] - A[..., p, p]) / (LD(2) * np.where(nz, apq, LD(1))), LD(0))
                    t = np.where(theta >= 0, LD(1), LD(-1)) / (np.abs(theta) + np.sqrt(theta * theta + LD(1)))
                    c = LD(1) / np.sqrt(t * t + LD(1))
                    s = np.where(nz, t * c, LD(0))
                    c = np.where(nz, c, LD(1))
                    c_, s_ = c[..., None], s[..., None]
                    ap, aq = A[..., :, p].copy(), A[..., :, q].copy()
                    A[..., :, p] = c_ * ap - s_ * aq
                    A[..., :, q] = s_ * ap + c_ * aq
                    ap, aq = A[..., p, :].copy(), A[..., q, :].copy()
                    A[..., p, :] = c_ * ap - s_ * aq
                    A[..., q, :] = s_ * ap + c_ * aq
                    vp, vq = V[..., :, p].copy(), V[..., :, q].copy()
                    V[..., :, p] = c_ * vp - s_ * vq
                    V[..., :, q] = s_ * vp + c_ * vq
    ev = np.stack([A[..., k, k] for k in range(4)], axis=-1)
    V = V / np.sqrt((V * V).sum(axis=-2, keepdims=True))
    return ev, V


def horn_matrix(S):
    """Horn's 4x4 from S = sum p' y'^T (..., 3, 3), as gpu.cc:106-111 writes it (any dtype)."""
    S = np.asarray(S)
    s = lambda r, c: S[..., r, c]
    rows = [
        [s(0, 0) + s(1, 1) + s(2, 2), s(1, 2) - s(2, 1), -1 * s(0, 2) + s(2, 0), s(0, 1) - s(1, 0)],
        [-1 * s(2, 1) + s(1, 2), s(0, 0) - s(2, 2) - s(1, 1), s(0, 1) + s(1, 0), s(0, 2) + s(2, 0)],
        [s(2, 0) - s(0, 2), s(1, 0) + s(0, 1), s(1, 1) - s(2, 2) - s(0, 0), s(1, 2) + s(2, 1)],
        [-1 * s(1, 0) + s(0, 1), s(2, 0) + s(0, 2), s(2, 1) + s(1, 2), s(2, 2) - s(1, 1) - s(0, 0)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def horn_matrix_inverse(N):
    """The S whose horn_matrix is the traceless symmetric N (the map is a bijection)."""
    N = np.asarray(N)
    n = lambda r, c: N[..., r, c]
    two = N.dtype.type(2)
    rows = [[(n(0, 0) + n(1, 1)) / two, (n(1, 2) + n(0, 3)) / two, (n(1, 3) - n(0, 2)) / two],
            [(n(1, 2) - n(0, 3)) / two, (n(0, 0) + n(2, 2)) / two, (n(2, 3) + n(0, 1)) / two],
            [(n(1, 3) + n(0, 2)) / two, (n(2, 3) - n(0, 1)) / two, (n(0, 0) + n(3, 3)) / two]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def rot_from_quat(q):
    """R = (Qbar^T Q)[1:4, 1:4] of the unit quaternion q (..., 4) (gpu.cc:119-133), longdouble."""
    q = _ld(q)
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    w, x, y, z = (q[..., k] for k in range(4))
    rows = [[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def top_eigen(N):
    """-> (q (..., 4), lam1, gap = (lam1 - lam2) / max |lam|, dpoly = P'(lam1) / ||N||_inf^3) of
    symmetric 4x4 matrices, in longdouble.  dpoly is the quantity icp_horn.h's hand-over tests."""
    N = _ld(N)
    ev, V = jacobi_sym4(N)
    order = np.argsort(-ev, axis=-1)
    evs = np.take_along_axis(ev, order, axis=-1)
    q = np.take_along_axis(V, order[..., None, :1], axis=-1)[..., 0]
    lam1 = evs[..., 0]
    gap = (lam1 - evs[..., 1]) / np.abs(ev).max(axis=-1)
    sym = (N + np.swapaxes(N, -1, -2)) / LD(2)
    nrm = np.abs(sym).sum(axis=-1).max(axis=-1)
    dpoly = (lam1 - evs[..., 1]) * (lam1 - evs[..., 2]) * (lam1 - evs[..., 3]) / (nrm * nrm * nrm)
    return q, lam1, gap, dpoly


def truth_alignment(p, y):
    """Horn's closed form over the pairs (p_j, y_j), in longdouble -> dict(mu_p, mu_y, S, d_caps, sp,
    N, q, lam1, gap, dpoly, s, R, t, x (the transformed p), e = sum ||y - x||^2)."""
    p, y = _ld(p), _ld(y)
    n = LD(p.shape[0])
    mu_p, mu_y = psum(p) / n, psum(y) / n
    pc, yc = p - mu_p, y - mu_y
    S = psum(pc[:, :, None] * yc[:, None, :])
    d_caps, sp = psum((yc * yc).sum(axis=1)), psum((pc * pc).sum(axis=1))
    N = horn_matrix(S)
    q, lam1, gap, dpoly = top_eigen(N)
    R = rot_from_quat(q)
    s = np.sqrt(d_caps / sp)
    t = mu_y - s * (R @ mu_p)
    x = s * (p @ R.T) + t
    d = y - x
    e = psum((d * d).sum(axis=1))
    return dict(mu_p=mu_p, mu_y=mu_y, S=S, d_caps=d_caps, sp=sp, N=N, q=q, lam1=lam1, gap=gap, dpoly=dpoly,
                s=s, R=R, t=t, x=x, e=e)


def truth_iteration(p, y, keep=None):
    """One iteration on the scene p with the correspondences y: the alignment over the kept pairs
    (all of them without keep), EVERY point transformed, err = 2 e / K with e the kept pairs'
    residual.  -> truth_alignment's dict with x over every point, plus err, K, p, y, keep."""
    p, y = _ld(p), _ld(y)
    keep = np.ones(p.shape[0], dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    tr = truth_alignment(p[keep], y[keep])
    tr["x"] = tr["s"] * (p @ tr["R"].T) + tr["t"]
    K = int(keep.sum())
    tr.update(err=LD(2) * tr["e"] / LD(K), K=K, p=p, y=y, keep=keep)
    # lever: how far any point lies from the kept pairs' principal axis through their centroid,
    # over the extent -- what a rotation about that axis (a rod's undetermined one) moves points by
    pc = np.asarray(p - tr["mu_p"], dtype=np.float64)
    u = np.linalg.eigh(pc[keep].T @ pc[keep])[1][:, -1]
    off = pc - np.outer(pc @ u, u)
    tr["lever"] = float(np.sqrt((off * off).sum(axis=1)).max() / np.sqrt((pc[keep] ** 2).sum(axis=1)).max())
    return tr


METRICS = ("ds", "dR", "dX", "dP", "dE", "dOpt", "dC")
FLOOR = {"ds": 16 * EPS64, "dR": 16 * EPS64, "dX": 16 * EPS64, "dE": 16 * EPS64, "dOpt": 16 * EPS64, "dP": 4.0,
         "dC": 16 * EPS64}


def deviation(got, truth):
    """got: dict(s, R, t[, scene_out][, err]) of the implementation under test; truth: a
    truth_iteration.  -> dict of the metrics it can compute (floats)."""
    s, R, t = LD(got["s"]), _ld(got["R"]).reshape(3, 3), _ld(got["t"]).reshape(3)
    p, y, keep = truth["p"], truth["y"], truth["keep"]
    out = {"ds": float(abs(s - truth["s"]) / truth["s"]), "dR": float(np.abs(R - truth["R"]).max())}
    x = s * (p @ R.T) + t
    extent = np.sqrt(((p[keep] - truth["mu_p"]) ** 2).sum(axis=1)).max()
    out["dX"] = float(np.sqrt(((x - truth["x"]) ** 2).sum(axis=1)).max() / extent)
    if got.get("scene_out") is not None:
        out["dP"] = float(np.abs(_ld(got["scene_out"]) - truth["x"]).max() / (LD(EPS64) * np.abs(truth["x"]).max()))
    if got.get("err") is not None:
        out["dE"] = float(abs(LD(got["err"]) - truth["err"]) / truth["err"])
    d = y[keep] - x[keep]
    e = psum((d * d).sum(axis=1))
    out["dOpt"] = float(abs(e - truth["e"]) / truth["e"])
    xc = s * (R @ truth["mu_p"]) + t  # (the truth maps mu_p onto mu_y exactly)
    out["dC"] = float(np.sqrt(((xc - truth["mu_y"]) ** 2).sum()) / extent)
    return out


def oracle_deviation(oracle, truth):
    """The yardstick: the fp64 oracle's find_alignment + err_compute on the same pairs."""
    p = np.asarray(truth["p"], dtype=np.float64)
    y = np.asarray(truth["y"], dtype=np.float64)
    keep = truth["keep"]
    al = oracle.find_alignment(p[keep], y[keep])
    e, _ = oracle.err_compute(p[keep], y[keep], al.s, al.R, al.t)
    _, new_p = oracle.err_compute(p, y, al.s, al.R, al.t)
    got = dict(s=al.s, R=np.array(al.R), t=np.array(al.t), scene_out=new_p, err=(al.err + e) / truth["K"])
    return deviation(got, truth)


def acceptance(engine, yard, rod=False, gap=None, lever=None):
    """The acceptance of the GPU tests, per metric: engine <= 8 max(oracle, floor).  On rods the
    rotation about the axis is determined only to rounding / gap, so dR is compared times the gap;
    that rotation moves a point by dR times its distance from the axis, so dX and dP are compared
    times gap / lever (truth_iteration's lever; never more than 1), and dOpt decides.  dC, where the
    transform puts the centroid, does not depend on R and is compared as it is: it is the check
    of t on rods.  -> (list of failures as text, dict metric -> engine / bound)"""
    fails, ratios = [], {}
    for k in METRICS:
        if k not in engine:
            continue
        w = 1.0
        if rod and k == "dR":
            w = float(gap)
        if rod and k in ("dX", "dP"):
            w = min(1.0, float(gap) / float(lever))
        bound = 8.0 * max(yard.get(k, 0.0) * w, FLOOR[k])
        ratios[k] = engine[k] * w / bound
        if not engine[k] * w <= bound:
            fails.append(f"{k}: engine {engine[k] * w:.3g} > 8 x max(oracle {yard.get(k, 0.0) * w:.3g}, floor {FLOOR[k]:.3g})")
    return fails, ratios


# ---- the named inputs ----------------------------------------------------------------------------

def rotation(angle_rad, axis=(1.0, 2.0, 3.0)):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle_rad) * K + (1 - np.cos(angle_rad)) * K @ K


PATCH_RATIOS = {"patch1e2": 1e2, "patch1e3": 1e3, "patch1e4": 1e4}
ROD_ASPECTS = {"rod0.05": 0.05, "rod1e-3": 1e-3}
FAR_NOMINAL = 5e4  # |centroid| / sigma of "far": what its coordinate sums carry around
CASES = ("plain", "far", "scaled_small", "scaled_big", "patch1e2", "patch1e3", "patch1e4", "rod0.05", "rod1e-3",
         "noisy")


def model_centre(m):
    """The engine's centring point c of a model (icp_set_model: its centroid); the first shifts
    of the one-pass moments were this point."""
    return np.asarray(m, dtype=np.float64).mean(axis=0)


def case(name, n, nm=None, gated=False, seed=0):
    """-> dict(m (nm, 3), p (n, 3), width, dmax (gated: 0.25 width, else None), rod (aspect or None)).

    The object A is nm uniform points (nm - 8 for a patch): a cube of width 2, for rod(a) a box of
    2 x 0.8a x 0.8a (relative eigenvalue gap of Horn's matrix 0.64 a^2).  The scene is A's first n
    points (past nm: further points of the same shape) turned about A's centroid and moved by 1%
    of its width, with noise of 2e-3 of the width on every point, so that the residual e* stays
    far above rounding and the relative metrics mean something at every iteration:
      plain     4 degree turn (the control)
      far       the same with extent 3, 5e4 from the origin on every axis
      scaled_*  plain times 1e-3; plain times 1e3 plus 7e4
      patchR    A plus 8 far points that put the model's centring point (its centroid) D = R sigma
                away from A (sigma: A's rms radius); 1 degree turn
      rodA      0.2 a radians of turn (the ends move less than the rod is thick), 1% of its
                thickness of shift, noise of a tenth of its thickness (the residual has to stay
                large against the rounding of the stored coordinates, |x| eps, or dE measures that
                rounding on two different clouds instead of the sums)
      noisy     plain with 10% of the scene points drawn afresh (pairs that fit nothing)
    gated: 5% of the scene becomes a clump two widths away, beyond dmax = 0.25 width from
    every model point, while no pair of A is farther apart than a tenth of dmax."""
    rng = np.random.default_rng([seed, n, nm or n, CASES.index(name), int(gated)])
    nm = n if nm is None else nm
    patch, rod = PATCH_RATIOS.get(name), ROD_ASPECTS.get(name)
    na = nm - 8 if patch else nm
    half = np.array([1.0, 1.0, 1.0])
    if rod:
        half = np.array([1.0, 0.4 * rod, 0.4 * rod])
    if name == "far":
        half = np.array([1.5, 1.5, 1.5])
    pts = rng.uniform(-1.0, 1.0, size=(max(n, na), 3)) * half
    width = 2.0 * half[0]
    fine = 2.0 * half[1]  # (the rod's thickness; the width otherwise)
    angle = 0.2 * rod if rod else np.deg2rad(1.0 if patch else 4.0)
    shift = 0.01 * fine * np.array([0.6, -0.64, 0.48])
    p = pts[:n] @ rotation(angle).T + shift + (0.1 if rod else 2e-3) * fine * rng.standard_normal((n, 3))
    if name == "noisy":
        k = n // 10
        p[rng.choice(n, k, replace=False)] = rng.uniform(-1.0, 1.0, size=(k, 3)) * half
    m = pts[:na]
    if gated:
        k = max(1, n // 20)
        p[rng.choice(n, k, replace=False)] = np.array([0.0, 2.0 * width, 0.0]) + 0.05 * width * rng.uniform(-1, 1, size=(k, 3))
    if patch:
        sigma = np.sqrt(((m - m.mean(0)) ** 2).sum(axis=1).mean())
        L = patch * sigma * nm / 8.0
        u = np.array([2.0, -3.0, 6.0]) / 7.0
        m = np.concatenate([m, u * L + rng.uniform(-1.0, 1.0, size=(8, 3))])
        m = m[rng.permutation(nm)]
    scale, offset = 1.0, np.zeros(3)
    if name == "far":
        offset = np.array([5e4, 5e4, 5e4])
    if name == "scaled_small":
        scale = 1e-3
    if name == "scaled_big":
        scale, offset = 1e3, np.array([7e4, 7e4, 7e4])
    m, p = m * scale + offset, p * scale + offset
    return dict(m=np.ascontiguousarray(m), p=np.ascontiguousarray(p), width=width * scale,
                dmax=0.25 * width * scale if gated else None, rod=rod)


def pairs_case(name, n, seed=0):
    """Pairs (p_j, y_j) given directly, for the find_alignment / err_compute operations: y is the
    case's model in the scene's order; 'noisy' shuffles the correspondences of 10% of the points."""
    c = case(name, n, seed=seed)
    y = c["m"].copy()
    if name == "noisy":
        rng = np.random.default_rng([seed, n, 77])
        j = rng.choice(n, n // 10, replace=False)
        y[j] = y[rng.permutation(j)]
    return c["p"], y, c["rod"]


def d_over_sigma(ref, y):
    """Distance of the point ref from the centroid of the matched points y, over their rms radius."""
    y = np.asarray(y, dtype=np.float64)
    mu = y.mean(axis=0)
    return float(np.linalg.norm(mu - ref) / np.sqrt(((y - mu) ** 2).sum(axis=1).mean()))
