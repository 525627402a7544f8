"""The reference of the model's k nearest neighbours and of the normals estimated from them
(icp_model_knn, icp_estimate_model_normals; icp_normals.hip), restated in numpy, and the inputs of
their tests (tests/test_normals_ref.py on the CPU, tests/test_gpu_normals.py).

For model point j (include/icp_capi.h, steps 1 to 4):
  1. d = m_j - m_i, d2 = (dx*dx + dy*dy) + dz*dz; N_j = the first k indices in ascending (d2, i)
     order: a stable sort by d2 is that order
  2. mu = (sum m_i) / k and C = sum (m_i - mu)(m_i - mu)^T, both summed in the order of N_j
  3. l0 <= l1 <= l2 the eigenvalues of C: !(l2 > 0) or l1 - l0 <= 1e-12 l2 -> the zero normal
     ("degenerate"), else the unit eigenvector of l0
  4. sign: n . (v - m_j) >= 0 with a viewpoint v, else the component of largest magnitude positive
dtype = np.float64 restates the engine's arithmetic (numpy.linalg.eigh); dtype = np.longdouble is the
extended-precision truth (the neighbour lists stay the fp64 ones; the eigen-solve is cyclic Jacobi,
numpy having no eigh for longdouble).
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import plane_ref as P

GAP_MIN = 1e-12    # step 3's condition
GAP_CLEAR = 1e-3   # the GPU tests compare directions where the gap ratio is at least this
SIGN_CLEAR = 1e-6  # ... and signs where the sign rule's margin is at least this
VIEW = (0.0, 0.0, 10.0)


def knn(m, k, chunk=512):
    """-> (idx (n, k) int32, d2 (n, k) float64, tie (n,) bool: the k-th and the (k+1)-th distance are equal)"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    n = m.shape[0]
    idx = np.empty((n, k), dtype=np.int32)
    d2k = np.empty((n, k))
    tie = np.zeros(n, dtype=bool)
    for b in range(0, n, chunk):
        q = m[b:b + chunk]
        dx = q[:, None, 0] - m[None, :, 0]
        dy = q[:, None, 1] - m[None, :, 1]
        dz = q[:, None, 2] - m[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        order = np.argsort(d2, axis=1, kind="stable")
        srt = np.take_along_axis(d2, order, axis=1)
        idx[b:b + chunk] = order[:, :k]
        d2k[b:b + chunk] = srt[:, :k]
        if k < n:
            tie[b:b + chunk] = srt[:, k - 1] == srt[:, k]
    return idx, d2k, tie


def _jacobi(a00, a01, a02, a11, a12, a22, sweeps=12):
    """Cyclic Jacobi on n symmetric 3 x 3 matrices in the arrays' dtype -> (w (n, 3), V (n, 3, 3)), unsorted."""
    dt = a00.dtype
    n = a00.shape[0]
    A = np.zeros((n, 3, 3), dtype=dt)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2] = a00, a01, a02, a11, a12, a22
    A[:, 1, 0], A[:, 2, 0], A[:, 2, 1] = a01, a02, a12
    V = np.zeros((n, 3, 3), dtype=dt)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1
    one = dt.type(1)
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[:, p, q]
            live = apq != 0
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (A[:, q, q] - A[:, p, p]) / (2 * apq)
                t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            t = np.where(live, t, 0)
            c = one / np.sqrt(t * t + one)
            s = t * c
            G = np.zeros((n, 3, 3), dtype=dt)
            G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1
            G[:, p, p], G[:, q, q], G[:, p, q], G[:, q, p] = c, c, s, -s
            A = np.einsum("nji,njk,nkl->nil", G, A, G)
            V = np.einsum("nij,njk->nik", V, G)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def normals_ref(m, k, viewpoint=None, dtype=np.float64):
    """-> dict(idx, d2, tie, normals (n, 3), gap ((l1 - l0) / l2; 0 where l2 is not > 0), zero (bool:
    the degenerate points), degenerate (their count), sign_margin (n,))"""
    m64 = np.ascontiguousarray(m, dtype=np.float64)
    idx, d2, tie = knn(m64, k)
    mx = m64.astype(dtype)
    nb = mx[idx]  # (n, k, 3) in list order
    s = np.zeros((mx.shape[0], 3), dtype=dtype)
    for i in range(k):
        s = s + nb[:, i]
    mu = s / dtype(k)
    C = np.zeros((mx.shape[0], 3, 3), dtype=dtype)
    for i in range(k):
        d = nb[:, i] - mu
        C = C + d[:, :, None] * d[:, None, :]
    if dtype is np.float64:
        w, V = np.linalg.eigh(C)
    else:
        w, V = _jacobi(C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2])
        order = np.argsort(w, axis=1, kind="stable")
        w = np.take_along_axis(w, order, axis=1)
        V = np.take_along_axis(V, order[:, None, :], axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        zero = ~(w[:, 2] > 0) | (w[:, 1] - w[:, 0] <= dtype(GAP_MIN) * w[:, 2])
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0)
    nrm = V[:, :, 0].copy()
    nrm = nrm / np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])[:, None]
    if viewpoint is not None:
        wv = np.asarray(viewpoint, dtype=np.float64).astype(dtype)[None, :] - mx
        dot = (nrm[:, 0] * wv[:, 0] + nrm[:, 1] * wv[:, 1]) + nrm[:, 2] * wv[:, 2]
        flip = dot < 0
        margin = np.abs(dot) / np.sqrt((wv * wv).sum(axis=1))
    else:
        a = np.abs(nrm)
        big = np.argmax(a, axis=1)  # (the first maximum: ties go to the lowest axis)
        flip = np.take_along_axis(nrm, big[:, None], axis=1)[:, 0] < 0
        srt = np.sort(a, axis=1)
        margin = srt[:, 2] - srt[:, 1]
    nrm = np.where(flip[:, None], -nrm, nrm)
    nrm[zero] = 0
    return dict(idx=idx, d2=d2, tie=tie, normals=nrm, gap=np.asarray(gap, dtype=np.float64), zero=zero,
                degenerate=int(zero.sum()), sign_margin=np.asarray(margin, dtype=np.float64))


# ---- inputs ---------------------------------------------------------------------------------

ELLIPSOIDS = (16, 17, 63, 64, 65, 257)  # P.ellipsoid(n, 100 + n), k = 16
KS_AT_257 = (3, 8, 30, 64)


def lattice():
    g = np.arange(9, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def far_points():
    return np.concatenate([P.ellipsoid(4089, 77)[0], np.array([40.0, 0.0, 0.0]) + 0.1 * P.ellipsoid(8, 78)[0]])


def line():
    return np.outer(np.linspace(-1, 1, 64), np.array([1.0, 2.0, -0.5]))


def duplicates():
    m = P.ellipsoid(257, 357)[0]
    return np.concatenate([m, m[:40]])


def equal_points():
    return np.tile(np.array([0.3, -0.2, 0.7]), (32, 1))


def model(name, load=None):
    """The named input -> (m, k).  "cow" needs load (a cloud's loader)."""
    if name.startswith("ell"):  # "ell<n>" or "ell257k<k>"
        n, _, k = name[3:].partition("k")
        n = int(n)
        seed = {4097: 4197, 9001: 9101}.get(n, 100 + n)
        return P.ellipsoid(n, seed)[0], int(k) if k else 16
    if name == "cow":
        import datasets
        return load(datasets.path("cow_ref")), 16
    make = {"lattice": lattice, "far": far_points, "line": line, "duplicates": duplicates, "equal": equal_points,
            "planar": lambda: P.planar()[0]}[name]
    return make(), 8 if name == "line" else 16


# every input of the k-NN test; the normals' tests use those of NORMAL_CASES
KNN_CASES = tuple("ell%d" % n for n in ELLIPSOIDS + (4097, 9001)) + tuple("ell257k%d" % k for k in KS_AT_257) + \
    ("ell64k64", "cow", "lattice", "duplicates", "equal", "far", "planar", "line")
# the inputs whose directions are compared (the gap-ratio table of the issue)
CLEAR_CASES = tuple("ell%d" % n for n in ELLIPSOIDS + (4097, 9001)) + ("cow", "lattice", "planar", "far")

_cache = {}


def reference(name, load=None, viewpoint=None, dtype=np.float64):
    """The reference of a named input, computed once a session and shared (never modified)
    -> (m, k, normals_ref(...))"""
    ck = (name, viewpoint, dtype)
    if ck not in _cache:
        m, k = model(name, load)
        _cache[ck] = (m, k, normals_ref(m, k, viewpoint, dtype))
    return _cache[ck]
