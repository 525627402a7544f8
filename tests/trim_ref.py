"""The reference of the trimmed ICP loop (icp_set_trim), from the oracle's own pieces, and the
inputs of the trimmed tests (tests/test_trim_ref.py on the CPU, tests/test_gpu_trim.py).

One trimmed iteration on the current scene p (all n points), T = max(1, int(f * n)) with the
product in fp64, D = dmax * dmax or +inf without a gate:
  Y = closest(p, m);  d2_j = (dx*dx + dy*dy) + dz*dz (gated_ref.d2_of)
  C = the T-th smallest d2 (np.sort);  keep_j = d2_j <= min(D, C): ties at C are all kept
  K = #keep;  T < 4 or K < 4: stop before the iteration changes anything ("few")
  Horn's closed form over the kept pairs (N = K); EVERY point moves;  err = (align.err + e) / K
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import gated_ref as G


def trim_count(f, n):
    """PCL's rule: the product in fp64 as written, truncated; at least 1."""
    return max(1, int(np.float64(f) * np.float64(n)))


def trimmed_ref(oracle, m, p, f, dmax, max_iter, threshold=1e-5):
    """-> dict(new_p, K (list), C (list), err (array), mask (last cut evaluated), status ('ok' | 'few'),
    margin (the smaller of (d2_(T+1) - C) / C over the iterations and, with a gate, gated_ref's
    |d2 - D| / D), T, s, R, t (the last completed iteration's), iterations; K_fail after 'few')."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64).copy()
    n = p.shape[0]
    T = trim_count(f, n)
    D = np.float64(dmax) * np.float64(dmax) if dmax else np.float64(np.inf)
    Ks, Cs, errs = [], [], []
    mask = np.zeros(n, dtype=bool)
    margin = np.inf
    s, R, t = 1.0, np.eye(3), np.zeros(3)

    def out(status, **more):
        return dict(new_p=p, K=Ks, C=Cs, err=np.array(errs), mask=mask, status=status, margin=margin, T=T, s=s, R=R,
                    t=t, iterations=len(errs), **more)

    for _ in range(max_iter):
        Y, _idx = oracle.closest(p, m)
        d2 = G.d2_of(p, Y)
        srt = np.sort(d2)
        C = srt[T - 1]
        with np.errstate(invalid="ignore"):
            keep = d2 <= min(D, C)
        mask = keep
        if T < n and C > 0:
            margin = min(margin, float((srt[T] - C) / C))
        if np.isfinite(D):
            margin = min(margin, float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        if T < 4 or K < 4:
            return out("few", K_fail=K, C_fail=C)
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
        Ks.append(K)
        Cs.append(float(C))
        errs.append(err)
        if err < threshold:
            break
    return out("ok")


def key_of(v):
    """The selection's 64-bit keys of doubles (uint64): the sign bit flipped for non-negatives,
    every bit flipped for negatives, every NaN all ones -- unsigned order = -inf < .. < -0 < +0 < .. < +inf < NaN."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    u = v.view(np.uint64)
    sign = np.uint64(1) << np.uint64(63)
    k = np.where(u & sign, ~u, u | sign)
    return np.where(np.isnan(v), np.uint64(0xFFFFFFFFFFFFFFFF), k).astype(np.uint64)


# ---- inputs ---------------------------------------------------------------------------------
# The cases of tests/test_gpu_trim.py with the reference K the issue quotes; each is checked on the
# CPU by tests/test_trim_ref.py (margin > 1e-6, the K list) before the GPU tests rely on it.
SIZES = {63: 44, 64: 44, 65: 45, 257: 179, 4096: 2867, 4097: 2867, 9001: 6300}  # n -> K, every iteration
SIZES_F, SIZES_ITERS = 0.7, 6  # synth(n, 100 + n, 0.25); n = 5 stops "few" at iteration 0 (T = 3)
NOISY = {(257, 0.5): 128, (4097, 0.5): 2048, (4097, 0.9): 3687}  # (n, f) -> K, every iteration
NOISY_ITERS = 8  # synth(n, 100 + n, 0.25, sigma=0.05)
BOTH_N, BOTH_F, BOTH_DMAX = 4097, 0.7, 0.10  # the gate binds first, then the trim
BOTH_K = [2776, 2790, 2817, 2858, 2867, 2867, 2867, 2867]
PARTIAL_F, PARTIAL_K, PARTIAL_ITERS = 0.6, 1306, 20
CLUMP_F, CLUMP_K, CLUMP_ITERS = 0.75, 2177, 17

_cache = {}


def case(oracle, key):
    """The inputs of a named case -> (m, p, f, dmax (0: no gate), max_iter, threshold).
    key: ("size", n) | ("noisy", n, f) | ("both",) | ("partial",) | ("clump",) | ("clump_gate",)"""
    if key[0] == "size":
        m, p = G.synth(key[1], 100 + key[1], 0.25)
        return m, p, SIZES_F, 0.0, SIZES_ITERS, -1.0
    if key[0] == "noisy":
        m, p = G.synth(key[1], 100 + key[1], 0.25, sigma=0.05)
        return m, p, key[2], 0.0, NOISY_ITERS, -1.0
    if key[0] == "both":
        m, p = G.synth(BOTH_N, 100 + BOTH_N, 0.25, sigma=0.05)
        return m, p, BOTH_F, BOTH_DMAX, NOISY_ITERS, -1.0
    ref_, _tr1, tr2 = G.load_cow(oracle)
    if key[0] == "partial":
        m, p = G.cow_partial(ref_, tr2)
        return m, p, PARTIAL_F, 0.0, PARTIAL_ITERS, -1.0
    if key[0] == "clump":
        return ref_, G.cow_clump(ref_, tr2), CLUMP_F, 0.0, 30, 1e-5
    if key[0] == "clump_gate":
        return ref_, G.cow_clump(ref_, tr2), CLUMP_F, 0.25 * G.cow_ext(ref_), 30, 1e-5
    raise KeyError(key)


MULTI = ([("size", n) for n in SIZES] + [("noisy", n, f) for n, f in NOISY] +
         [("both",), ("partial",), ("clump",), ("clump_gate",)])


def reference(oracle, key, iters=None):
    """The case's inputs and its reference, computed once a session and shared (never modified);
    iters: another iteration count (1: the exact first iteration) -> (m, p, f, dmax, max_iter, threshold, ref)"""
    ck = (key, iters)
    if ck not in _cache:
        m, p, f, dmax, max_iter, threshold = case(oracle, key)
        if iters is not None:
            max_iter, threshold = iters, -1.0
        _cache[ck] = (m, p, f, dmax, max_iter, threshold, trimmed_ref(oracle, m, p, f, dmax, max_iter, threshold))
    return _cache[ck]
