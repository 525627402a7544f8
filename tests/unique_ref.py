"""The reference of the one-to-one ICP loop (icp_set_one_to_one), from the oracle's own pieces, and
the inputs of the one-to-one tests (tests/test_unique_ref.py on the CPU, tests/test_gpu_unique.py).

One iteration on the current scene p (all n points), with an optional gate (D = dmax * dmax, else
+inf) and an optional trim (T = trim_ref.trim_count(f, n), C = the T-th smallest d2 over ALL pairs):
  Y, idx = closest(p, m);  d2_i = (dx*dx + dy*dy) + dz*dz (gated_ref.d2_of)
  B_j = min{ d2_i : idx_i = j } (np.minimum.at);  keep_i = d2_i == B_{idx_i} and d2_i <= min(D, C)
  ties are kept whole; a NaN d2 never wins and is never kept
  K = #keep;  K < 4 (or T < 4): stop before the iteration changes anything ("few")
  Horn's closed form over the kept pairs (N = K); EVERY point moves;  err = (align.err + e) / K
A helper module, not a conftest: no fixtures, no hooks.
"""
import numpy as np

import gated_ref as G
import trim_ref as TR


def unique_mask(idx, d2, nm):
    """keep_i = d2_i == min{ d2_k : idx_k = idx_i }; NaN never wins, never kept."""
    best = np.full(nm, np.inf)
    ok = ~np.isnan(d2)
    np.minimum.at(best, idx[ok], d2[ok])
    return ok & (d2 == best[idx])


def unique_margin(idx, d2):
    """The smallest, over the model points chosen more than once, of (second-smallest d2 - B_j) /
    second-smallest d2 (inf when no model point is chosen twice; 0 at a tie)."""
    order = np.lexsort((d2, idx))
    i, d = idx[order], d2[order]
    first = np.flatnonzero(np.r_[True, i[1:] != i[:-1]])  # each group's smallest
    twice = first[np.r_[first[1:] - first[:-1] > 1, len(i) - first[-1] > 1]]
    if twice.size == 0:
        return np.inf
    second, b = d[twice + 1], d[twice]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(second > 0, (second - b) / second, 0.0)
    return float(rel.min())


def one_to_one_ref(oracle, m, p, max_iter, threshold=1e-5, dmax=0.0, f=None):
    """-> dict(new_p, K (list), err (array), mask (the last one evaluated), status ('ok' | 'few'),
    margin (unique_margin over the iterations; with a gate min |d2 - D| / D and with a trim
    (d2_(T+1) - C) / C folded in), s, R, t (the last completed iteration's), iterations, idx and Y of
    the last iteration evaluated; K_fail after 'few')."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64).copy()
    n, nm = p.shape[0], m.shape[0]
    D = np.float64(dmax) * np.float64(dmax) if dmax else np.float64(np.inf)
    T = TR.trim_count(f, n) if f is not None else None
    Ks, errs = [], []
    mask = np.zeros(n, dtype=bool)
    margin = np.inf
    s, R, t = 1.0, np.eye(3), np.zeros(3)
    idx = Y = None

    def out(status, **more):
        return dict(new_p=p, K=Ks, err=np.array(errs), mask=mask, status=status, margin=margin, s=s, R=R, t=t,
                    iterations=len(errs), idx=idx, Y=Y, T=T, **more)

    for _ in range(max_iter):
        Y, idx = oracle.closest(p, m)
        idx = np.asarray(idx).astype(np.int64)
        d2 = G.d2_of(p, Y)
        bound = D
        if T is not None:
            srt = np.sort(d2)
            C = srt[T - 1]
            bound = min(D, C)
            if T < n and C > 0:
                margin = min(margin, float((srt[T] - C) / C))
        with np.errstate(invalid="ignore"):
            keep = unique_mask(idx, d2, nm) & (d2 <= bound)
        mask = keep
        margin = min(margin, unique_margin(idx, d2))
        if np.isfinite(D):
            margin = min(margin, float(np.min(np.abs(d2 - D) / D)))
        K = int(keep.sum())
        if K < 4 or (T is not None and T < 4):
            return out("few", K_fail=K)
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
        errs.append(err)
        if err < threshold:
            break
    return out("ok")


# ---- inputs ---------------------------------------------------------------------------------
# The cases of tests/test_gpu_unique.py with this reference's own K lists; each is checked on the
# CPU by tests/test_unique_ref.py (margin > 1e-6, the K list) before the GPU tests rely on it.
SIZES_ITERS = 6  # synth(n, 100 + n, 0.25)
SIZES = {
    5: [4] * 6,
    63: [48] + [45] * 5,
    64: [47] + [48] * 5,
    65: [49] * 6,
    257: [178] + [193] * 5,
    4096: [2402, 2556, 2817, 3039, 3049, 3049],
    4097: [2385, 2531, 2789, 3027, 3040, 3040],
    9001: [4997, 5116, 5248, 5445, 5879, 6488],
}
PARTIAL_ITERS = 20  # gated_ref.cow_partial; K is constant from iteration 15
PARTIAL_K = [650, 693, 741, 788, 845, 881, 919, 954, 1008, 1055, 1107, 1147, 1251, 1368, 1443, 1451, 1451, 1451, 1451, 1451]
CLUMP_ITERS = 30  # gated_ref.cow_clump
CLUMP_K = [811, 824, 835, 877, 906, 933, 964, 1002, 1011, 1054, 1082, 1089, 1097, 1122, 1122, 1112, 1114, 1142, 1169,
           1227, 1269, 1313, 1377, 1445, 1494, 1536, 1579, 1593, 1606, 1647]
NOISY_ITERS = 8  # synth(n, 100 + n, 0.25, sigma=0.05), as trim_ref's noisy inputs
NOISY_DMAX, NOISY_F = 0.12, 0.7
# (n, "gate" | "trim" | "both") -> K per iteration (at 257 the gate binds under both, at 4097 the trim)
NOISY = {(257, "gate"): [118, 156, 165, 169, 168, 168, 167, 167],
         (4097, "gate"): [2138, 2161, 2209, 2242, 2260, 2250, 2285, 2305],
         (257, "trim"): [161, 170, 171, 172, 172, 172, 172, 172],
         (4097, "trim"): [2100, 2106, 2149, 2153, 2166, 2170, 2182, 2209],
         (257, "both"): [118, 156, 165, 169, 168, 168, 167, 167],
         (4097, "both"): [2100, 2106, 2149, 2153, 2166, 2170, 2182, 2209]}


def one_address():
    """4,097 scene points of which 4,090 lie nearest to corner 0 of an 8-point model (a cube's corners)
    and one nearest to each of the other seven: the contended scatter.  -> (m, p), K = 8."""
    r = np.random.default_rng(4097)
    m = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    p = np.concatenate([m[0] + r.uniform(-0.3, 0.3, size=(4090, 3)), m[1:] + r.uniform(-0.1, 0.1, size=(7, 3))])
    return m, p[r.permutation(p.shape[0])]


def few_case():
    """8 x 8 with every scene point nearest to one of three model points: K = 3 < 4.  -> (m, p)"""
    r = np.random.default_rng(8)
    m = np.concatenate([r.uniform(-1, 1, size=(3, 3)), 100.0 + r.uniform(-1, 1, size=(5, 3))])
    return m, r.uniform(-1, 1, size=(8, 3))


_cache = {}


def case(oracle, key):
    """The inputs of a named case -> (m, p, dmax (0: no gate), f (None: no trim), max_iter).
    key: ("size", n) | ("noisy", n, "gate" | "trim" | "both") | ("partial",) | ("clump",)"""
    if key[0] == "size":
        m, p = G.synth(key[1], 100 + key[1], 0.25)
        return m, p, 0.0, None, SIZES_ITERS
    if key[0] == "noisy":
        m, p = G.synth(key[1], 100 + key[1], 0.25, sigma=0.05)
        return (m, p, NOISY_DMAX if key[2] in ("gate", "both") else 0.0, NOISY_F if key[2] in ("trim", "both") else None,
                NOISY_ITERS)
    ref_, _tr1, tr2 = G.load_cow(oracle)
    if key[0] == "partial":
        m, p = G.cow_partial(ref_, tr2)
        return m, p, 0.0, None, PARTIAL_ITERS
    if key[0] == "clump":
        return ref_, G.cow_clump(ref_, tr2), 0.0, None, CLUMP_ITERS
    raise KeyError(key)


PLAIN = [("size", n) for n in SIZES] + [("partial",), ("clump",)]
MULTI = PLAIN + [("noisy", n, how) for n, how in NOISY]


def reference(oracle, key, iters=None):
    """The case's inputs and its reference, computed once a session and shared (never modified);
    iters: another iteration count (1: the exact first iteration) -> (m, p, dmax, f, max_iter, ref)"""
    ck = (key, iters)
    if ck not in _cache:
        m, p, dmax, f, max_iter = case(oracle, key)
        if iters is not None:
            max_iter = iters
        _cache[ck] = (m, p, dmax, f, max_iter, one_to_one_ref(oracle, m, p, max_iter, -1.0, dmax, f))
    return _cache[ck]
