"""The host Horn step (icp_horn_solve: the code the device runs, icp_horn.h) against the
extended-precision truth of tests/align_ref.py, on prescribed spectra of Horn's 4x4 on both sides
of the polynomial eigen path's hand-over to Jacobi (P'(l) <= 1e-3 |N|^3), and on the two rod
clouds the GPU tests use as their handle on the two branches.  No GPU.

The rotation's inherent sensitivity is rounding / gap (gap: (l1 - l2) / max |l|), so |dR| gap is
the conditioning-free figure.  Below gap 1e-4 the polynomial path cannot be taken
(P' <= 4 gap |N|^3) and the oracle's Jacobi is the yardstick; from 1e-4 on |dR| <= 2.5e-10, a
quarter of the documented 1e-9 parity of R, the rest left to the moments."""
import numpy as np
import pytest

import align_ref as A

LD = A.LD
GAPS = 10.0 ** (-0.25 * np.arange(2, 33))  # 10^-0.5 ... 10^-8 in quarter decades
SCALES = 10.0 ** np.arange(-6, 7, 2)
KINDS = ("spread", "clustered", "opposite")
BASES = 4  # random bases per (gap, kind, scale): 31 x 3 x 7 x 4 = 2,604 spectra


def spectrum(kind, g, rng):
    """Traceless (l1 = 1, l2, l3, l4) with relative gap ~ g: the rest (a) spread, (b) clustered
    under the top, (c) both near -l1, which maximises P'(l1) at a given gap."""
    if kind == "spread":
        u = rng.uniform(0.2, 0.8)
        g1 = g * max(1.0, 2.0 * max(u, 1.0 - u))
        return [1.0, 1.0 - g1, -(2.0 - g1) * u, -(2.0 - g1) * (1.0 - u)]
    if kind == "clustered":
        g1 = 3.0 * g
        l3 = 1.0 - g1 * (1.0 + rng.uniform(1.0, 3.0))
        return [1.0, 1.0 - g1, l3, -(2.0 - g1 + l3)]
    d = rng.uniform(0.0, 0.01)
    return [1.0, 1.0 - g, -(2.0 - g) / 2.0 * (1.0 + d), -(2.0 - g) / 2.0 * (1.0 - d)]


@pytest.fixture(scope="module")
def sweep(icp_lib, oracle):
    """Every spectrum once: S in fp64 (the map S <-> N is a bijection), the truth of that S, the
    host solver's and the oracle's rotation."""
    rng = np.random.default_rng(20240607)
    Ss, meta = [], []
    for g in GAPS:
        for kind in KINDS:
            for scale in SCALES:
                for _ in range(BASES):
                    lam = np.array(spectrum(kind, g, rng), dtype=LD)
                    Q = A._ld(np.linalg.qr(rng.standard_normal((4, 4)))[0])
                    N = (Q * lam) @ Q.T
                    N = (N + N.T) / LD(2)
                    N -= np.trace(N) / LD(4) * np.eye(4, dtype=LD)
                    Ss.append(np.asarray(A.horn_matrix_inverse(N) * LD(scale), dtype=np.float64))
                    meta.append((kind, scale))
    S = np.array(Ss)
    q, lam1, gap, dpoly = A.top_eigen(A.horn_matrix(A._ld(S)))
    Rt = A.rot_from_quat(q)
    N64 = A.horn_matrix(S)
    rows = []
    for j in range(S.shape[0]):
        l1 = float(lam1[j])
        d_caps = sp = 1.05 * l1  # (d_caps + sp) / 2 >= l1, as for real moments; s = 1
        s, R, _t = icp_lib.horn_solve(S[j], np.zeros(3), np.zeros(3), d_caps, sp)
        ev, V = oracle.eig_sym4(N64[j])
        Ro = A.rot_from_quat(V[:, int(np.argmax(ev))])
        Rl = A._ld(R)
        obj = (Rl * A._ld(S[j]).T).sum()  # sum y'.R p' = sum_ij R_ij S_ji
        e_opt = LD(d_caps) + LD(sp) - 2 * lam1[j]
        rows.append(dict(kind=meta[j][0], scale=meta[j][1], gap=float(gap[j]), dpoly=float(dpoly[j]), s=s,
                         dR=float(np.abs(Rl - Rt[j]).max()), dR_oracle=float(np.abs(Ro - Rt[j]).max()),
                         orth=float(np.abs(Rl @ Rl.T - np.eye(3)).max()),
                         det=float(abs(np.linalg.det(R) - 1.0)),
                         dOpt=float(abs(2 * (lam1[j] - obj)) / e_opt)))
    return rows


def test_sweep_covers_both_branches(sweep):
    assert len(sweep) >= 2000
    poly = [r for r in sweep if r["dpoly"] > A.HANDOVER]
    jac = [r for r in sweep if r["dpoly"] <= A.HANDOVER]
    near = [r for r in poly if r["dpoly"] <= 10 * A.HANDOVER]
    assert len(poly) > 500 and len(jac) > 500 and len(near) > 100
    assert all(r["dpoly"] <= 4.0 * r["gap"] * (1 + 1e-9) for r in sweep)  # P' <= 4 gap |N|^3
    for name, rows in (("polynomial", poly), ("polynomial, within 10x of the hand-over", near), ("Jacobi", jac)):
        print(f"{name}: {len(rows)} spectra, worst |dR| gap {max(r['dR'] * r['gap'] for r in rows):.3g}, "
              f"worst |dR| {max(r['dR'] for r in rows):.3g}; oracle's Jacobi on the same: "
              f"|dR| gap {max(r['dR_oracle'] * r['gap'] for r in rows):.3g}")


def test_below_the_handover_matches_the_oracles_jacobi(sweep):
    rows = [r for r in sweep if r["gap"] < 1e-4]
    assert len(rows) > 800 and all(r["dpoly"] <= A.HANDOVER for r in rows)
    yard = max(r["dR_oracle"] * r["gap"] for r in rows)
    worst = max(rows, key=lambda r: r["dR"] * r["gap"])
    print("gap < 1e-4: host |dR| gap", worst["dR"] * worst["gap"], "oracle's worst", yard, worst)
    assert worst["dR"] * worst["gap"] <= 8.0 * yard


def test_at_and_above_the_handover_R_is_within_a_quarter_of_its_parity(sweep):
    rows = [r for r in sweep if r["gap"] >= 1e-4]
    assert len(rows) > 800
    worst = max(rows, key=lambda r: r["dR"])
    print("gap >= 1e-4: worst |dR|", worst)
    assert worst["dR"] <= 2.5e-10


def test_rotation_is_a_rotation_and_optimal_everywhere(sweep):
    for key, bound in (("orth", 1e-13), ("det", 1e-13), ("dOpt", 1e-12)):
        worst = max(sweep, key=lambda r: r[key])
        print(key, worst[key], worst["kind"], worst["gap"], worst["scale"])
        assert worst[key] <= bound, (key, worst)
    assert all(abs(r["s"] - 1.0) <= 4 * A.EPS64 for r in sweep)


@pytest.mark.parametrize("n", [1000, 4097])
def test_rods_sit_on_both_branches(icp_lib, oracle, n):
    """rod(0.05): on the polynomial side, within [1, 10] x the hand-over constant; rod(1e-3): a
    decade below it (Jacobi).  The host step on their moments meets the sweep's bounds."""
    for name, lo, hi in (("rod0.05", A.HANDOVER, 10 * A.HANDOVER), ("rod1e-3", 0.0, 1e-4)):
        c = A.case(name, n)
        Y, _ = oracle.closest(c["p"], c["m"])
        tr = A.truth_iteration(c["p"], Y)
        f = lambda v: np.asarray(v, dtype=np.float64)
        s, R, t = icp_lib.horn_solve(f(tr["S"]), f(tr["mu_p"]), f(tr["mu_y"]), float(tr["d_caps"]), float(tr["sp"]))
        dev = A.deviation(dict(s=s, R=R, t=t), tr)
        yard = A.oracle_deviation(oracle, tr)
        print(name, n, "gap", float(tr["gap"]), "P'/|N|^3", float(tr["dpoly"]), dev, "oracle", yard)
        assert lo < tr["dpoly"] <= hi if lo else tr["dpoly"] < hi
        assert 0.3 * c["rod"] ** 2 <= tr["gap"] <= 1.2 * c["rod"] ** 2
        assert dev["dR"] <= 2.5e-10 and dev["dOpt"] <= 1e-12
        assert A.acceptance(dev, yard, rod=True, gap=tr["gap"], lever=tr["lever"])[0] == []
