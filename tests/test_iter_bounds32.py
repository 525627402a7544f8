"""The fused grid iteration's bounds that keep one fp64 root a batch (icp_grid.hip
nn_grid_iter2_kernel, CPU restatement in exact rational arithmetic).

A walk has the seed distance wb and takes s0 = fl(sqrt(wb)) once.  Its radius is rw = fl(s0 + skin)
(rw = s0 without the skin), and it must scan every model point with D64 <= ew = fl(rw rw).  ew is
never formed; three values are derived from rw instead of three more roots of ew:

  rb = fl(rw (1 + 2^-51))        the radius of the cell box (complete_box_r) and of the sphere prune
                                 (rcf): at least sqrt(ew), so both keep every point within ew;
  u0 = fl(rw (1 - 2^-40))        the bound on every point the walk did not scan (D64 > ew): at most
                                 its true distance;
  lower(a) = fl(fl(sqrtf(a)) (1 - 2^-20)) - sqrt(3) eq (1 + 2^-20)
                                 the bound from a list value a (a computed fp32 d32, or a D64 rounded
                                 down to fp32), its root by v_sqrt_f32: at most the true distance;

and the certificate's pair test bounds the pair's loser by

  lb = fl(sqrtf(rd32(D64)) (1 - 2^-21))                             at most its true distance.

The hardware's fp32 root is taken two ulps off the correctly rounded one in the adverse direction
(high: each of these is a lower bound).  Every claim has a negative control: the same check with
the room removed fails.  Boxes at 0, 1e3 and +-5e4 from the origin, extents from 2e-6 to 1e5.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_iter_prune import (F, SQRT3, adversarial_cases, cell1, d32, d64, em32, exact_d2, k_seed, sqrtf_low)

CASES = [(0.0, 2.0), (1e3, 2.0), (5e4, 3.0), (-5e4, 10.0), (7.0, 1e5), (0.0, 2e-6), (1e3, 2e-6)]


def sqrtf_high(x):
    """sqrtf, then two ulps up (v_sqrt_f32 is within an ulp or two of the rounded root)."""
    r = np.sqrt(F(x))
    return np.nextafter(np.nextafter(r, F(np.inf)), F(np.inf))


def f32_rd(x):
    """__double2float_rd: the largest float32 <= x."""
    f = F(x)
    return F(np.nextafter(f, F(-np.inf))) if float(f) > x else f


def radii(wb, skin, room=1.0):
    """(rw, rb, u0) of a walk as the kernel forms them."""
    s0 = math.sqrt(wb)
    rw = s0 + skin if skin else s0
    rb = rw * (1.0 + 2.0 ** -51 * room) if skin else s0
    u0 = rw * (1.0 - 2.0 ** -40 * room)
    return rw, rb, u0


def walks(centre, extent, n=400):
    """(wb, skin): seed distances from 1e-7 of the extent to the extent, skins of a cell's fraction."""
    rng = np.random.default_rng(k_seed(centre) + int(extent * 1e6) % 997)
    for _ in range(n):
        wb = (extent * 10.0 ** rng.uniform(-7, 0)) ** 2
        skin = extent / 64.0 * 10.0 ** rng.uniform(-3, 0)
        yield wb, skin


# ---- rb: the box's and the prune's radius -------------------------------------------------------
@pytest.mark.parametrize("centre,extent", CASES)
def test_box_radius_covers_the_scanned_square(centre, extent):
    for wb, skin in walks(centre, extent):
        rw, rb, _ = radii(wb, skin)
        ew = rw * rw
        assert Fraction(rb) ** 2 >= Fraction(ew)
        assert rb >= math.sqrt(ew)  # (the value complete_box(ew) took: the box only grows)
        rw0, rb0, _ = radii(wb, 0.0)  # (the seed alone: the root itself, the parent's radius)
        assert rb0 == rw0 == math.sqrt(wb)


def test_box_radius_negative_control():
    """Without the 2^-51, rw itself falls below sqrt(fl(rw rw)) whenever the square rounds up."""
    bad = 0
    for wb, skin in walks(1e3, 2.0):
        rw, rb, _ = radii(wb, skin, room=0.0)
        bad += Fraction(rb) ** 2 < Fraction(rw * rw)
    assert bad > 0


def complete_box_r(q, R, lo, inv_h, g):
    c0, c1 = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        s = (abs(q[a]) + R) * 2.0 ** -44
        c0[a] = cell1(q[a] - (R + s), lo[a], inv_h, g[a])
        c1[a] = cell1(q[a] + (R + s), lo[a], inv_h, g[a])
    return c0, c1


def prune_rows_r(q, rb, lo, inv_h, c0, c1):
    """test_iter_prune.prune_rows with the radius given (rcf from rb, not from a root of ew)."""
    tr = [F((q[a] - lo[a]) * inv_h - float(c0[a])) for a in range(3)]
    rcf = F(rb * inv_h * (1.0 + 2.0 ** -18) +
            2.0 ** -20 * (1.0 + abs(float(tr[0])) + abs(float(tr[1])) + abs(float(tr[2]))))
    rc2 = F(rcf * rcf)
    xroom = F(F(2.0 ** -20) * F(F(1.0) + abs(tr[0])))
    xspan = F(c1[0] - c0[0] + 1)
    ny, nz = c1[1] - c0[1] + 1, c1[2] - c0[2] + 1
    inv_ny = F(F(1.0) / F(ny))
    rows = {}
    for r in range(ny * nz):
        rz = int(F(F(F(r) + F(0.5)) * inv_ny))
        ry = r - rz * ny
        dy = max(F(0.0), max(F(F(ry) - tr[1]), F(tr[1] - F(ry + 1))))
        dz = max(F(0.0), max(F(F(rz) - tr[2]), F(tr[2] - F(rz + 1))))
        rem = F(F(rc2 - F(dy * dy)) - F(dz * dz))
        if rem < F(0.0):
            continue
        xw = F(F(sqrtf_low(rem) * F(1.0 + 2.0 ** -20)) + xroom)
        x0 = max(c0[0], c0[0] + int(math.floor(max(F(tr[0] - xw), F(-1.0)))))
        x1 = min(c1[0], c0[0] + int(math.floor(min(F(tr[0] + xw), xspan))))
        if x0 <= x1:
            rows[(ry, rz)] = (x0, x1)
    return rows


@pytest.mark.parametrize("centre,extent,gx", [(0.0, 2.0, 80), (1e3, 2.0, 64), (-5e4, 10.0, 200), (5e4, 3.0, 97),
                                              (7.0, 1e5, 4096), (0.0, 2e-6, 16)])
def test_walk_with_the_kept_radius_scans_every_point_within_it(centre, extent, gx):
    """The walk as the kernel now runs it: s0 = fl(sqrt(seed distance)), rw = s0 + skin, the box and
    the prune from rb.  Points on and one ulp inside the sphere of squared radius ew = fl(rw rw)."""
    missed = checked = 0
    for q, pts, ew_target, lo, inv_h, g in adversarial_cases(centre, extent, gx, seed=gx + 7 + k_seed(centre), n_q=25):
        # a seed distance and a skin whose walk radius is the case's sphere: rw = sqrt(ew_target)
        rw_t = math.sqrt(ew_target)
        for frac in (0.0, 0.3):
            skin = frac * rw_t
            wb = (rw_t - skin) ** 2
            rw, rb, _ = radii(wb, skin)
            ew = rw * rw
            c0, c1 = complete_box_r(q, rb, lo, inv_h, g)
            rows = prune_rows_r(q, rb, lo, inv_h, c0, c1)
            for m in pts[d64(q, pts) <= ew]:
                c = [cell1(m[a], lo[a], inv_h, g[a]) for a in range(3)]
                run = rows.get((c[1] - c0[1], c[2] - c0[2]))
                checked += 1
                if not all(c0[a] <= c[a] <= c1[a] for a in range(3)) or run is None or not run[0] <= c[0] <= run[1]:
                    missed += 1
    assert checked > 0 and missed == 0


# ---- u0: the points the walk did not scan --------------------------------------------------------
def unscanned_floor2(ew):
    """A point the walk did not scan has D64 > ew, and D64 <= |v|^2 (1 + 2^-50) (three roundings of
    2^-53 on non-negative terms, generously): |v|^2 >= this."""
    return Fraction(np.nextafter(ew, np.inf)) / (1 + Fraction(1, 2 ** 50))


@pytest.mark.parametrize("centre,extent", CASES)
def test_unscanned_bound_is_below_every_unscanned_point(centre, extent):
    for wb, skin in walks(centre, extent):
        for sk in (skin, 0.0):
            rw, _, u0 = radii(wb, sk)
            assert Fraction(u0) ** 2 <= unscanned_floor2(rw * rw)


def test_unscanned_bound_negative_control():
    bad = 0
    for wb, skin in walks(0.0, 2.0):
        rw, _, u0 = radii(wb, skin, room=0.0)
        bad += Fraction(u0) ** 2 > unscanned_floor2(rw * rw)
    assert bad > 0


# ---- lower(a): the lists' bounds with the fp32 root ---------------------------------------------
def lower32(a, eq, room=1.0):
    return float(sqrtf_high(a)) * (1.0 - 2.0 ** -20 * room) - SQRT3 * eq * (1.0 + 2.0 ** -20) * room


def below(b, d2):
    return b <= 0.0 or Fraction(b) ** 2 <= d2


def pairs(centre, extent, n=300):
    """(q, m, eq): a query in or just outside the box, a model point 1e-7 .. 1e-1 extents away."""
    rng = np.random.default_rng(int(abs(centre) + extent * 1e6) % 9973)
    lo = [centre - extent / 2] * 3
    hi = [centre + extent / 2] * 3
    c = [l + 0.5 * (h - l) for l, h in zip(lo, hi)]
    em = em32(lo, hi)
    for _ in range(n):
        q = rng.uniform(np.array(lo) - 0.1 * extent, np.array(hi) + 0.1 * extent)
        r = extent * 10.0 ** rng.uniform(-7, -1)
        m = np.clip(q + r * rng.normal(size=3) / math.sqrt(3), lo, hi)
        eq = math.ldexp(max(abs(q[a] - c[a]) for a in range(3)), -23) + em
        yield q, m, eq, c


@pytest.mark.parametrize("centre,extent", CASES)
def test_list_bounds_with_the_fp32_root_are_below_the_true_distance(centre, extent):
    worst = 0.0
    for q, m, eq, c in pairs(centre, extent):
        true2 = exact_d2(q, m)
        for a in (d32(q, m, c), max(f32_rd(float(d64(q, m))), F(0))):  # (a screen value; a D64 rounded down)
            b = lower32(a, eq)
            assert below(b, true2), (q, m, a, eq)
            if b > 0:
                worst = max(worst, b / math.sqrt(float(true2)))
    assert worst < 1.0


def test_list_bounds_negative_control():
    """Without the 2^-20 and the screen's error term, a root two ulps high exceeds the distance."""
    bad = 0
    for q, m, eq, c in pairs(1e3, 2.0):
        a = max(f32_rd(float(d64(q, m))), F(0))
        bad += not below(lower32(a, eq, room=0.0), exact_d2(q, m))
    assert bad > 0


# ---- lb: the pair's loser -----------------------------------------------------------------------
def loser_bound(x, room=1.0):
    return float(sqrtf_high(f32_rd(x))) * (1.0 - 2.0 ** -21 * room)


@pytest.mark.parametrize("centre,extent", CASES)
def test_pair_loser_bound_is_below_its_true_distance(centre, extent):
    worst = 0.0
    for q, m, _, _ in pairs(centre, extent):
        true2 = exact_d2(q, m)
        b = loser_bound(float(d64(q, m)))
        assert below(b, true2), (q, m)
        worst = max(worst, b / math.sqrt(float(true2)))
    assert 0.999 < worst < 1.0  # (and it costs under 2^-20 of the distance)


def test_pair_loser_bound_negative_control():
    bad = 0
    for q, m, _, _ in pairs(-5e4, 10.0):
        bad += not below(loser_bound(float(d64(q, m)), room=0.0), exact_d2(q, m))
    assert bad > 0
