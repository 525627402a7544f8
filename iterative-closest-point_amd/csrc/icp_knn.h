// icp_knn.h -- the exact grid k-NN's device half: a lane's sorted (d2, index) list in LDS and the search
// that fills it.  Shared by the kernels of icp_normals.hip (the lists, the normals) and
// icp_filter.hip (the statistical filter's mean distances), whose grids icp_cloud.hip builds, and, with the
// k = 1 form in registers below, by icp_eval.hip (a cloud searched in another cloud's grid); the rules and
// the bounds of every loop are stated at the head of icp_normals.hip.  Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "icp_gridbox.h"
#include "icp_kernels.h"

namespace icp {

constexpr int kKnnBlock = 64; // one wave: a lane's list is a column of the [slot][lane] arrays

// the list's order: ascending (d2, index) -- the first-minimum rule extended to k
__device__ __forceinline__ bool knn_less(double da, int ia, double db, int ib)
{
    return da < db || (da == db && ia < ib);
}

// offers (d2, i) to this lane's sorted list (ld, li: its column; n of k slots filled; worst: the
// k-th distance once the list is full, +inf before, kept in a register so that a candidate beyond
// it costs no LDS access)
__device__ __forceinline__ void knn_offer(double *ld, int *li, int k, int &n, double &worst, double d2, int i)
{
    if (d2 > worst || (d2 == worst && i > li[(k - 1) * kKnnBlock])) return;
    int j = n < k ? n : k - 1;
    for (; j > 0; --j) { // (at most k - 1 moves)
        const double dp = ld[(j - 1) * kKnnBlock];
        const int ip = li[(j - 1) * kKnnBlock];
        if (!knn_less(d2, i, dp, ip)) break;
        ld[j * kKnnBlock] = dp;
        li[j * kKnnBlock] = ip;
    }
    ld[j * kKnnBlock] = d2;
    li[j * kKnnBlock] = i;
    if (n < k) ++n;
    if (n == k) worst = ld[(k - 1) * kKnnBlock];
}

// the sorted points [b, e) against the query
__device__ __forceinline__ void knn_scan_range(const double4 *__restrict__ pts, int b, int e, double qx, double qy,
                                               double qz, double *ld, int *li, int k, int &n, double &worst)
{
    for (int p = b; p < e; ++p) {
        const double4 m = pts[p];
        const double dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        knn_offer(ld, li, k, n, worst, d2, (int)m.w);
    }
}

// cells [x0, x1] of the row starting at cell `row` (nothing when x0 > x1); returns the points evaluated
__device__ __forceinline__ int knn_scan_run(const GridView &gv, int row, int x0, int x1, double qx, double qy, double qz,
                                            double *ld, int *li, int k, int &n, double &worst)
{
    if (x0 > x1) return 0;
    const int b = gv.start[row + x0], e = gv.start[row + x1 + 1];
    knn_scan_range(gv.pts, b, e, qx, qy, qz, ld, li, k, n, worst);
    return e - b;
}

// the box of cells [c0, c1] as x-runs, without the cells of the box [e0, e1] when kExcept (they
// have been scanned: each point is offered once); returns the points evaluated
template <bool kExcept>
__device__ __forceinline__ int knn_scan_box(const GridView &gv, const int c0[3], const int c1[3], const int e0[3],
                                            const int e1[3], double qx, double qy, double qz, double *ld, int *li, int k,
                                            int &n, double &worst)
{
    int seen = 0;
    for (int cz = c0[2]; cz <= c1[2]; ++cz)
        for (int cy = c0[1]; cy <= c1[1]; ++cy) {
            const int row = (cz * gv.g[1] + cy) * gv.g[0];
            if (kExcept && cz >= e0[2] && cz <= e1[2] && cy >= e0[1] && cy <= e1[1]) {
                seen += knn_scan_run(gv, row, c0[0], min(c1[0], e0[0] - 1), qx, qy, qz, ld, li, k, n, worst);
                seen += knn_scan_run(gv, row, max(c0[0], e1[0] + 1), c1[0], qx, qy, qz, ld, li, k, n, worst);
            } else {
                seen += knn_scan_run(gv, row, c0[0], c1[0], qx, qy, qz, ld, li, k, n, worst);
            }
        }
    return seen;
}

struct KnnCount {
    int scans;    // box scans (1 or 2; 0 when the query went straight to the scan of every point)
    int brute;    // 1 when every point was scanned
    long long seen; // candidates evaluated
};

// this lane's k nearest model points of q, sorted, into its list
__device__ __forceinline__ KnnCount knn_search(const GridView &gv, int nm, int k, int budget, double qx, double qy,
                                               double qz, double *ld, int *li)
{
    KnnCount kc{0, 0, 0};
    const double q[3] = {qx, qy, qz};
    int c[3], c0[3], c1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = cell1(q[a], gv.lo[a], gv.inv_h, gv.g[a]);
    const int gmax = max(gv.g[0], max(gv.g[1], gv.g[2]));
    bool found = false;
    for (int r = 0; r < gmax && !found; ++r) { // (a): from the own cell; the box of radius gmax - 1 is the whole grid
        long long cells = 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c0[a] = max(c[a] - r, 0);
            c1[a] = min(c[a] + r, gv.g[a] - 1);
            cells *= (long long)(c1[a] - c0[a] + 1);
        }
        if (cells > budget) break;
        int have = 0;
        for (int cz = c0[2]; cz <= c1[2]; ++cz)
            for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                const int row = (cz * gv.g[1] + cy) * gv.g[0];
                have += gv.start[row + c1[0] + 1] - gv.start[row + c0[0]];
            }
        found = have >= k;
    }
    int n = 0;
    double worst = INFINITY;
    if (found) {
        kc.seen += knn_scan_box<false>(gv, c0, c1, c0, c1, qx, qy, qz, ld, li, k, n, worst); // (b)
        kc.scans = 1;
        int b0[3], b1[3];
        const bool fits = complete_box_r(q, sqrt(worst), gv, budget, b0, b1); // (c)
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) inside = inside && b0[a] >= c0[a] && b1[a] <= c1[a];
        if (inside) return kc;
        if (fits) { // (the list stays: its points are candidates like the new cells')
            kc.seen += knn_scan_box<true>(gv, b0, b1, c0, c1, qx, qy, qz, ld, li, k, n, worst);
            kc.scans = 2;
            return kc;
        }
        n = 0;
        worst = INFINITY;
    }
    knn_scan_range(gv.pts, 0, nm, qx, qy, qz, ld, li, k, n, worst);
    kc.seen += nm;
    kc.brute = 1;
    return kc;
}

// ---- k = 1: the best (d2, index) under knn_less in two registers, no list (icp_eval.hip: one cloud's
// points searched in ANOTHER cloud's grid).  (bd, bi) start at (+inf, INT_MAX); bi == INT_MAX afterwards:
// no candidate had a d2 that compares (a NaN query).  A query may lie outside the grid's box: cell1 clamps,
// so its cell is the nearest boundary cell, and every stop below follows from complete_box_r alone, never
// from the query lying in its own cell.

__device__ __forceinline__ void nn1_scan_range(const double4 *__restrict__ pts, int b, int e, double qx, double qy,
                                               double qz, double &bd, int &bi)
{
    for (int p = b; p < e; ++p) {
        const double4 m = pts[p];
        const double dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const int i = (int)m.w;
        if (knn_less(d2, i, bd, bi)) {
            bd = d2;
            bi = i;
        }
    }
}

// the box of cells [c0, c1] as x-runs, without the cells of the box [e0, e1] when kExcept
template <bool kExcept>
__device__ __forceinline__ void nn1_scan_box(const GridView &gv, const int c0[3], const int c1[3], const int e0[3],
                                             const int e1[3], double qx, double qy, double qz, double &bd, int &bi)
{
    for (int cz = c0[2]; cz <= c1[2]; ++cz)
        for (int cy = c0[1]; cy <= c1[1]; ++cy) {
            const int row = (cz * gv.g[1] + cy) * gv.g[0];
            if (kExcept && cz >= e0[2] && cz <= e1[2] && cy >= e0[1] && cy <= e1[1]) {
                const int xa = min(c1[0], e0[0] - 1), xb = max(c0[0], e1[0] + 1);
                if (c0[0] <= xa) nn1_scan_range(gv.pts, gv.start[row + c0[0]], gv.start[row + xa + 1], qx, qy, qz, bd, bi);
                if (xb <= c1[0]) nn1_scan_range(gv.pts, gv.start[row + xb], gv.start[row + c1[0] + 1], qx, qy, qz, bd, bi);
            } else {
                nn1_scan_range(gv.pts, gv.start[row + c0[0]], gv.start[row + c1[0] + 1], qx, qy, qz, bd, bi);
            }
        }
}

// knn_search's expansion with k = 1: (a) the ring around the query's (clamped) cell until the box holds
// a point or goes over the budget, (b) that box scanned, (c) the completeness box of the best distance:
// inside the scanned box -> done, within the budget -> its other cells, else (d) every point.  Every loop
// is bounded by the grid's size or by nm.
__device__ __forceinline__ void nn1_search(const GridView &gv, int nm, int budget, double qx, double qy, double qz,
                                           double &bd, int &bi)
{
    const double q[3] = {qx, qy, qz};
    int c[3], c0[3], c1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = cell1(q[a], gv.lo[a], gv.inv_h, gv.g[a]);
    const int gmax = max(gv.g[0], max(gv.g[1], gv.g[2]));
    bool found = false;
    for (int r = 0; r < gmax && !found; ++r) {
        long long cells = 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c0[a] = max(c[a] - r, 0);
            c1[a] = min(c[a] + r, gv.g[a] - 1);
            cells *= (long long)(c1[a] - c0[a] + 1);
        }
        if (cells > budget) break;
        for (int cz = c0[2]; cz <= c1[2] && !found; ++cz)
            for (int cy = c0[1]; cy <= c1[1] && !found; ++cy) {
                const int row = (cz * gv.g[1] + cy) * gv.g[0];
                found = gv.start[row + c1[0] + 1] > gv.start[row + c0[0]];
            }
    }
    if (found) {
        nn1_scan_box<false>(gv, c0, c1, c0, c1, qx, qy, qz, bd, bi);
        if (bi != INT_MAX) { // (else no d2 compared: the scan of every point below ends the same way)
            int b0[3], b1[3];
            const bool fits = complete_box_r(q, sqrt(bd), gv, budget, b0, b1);
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) inside = inside && b0[a] >= c0[a] && b1[a] <= c1[a];
            if (inside) return;
            if (fits) { // (the best so far stays: a candidate like the new cells' points)
                nn1_scan_box<true>(gv, b0, b1, c0, c1, qx, qy, qz, bd, bi);
                return;
            }
        }
        bd = INFINITY;
        bi = INT_MAX;
    }
    nn1_scan_range(gv.pts, 0, nm, qx, qy, qz, bd, bi);
}

// the dynamic LDS of a launch of kKnnBlock lanes with lists of k entries
inline size_t knn_lds_bytes(int k) { return (size_t)k * kKnnBlock * (sizeof(double) + sizeof(int)); }

} // namespace icp
