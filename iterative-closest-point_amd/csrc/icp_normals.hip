// icp_normals.hip -- the model's k nearest neighbours over its own grid, and the normals estimated
// from them (icp_model_knn, icp_estimate_model_normals).
//
// One lane per query, the queries in the grid's cell-sorted order (a wave's queries share boxes and
// rows), the results written by the model index each sorted point carries in w.  A lane keeps its k
// best (d2, index) pairs as a sorted list in LDS, laid out [slot][lane] so that the wave's accesses
// to one slot fall into consecutive banks; nothing of it is indexed in registers, so no kernel here
// has a private array with a runtime index.
//
// A query is answered by at most two scans:
//   (a) the ring radius r around its cell grows, on differences of the cell starts alone, until the
//       box of cells holds >= k points;
//   (b) that box is scanned row by row -- a run of cells along x is one contiguous range of the
//       sorted points -- and the k best are kept; d_k is the k-th squared distance;
//   (c) the list is final when the complete box of radius sqrt(d_k) (icp_gridbox.h: every point
//       with D64 <= d_k lies in it; a face clamped at the grid's edge has nothing beyond it) lies
//       inside the scanned box.  Otherwise that complete box holds every point that can be among
//       the k nearest, and its cells outside the scanned box are offered to the same list: the
//       second scan is always final.  (Measured: rebuilding the list from the complete box instead
//       cost more than the candidates it spared, the first k offers of a scan all being inserts.)
//   A box over the cell budget sends the query to a scan of all nm points.
// Every loop is bounded: r by the grid's largest extent, a scan by its box, an insertion by k.
// Compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz rounds as written.
#include <hip/hip_runtime.h>

#include "icp_knn.h"

namespace icp {
namespace {

// One Jacobi rotation of a symmetric 3 x 3 matrix in the (p, q) plane: it annihilates a_pq; r is
// the third index.  v?p / v?q: the accumulated eigenvectors' columns p and q.  Every operand is a
// named scalar, so the indices are compile-time.
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                           double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    // (theta * theta may overflow to +inf: then t = 0 and the rotation is the identity, as it should)
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = cs * arp - sn * arq, rq = sn * arp + cs * arq;
    arp = rp;
    arq = rq;
    const double u0 = cs * v0p - sn * v0q, w0 = sn * v0p + cs * v0q;
    const double u1 = cs * v1p - sn * v1q, w1 = sn * v1p + cs * v1q;
    const double u2 = cs * v2p - sn * v2q, w2 = sn * v2p + cs * v2q;
    v0p = u0, v0q = w0, v1p = u1, v1q = w1, v2p = u2, v2q = w2;
}

constexpr int kJacobiSweeps = 10; // (cyclic Jacobi converges quadratically: 3 x 3 settles in 4 or 5)

// the normal of the neighbourhood in this lane's list (steps 2 to 4 of the header's semantics);
// returns false, and a zero normal, when the direction is undetermined
__device__ __forceinline__ bool knn_normal(const double4 *__restrict__ m4, const int *li, int k, double qx, double qy,
                                           double qz, bool has_view, double vx, double vy, double vz, double nrm[3])
{
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int s = 0; s < k; ++s) {
        const double4 m = m4[li[s * kKnnBlock]];
        sx += m.x, sy += m.y, sz += m.z;
    }
    const double kk = (double)k;
    const double mx = sx / kk, my = sy / kk, mz = sz / kk;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int s = 0; s < k; ++s) {
        const double4 m = m4[li[s * kKnnBlock]];
        const double dx = m.x - mx, dy = m.y - my, dz = m.z - mz;
        a00 += dx * dx, a01 += dx * dy, a02 += dx * dz;
        a11 += dy * dy, a12 += dy * dz, a22 += dz * dz;
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21); // (0, 1), r = 2
        jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22); // (0, 2), r = 1
        jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22); // (1, 2), r = 0
    }
    // the eigenvalues are the diagonal; the smallest one's column (the first at a tie)
    const double l_lo = fmin(a00, fmin(a11, a22)), l_hi = fmax(a00, fmax(a11, a22));
    const double l_mid = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
    nrm[0] = nrm[1] = nrm[2] = 0.0;
    if (!(l_hi > 0.0) || l_mid - l_lo <= 1e-12 * l_hi) return false;
    double nx, ny, nz;
    if (a00 <= a11 && a00 <= a22) nx = v00, ny = v10, nz = v20;
    else if (a11 <= a22) nx = v01, ny = v11, nz = v21;
    else nx = v02, ny = v12, nz = v22;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx /= len, ny /= len, nz /= len;
    bool flip;
    if (has_view) {
        const double wx = vx - qx, wy = vy - qy, wz = vz - qz;
        flip = (nx * wx + ny * wy) + nz * wz < 0.0;
    } else {
        const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
        const double big = ax >= ay && ax >= az ? nx : (ay >= az ? ny : nz);
        flip = big < 0.0;
    }
    nrm[0] = flip ? -nx : nx;
    nrm[1] = flip ? -ny : ny;
    nrm[2] = flip ? -nz : nz;
    return true;
}

struct KnnView {
    double v[3];
    int on;
};

// kNormals: n4[index] = the query's normal; else row `index` of idx_out / d2_out (nullable) = its list.
// counters (nullable unless kNormals): [0] undetermined normals; with debug also [1] second scans,
// [2] scans of every point, [3] candidates evaluated.
template <bool kNormals>
__global__ __launch_bounds__(kKnnBlock) void model_knn_kernel(GridView gv, const double4 *__restrict__ m4, int nm, int k,
                                                               int budget, int *__restrict__ idx_out,
                                                               double *__restrict__ d2_out, double4 *__restrict__ n4,
                                                               KnnView view, unsigned long long *counters, int debug)
{
    extern __shared__ double knn_lds[];
    double *ld = knn_lds + threadIdx.x;
    int *li = (int *)(knn_lds + (size_t)k * kKnnBlock) + threadIdx.x;
    const int t = blockIdx.x * kKnnBlock + threadIdx.x;
    if (t >= nm) return; // (no barrier below: a lane's list is its own)
    const double4 q = gv.pts[t];
    const int self = (int)q.w;
    const KnnCount kc = knn_search(gv, nm, k, budget, q.x, q.y, q.z, ld, li);
    if (kNormals) {
        double nrm[3];
        const bool ok = knn_normal(m4, li, k, q.x, q.y, q.z, view.on != 0, view.v[0], view.v[1], view.v[2], nrm);
        n4[self] = make_double4(nrm[0], nrm[1], nrm[2], 0.0);
        if (!ok) atomicAdd(&counters[0], 1ULL);
    } else {
        const size_t row = (size_t)self * (size_t)k;
        for (int s = 0; s < k; ++s) {
            idx_out[row + s] = li[s * kKnnBlock];
            if (d2_out) d2_out[row + s] = ld[s * kKnnBlock];
        }
    }
    if (debug && counters) {
        if (kc.scans == 2) atomicAdd(&counters[1], 1ULL);
        if (kc.brute) atomicAdd(&counters[2], 1ULL);
        atomicAdd(&counters[3], (unsigned long long)kc.seen);
    }
}

} // namespace

void launch_model_knn(const GridView &gv, const double4 *m4, int nm, int k, int budget, int *idx, double *d2,
                      hipStream_t st)
{
    if (nm <= 0) return;
    model_knn_kernel<false><<<(nm + kKnnBlock - 1) / kKnnBlock, kKnnBlock, knn_lds_bytes(k), st>>>(
        gv, m4, nm, k, budget, idx, d2, nullptr, KnnView{{0.0, 0.0, 0.0}, 0}, nullptr, 0);
}

void launch_model_normals(const GridView &gv, const double4 *m4, int nm, int k, int budget, const double *viewpoint,
                          double4 *n4, unsigned long long *counters, bool debug, hipStream_t st)
{
    if (nm <= 0) return;
    KnnView view{{0.0, 0.0, 0.0}, 0};
    if (viewpoint) view = KnnView{{viewpoint[0], viewpoint[1], viewpoint[2]}, 1};
    model_knn_kernel<true><<<(nm + kKnnBlock - 1) / kKnnBlock, kKnnBlock, knn_lds_bytes(k), st>>>(
        gv, m4, nm, k, budget, nullptr, nullptr, n4, view, counters, debug ? 1 : 0);
}

} // namespace icp
