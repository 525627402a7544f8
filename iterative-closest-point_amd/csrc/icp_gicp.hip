// icp_gicp.hip — the kernels of icp_run's plane-to-plane iteration (icp_set_plane_to_plane on
// ICP_METRIC_POINT_TO_PLANE; generalised ICP, Segal, Haehnel and Thrun 2009, in the regularised form of
// PCL and Open3D): the moments of the 6 x 6 normal equations with a 3 x 3 information matrix a pair, and
// the transform with the Mahalanobis residual.  The fold, the solve and the step are icp_plane.hip's
// one-sided plane_solve_kernel as it stands, the residual's fold and error step icp_gated.hip's.
//
// A point's covariance has the eigenvalues (eps, 1, 1), eps along its normal: C = I - (1 - eps) n n^T, a
// function of the normals the context holds.  One iteration on the scene p (n points on this rank),
// after the search has left idx; N = the model's normals as given, u0 = the scene's as given, in the
// scene's current order, c = the model's centre, Q = the rotation of the total since icp_set_scene* at
// the iteration's start (SymmArgs, as the symmetric form holds it), k1 = 1 - eps (fp64, once on the host):
//   y_j = m[idx_j], d_j = p_j - y_j, d2_j, keep_j, the mask and K: kept_pairs_pass, as every kept-pairs loop;
//   N_j = N[idx_j], u_j = Q u0_j (each row summed as ((Q0 u0 + Q1 u1) + Q2 u2));
//   S = 2 I - k1 (N_j N_j^T + u_j u_j^T): s_ab = [a == b ? 2 : 0] - k1 * (N_a * N_b + u_a * u_b), six
//   entries; a zero normal leaves that cloud's covariance I, and no bit depends on a normal's sign;
//   the cofactors c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11,
//   c11 = s00 s22 - s02 s02, c12 = s01 s02 - s00 s12, c22 = s00 s11 - s01 s01,
//   det = (s00 c00 + s01 c01) + s02 c02;  S is positive definite when s00 > 0, c22 > 0 and det > 0 (false
//   for a NaN): otherwise the pair counts in K and adds nothing else;  M = c * (1 / det);
//   v = p_j - c, g = M d (rows summed as above), r2 = (dx g0 + dy g1) + dz g2, w = the robust weight of r2
//   (1 without: not multiplied; with it M and g are scaled by w before the sums);
//   H = [v]x M (column k = v x M_k);  the sums, in the plane metric's columns (upper triangle of the 6 x 6
//   by rows, then b, then the count): rows 0..2 x columns 0..2 = row r of H crossed, (v x H_r)_c; rows
//   0..2 x columns 3..5 = H; rows 3..5 x columns 3..5 = M; b = [v x g ; g] (the solve negates it); with
//   weights W = sum w and K+ = #{w > 0} behind the count.  For M = n n^T these are icp_plane.hip's a a^T
//   and a r.
//   The one-sided solve gives x: R = exp([omega]x), t = (c + tau) - R c, s = 1; every point moves by
//   q = R p + t, and err = (e + e) / K with e = sum over the kept pairs of (q - y)^T M' (q - y), M' formed
//   as above from N_j and Q' u0_j, Q' the total's rotation with this step composed (a pair whose S' is
//   not positive definite adds 0).
// The loop over the pairs with the gate and its mask, the transform's body and the robust weight are
// icp_kept.h's.  Compiled with IEEE semantics like icp_plane.hip (`d2 <= D` and the three `> 0` must stay
// false for a NaN).  The total's rotation and the wave-uniform read are icp_plane.hip's, restated here:
// that file's kernels keep their source until these twins are folded into them.
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_fold.h"
#include "icp_kept.h"
#include "icp_kernels.h"

namespace icp {
namespace {

// Q = the rotation of the total since icp_set_scene*, by one thread (icp_plane.hip's symm_total_rotation:
// the run's so far composed onto the context's at the run's start, in compose_srt's arithmetic)
__device__ __forceinline__ void gicp_total_rotation(const IterState *__restrict__ st, const SymmArgs &sy, double *q)
{
    if (st->tot_n == 0) {
        for (int k = 0; k < 9; ++k) q[k] = sy.q0[k]; // (the identity without one)
    } else if (!sy.have_q0) {
        for (int k = 0; k < 9; ++k) q[k] = st->tot[1 + k];
    } else {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double a = st->tot[1 + 3 * r] * sy.q0[c], b = st->tot[2 + 3 * r] * sy.q0[3 + c],
                             d = st->tot[3 + 3 * r] * sy.q0[6 + c];
                q[3 * r + c] = (a + b) + d;
            }
    }
}

// v, which every lane of the wave holds alike, as a value the compiler knows to be wave-uniform
__device__ __forceinline__ double wave_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// Q into scalar registers: one thread forms it in LDS, every wave reads it uniformly
__device__ __forceinline__ void gicp_load_rotation(const SymmArgs &sy, double *Q)
{
    __shared__ double sq[9];
    if (threadIdx.x == 0) gicp_total_rotation(sy.st, sy, sq);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) Q[k] = wave_uniform(sq[k]);
}

// The pair's information matrix M = S^-1 (m: 00 01 02 11 12 22) from the model's N and the scene's u0 as
// given; false, and m untouched, when S is not positive definite (the file's head).
__device__ __forceinline__ bool gicp_information(const double4 &N, double a0, double a1, double a2, const double *Q, double k1,
                                                 double *m)
{
    const double u0 = (Q[0] * a0 + Q[1] * a1) + Q[2] * a2;
    const double u1 = (Q[3] * a0 + Q[4] * a1) + Q[5] * a2;
    const double u2 = (Q[6] * a0 + Q[7] * a1) + Q[8] * a2;
    const double s00 = 2.0 - k1 * (N.x * N.x + u0 * u0);
    const double s01 = 0.0 - k1 * (N.x * N.y + u0 * u1);
    const double s02 = 0.0 - k1 * (N.x * N.z + u0 * u2);
    const double s11 = 2.0 - k1 * (N.y * N.y + u1 * u1);
    const double s12 = 0.0 - k1 * (N.y * N.z + u1 * u2);
    const double s22 = 2.0 - k1 * (N.z * N.z + u2 * u2);
    const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    if (!(s00 > 0.0 && c22 > 0.0 && det > 0.0)) return false;
    const double inv = 1.0 / det;
    m[0] = c00 * inv;
    m[1] = c01 * inv;
    m[2] = c02 * inv;
    m[3] = c11 * inv;
    m[4] = c12 * inv;
    m[5] = c22 * inv;
    return true;
}

// The sums over the kept pairs (kept_pairs_pass): the plane metric's 21 + 6 and the kept count, in its
// columns, each pair entering with its own 3 x 3 information matrix (the file's head).  KIND, a robust
// weight of the squared Mahalanobis residual (X = k, k2): M and g are scaled by w, and W and K+ are the
// 29th and 30th sums.  Q goes through LDS into scalar registers as in the symmetric kernels.
// A frozen iteration (st->done) returns at once: neither its sums nor the mask are written.
template <bool YIN, int KIND, class CUT, class... X>
__global__ __launch_bounds__(kBlock) void gicp_moments_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double4 *__restrict__ n4,
    const double *__restrict__ px, const double *__restrict__ py, const double *__restrict__ pz, int n,
    double *__restrict__ yx, double *__restrict__ yy, double *__restrict__ yz, const IterState *__restrict__ st, double D,
    double c0, double c1, double c2, unsigned long long *__restrict__ mask, double *__restrict__ partials,
    const int *__restrict__ kpos, const double4 *__restrict__ m4kd, GicpArgs ga, X... kk, CUT cut)
{
    constexpr bool kRobust = KIND != kRobustNone;
    constexpr int WIDTH = kept_width(true, kRobust);
    if (st->done != 0) return;
    double Q[9]; // (the same in every lane: kept in scalar registers)
    gicp_load_rotation(ga.sy, Q);
    const double k1 = ga.k1;
    double a[WIDTH];
#pragma unroll
    for (int j = 0; j < WIDTH; ++j) a[j] = 0.0;
    kept_pairs_pass<YIN, kKeptUnique<CUT>>(
        idx, m4, px, py, pz, n, yx, yy, yz, kept_cut(D, cut_of(cut)), mask, kpos, m4kd, best_of(cut),
        [&](long long i, double q0, double q1, double q2, const double4 &, double dx, double dy, double dz)
            __attribute__((always_inline)) {
                a[kPlaneCount] += 1.0;
                double m[6];
                if (!gicp_information(n4[idx[i]], ga.sy.ux[i], ga.sy.uy[i], ga.sy.uz[i], Q, k1, m)) return;
                double g[3];
                g[0] = (m[0] * dx + m[1] * dy) + m[2] * dz;
                g[1] = (m[1] * dx + m[3] * dy) + m[4] * dz;
                g[2] = (m[2] * dx + m[4] * dy) + m[5] * dz;
                if constexpr (kRobust) {
                    const double r2 = (dx * g[0] + dy * g[1]) + dz * g[2];
                    const double w = robust_weight<KIND>(r2, kk...);
#pragma unroll
                    for (int k = 0; k < 6; ++k) m[k] = w * m[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) g[k] = w * g[k];
                    a[kRobustPlaneW] += w;
                    a[kRobustPlaneKpos] += w > 0.0 ? 1.0 : 0.0;
                }
                const double v0 = q0 - c0, v1 = q1 - c1, v2 = q2 - c2;
                // the columns of M: M_0 = (m0, m1, m2), M_1 = (m1, m3, m4), M_2 = (m2, m4, m5)
                const double mc[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
                double h[3][3]; // H = [v]x M: h[r][k] = (v x M_k)_r
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    h[0][k] = v1 * mc[k][2] - v2 * mc[k][1];
                    h[1][k] = v2 * mc[k][0] - v0 * mc[k][2];
                    h[2][k] = v0 * mc[k][1] - v1 * mc[k][0];
                }
                // rows 0..2: (v x H_r)_c for c >= r, then H's row r
                a[0] += v1 * h[0][2] - v2 * h[0][1];
                a[1] += v2 * h[0][0] - v0 * h[0][2];
                a[2] += v0 * h[0][1] - v1 * h[0][0];
                a[3] += h[0][0];
                a[4] += h[0][1];
                a[5] += h[0][2];
                a[6] += v2 * h[1][0] - v0 * h[1][2];
                a[7] += v0 * h[1][1] - v1 * h[1][0];
                a[8] += h[1][0];
                a[9] += h[1][1];
                a[10] += h[1][2];
                a[11] += v0 * h[2][1] - v1 * h[2][0];
                a[12] += h[2][0];
                a[13] += h[2][1];
                a[14] += h[2][2];
                // rows 3..5: M's upper triangle
                a[15] += m[0];
                a[16] += m[1];
                a[17] += m[2];
                a[18] += m[3];
                a[19] += m[4];
                a[20] += m[5];
                // b = [v x g ; g]
                a[kPlaneB + 0] += v1 * g[2] - v2 * g[1];
                a[kPlaneB + 1] += v2 * g[0] - v0 * g[2];
                a[kPlaneB + 2] += v0 * g[1] - v1 * g[0];
                a[kPlaneB + 3] += g[0];
                a[kPlaneB + 4] += g[1];
                a[kPlaneB + 5] += g[2];
            });
    block_sum_store<WIDTH>(a, partials + (size_t)blockIdx.x * WIDTH);
}

// Every point moves, and the squared Mahalanobis residual is summed over the kept points
// (kept_transform): M' is formed again from N gathered through idx and Q' u0, Q' the total's rotation
// with the step just composed (the step kernel ran before this one; a frozen run returns before Q' is
// used).
__global__ __launch_bounds__(kBlock) void gicp_transform_kernel(
    double *__restrict__ px, double *__restrict__ py, double *__restrict__ pz, const double *__restrict__ yx,
    const double *__restrict__ yy, const double *__restrict__ yz, int n, const Xform *__restrict__ xfd,
    const int *__restrict__ done, float4 *__restrict__ p32, const unsigned long long *__restrict__ mask,
    const int *__restrict__ idx, const double4 *__restrict__ n4, double *__restrict__ partials, GicpArgs ga)
{
    double Q[9]; // (the same in every lane: kept in scalar registers)
    gicp_load_rotation(ga.sy, Q);
    const double k1 = ga.k1;
    kept_transform(px, py, pz, n, xfd, done, p32, mask, partials,
                   [&](long long i, double q0, double q1, double q2) __attribute__((always_inline)) {
                       double m[6];
                       if (!gicp_information(n4[idx[i]], ga.sy.ux[i], ga.sy.uy[i], ga.sy.uz[i], Q, k1, m)) return 0.0;
                       const double e0 = q0 - yx[i], e1 = q1 - yy[i], e2 = q2 - yz[i];
                       const double g0 = (m[0] * e0 + m[1] * e1) + m[2] * e2;
                       const double g1 = (m[1] * e0 + m[3] * e1) + m[4] * e2;
                       const double g2 = (m[2] * e0 + m[4] * e1) + m[5] * e2;
                       return (e0 * g0 + e1 * g1) + e2 * g2;
                   });
}

} // namespace

void launch_gicp_moments(const KeptPass &a, bool y_ready)
{
    kept_dispatch(y_ready, a.robust_kind, [&](auto yin, auto kind) {
        const auto go = [&](auto... kk) {
            kept_tail(yin, a, [&](auto cut) {
                gicp_moments_kernel<yin(), kind(), decltype(cut), decltype(kk)...><<<red_blocks(a.n), kBlock, 0, a.st>>>(
                    a.idx, a.m4, a.n4, a.px, a.py, a.pz, a.n, a.yx, a.yy, a.yz, a.st_dev, a.D, a.c[0], a.c[1], a.c[2], a.mask,
                    a.partials, a.kpos, a.m4kd, *a.gicp, kk..., cut);
            });
        };
        if constexpr (kind() == kRobustNone) go();
        else go(a.k, a.k2);
    });
}

void launch_gicp_transform(double *px, double *py, double *pz, const double *yx, const double *yy, const double *yz, int n,
                           const Xform *xf, const int *done, float4 *p32, const unsigned long long *mask, const int *idx,
                           const double4 *n4, double *partials, hipStream_t st, const GicpArgs &gicp)
{
    gicp_transform_kernel<<<red_blocks(n), kBlock, 0, st>>>(px, py, pz, yx, yy, yz, n, xf, done, p32, mask, idx, n4, partials,
                                                            gicp);
}

} // namespace icp
