// icp_global.hip -- global registration: FPFH descriptors of a cloud, the nearest
// descriptor of every row of one set in another, a rigid pose from putative pairs by RANSAC, and
// the chain of the three (icp_fpfh, icp_match_features, icp_ransac_pose, icp_global_pose;
// include/icp_capi.h states every rule).  The four calls take host arrays, are synchronous, keep
// their device memory to themselves (an owning Scratch, icp_engine.h: allocated and freed inside the call)
// and touch neither the resident clouds nor anything a run depends on.  icp_fpfh's grid: cloud_knn, icp_cloud.hip.
//
// Kernels (all fp64 as written, -ffp-contract=off; no floating-point atomic anywhere):
//   spfh_kernel          one wave a point, one list entry a lane: the pair feature of (i, N_i[lane]),
//                        its three bins counted by LDS integer atomics, the counted pairs by a ballot;
//                        lanes 0-32 write cnt * (100 / c).  Integer counts: the order cannot matter.
//   fpfh_kernel          one wave a point, lanes 0-32 a bin each: the k neighbours' SPFH rows (one
//                        coalesced 264-byte read each) weighted by 1 / d2 serially in list order; the
//                        three third-sums serially in bin order from the wave's LDS row.
//   match_kernel         one query a lane, its 33 doubles in registers; a workgroup takes one range
//                        of fb (blockIdx.y), staged in LDS in tiles of kMatchTile rows and read by
//                        broadcast; the lane keeps the first minimum of its range.
//   match_merge_kernel   the ranges' (D, index) partials in ascending range order, strict <: the
//                        first minimum over all of fb.
//   ransac_pose_kernel   pass A, one hypothesis a lane: the draw, the edge check, Horn's pose
//                        (icp_horn.h); the survivors' poses are compacted (an integer atomic slot).
//   ransac_count_kernel  pass B, one wave a survivor: the pairs within max_dist counted by ballots,
//                        then the unsigned 64-bit atomic maximum over (count << 32) | (2^32 - 1 - h).
//   ransac_winner_kernel, ransac_mask_kernel: the winner's pose made again from its h, its mask.
// Every loop is bounded: by k, by the tile, by the range, by C, by the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "icp_engine.h"
#include "icp_horn.h"

namespace {

constexpr int kDim = ICP_FPFH_DIM;
constexpr int kFeatWaves = 4; // points a workgroup of the two descriptor kernels

// clamp(floor(11 u), 0, 10); a NaN goes to bin 0
__device__ __forceinline__ int fpfh_bin(double u)
{
    const double f = floor(11.0 * u);
    if (!(f >= 0.0)) return 0;
    return f > 10.0 ? 10 : (int)f;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(64 * kFeatWaves) void spfh_kernel(const double4 *__restrict__ rows,
                                                               const double4 *__restrict__ nrm,
                                                               const int *__restrict__ idx, int n, int k,
                                                               double *__restrict__ spfh)
{
    __shared__ int cnt[kFeatWaves][kDim + 1];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kFeatWaves + w;
    if (lane < kDim) cnt[w][lane] = 0;
    __syncthreads();
    bool counted = false;
    if (i < n && lane < k) {
        const int j = idx[(size_t)i * (size_t)k + lane];
        const double4 xi = rows[i], ni = nrm[i];
        const double4 xj = rows[j], nj = nrm[j];
        const double dx = xj.x - xi.x, dy = xj.y - xi.y, dz = xj.z - xi.z;
        const double L2 = (dx * dx + dy * dy) + dz * dz;
        const bool zi = ni.x == 0.0 && ni.y == 0.0 && ni.z == 0.0, zj = nj.x == 0.0 && nj.y == 0.0 && nj.z == 0.0;
        if (j != i && L2 != 0.0 && !zi && !zj) {
            const double L = sqrt(L2);
            const double a1 = dot3(ni.x, ni.y, ni.z, dx, dy, dz) / L, a2 = dot3(nj.x, nj.y, nj.z, dx, dy, dz) / L;
            const bool swap = fabs(a1) < fabs(a2); // the frame on the point whose normal is closer to the line
            const double n1x = swap ? nj.x : ni.x, n1y = swap ? nj.y : ni.y, n1z = swap ? nj.z : ni.z;
            const double n2x = swap ? ni.x : nj.x, n2y = swap ? ni.y : nj.y, n2z = swap ? ni.z : nj.z;
            const double ex = swap ? -dx : dx, ey = swap ? -dy : dy, ez = swap ? -dz : dz;
            const double f3 = swap ? -a2 : a1;
            double vx = ey * n1z - ez * n1y, vy = ez * n1x - ex * n1z, vz = ex * n1y - ey * n1x;
            const double vl2 = (vx * vx + vy * vy) + vz * vz;
            if (vl2 != 0.0) {
                const double vl = sqrt(vl2);
                vx /= vl, vy /= vl, vz /= vl;
                const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
                const double f2 = dot3(vx, vy, vz, n2x, n2y, n2z);
                const double f1 = atan2(dot3(wx, wy, wz, n2x, n2y, n2z), dot3(n1x, n1y, n1z, n2x, n2y, n2z));
                counted = true;
                atomicAdd(&cnt[w][fpfh_bin((f1 + M_PI) / (2.0 * M_PI))], 1);
                atomicAdd(&cnt[w][11 + fpfh_bin((f2 + 1.0) / 2.0)], 1);
                atomicAdd(&cnt[w][22 + fpfh_bin((f3 + 1.0) / 2.0)], 1);
            }
        }
    }
    const int c = __popcll(__ballot(counted));
    __syncthreads();
    if (i < n && lane < kDim)
        spfh[(size_t)i * kDim + lane] = c > 0 ? (double)cnt[w][lane] * (100.0 / (double)c) : 0.0;
}

__global__ __launch_bounds__(64 * kFeatWaves) void fpfh_kernel(const int *__restrict__ idx, const double *__restrict__ d2,
                                                               const double *__restrict__ spfh, int n, int k,
                                                               double *__restrict__ out)
{
    __shared__ double acc[kFeatWaves][kDim + 1];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kFeatWaves + w;
    const bool own = i < n && lane < kDim;
    double a = 0.0;
    if (own) {
        const size_t row = (size_t)i * (size_t)k;
        for (int s = 0; s < k; ++s) { // (the list's order: the stated order of the sum)
            const int j = idx[row + s];
            const double dd = d2[row + s];
            if (j != i && dd > 0.0) a += (1.0 / dd) * spfh[(size_t)j * kDim + lane];
        }
        acc[w][lane] = a;
    }
    __syncthreads();
    if (own) {
        const int b0 = (lane / 11) * 11;
        double T = 0.0;
        for (int b = 0; b < 11; ++b) T += acc[w][b0 + b];
        a = T > 0.0 ? a * (100.0 / T) : 0.0;
        out[(size_t)i * kDim + lane] = a + spfh[(size_t)i * kDim + lane];
    }
}

// ---- the feature match -------------------------------------------------------------------------
constexpr int kMatchBlock = 64;     // queries a workgroup: one wave
constexpr int kMatchTile = 64;      // rows of fb staged at a time
constexpr int kMatchRow = kDim + 1; // a staged row's doubles (16-byte aligned rows)
constexpr int kMatchMaxSplits = 64; // ranges of fb at most
constexpr int kMatchBlocks = 1024;  // workgroups aimed at

__global__ __launch_bounds__(kMatchBlock) void match_kernel(const double *__restrict__ fa, int na,
                                                            const double *__restrict__ fb, int nb, int chunk,
                                                            double *__restrict__ part_d, int *__restrict__ part_i)
{
    __shared__ double tile[kMatchTile * kMatchRow];
    const int a = blockIdx.x * kMatchBlock + threadIdx.x;
    const int ar = a < na ? a : na - 1; // (a lane past the end computes the last query and writes nothing)
    double q[kDim];
#pragma unroll
    for (int c = 0; c < kDim; ++c) q[c] = fa[(size_t)ar * kDim + c];
    const long long lo = (long long)blockIdx.y * chunk;
    const int b_lo = (int)(lo < nb ? lo : nb), b_hi = (int)(lo + chunk < nb ? lo + chunk : nb);
    double best = 0.0;
    int bi = -1;
    for (int t0 = b_lo; t0 < b_hi; t0 += kMatchTile) {
        const int rows = b_hi - t0 < kMatchTile ? b_hi - t0 : kMatchTile;
        __syncthreads();
        for (int e = threadIdx.x; e < rows * kDim; e += kMatchBlock) {
            const int r = e / kDim;
            tile[r * kMatchRow + (e - r * kDim)] = fb[(size_t)t0 * kDim + e];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const double *row = tile + r * kMatchRow;
            double D = 0.0;
#pragma unroll
            for (int c = 0; c < kDim; ++c) {
                const double d = q[c] - row[c];
                D += d * d;
            }
            if (D < best || (bi < 0 && D == D)) { // ascending b, strict <: the first minimum; a NaN never wins
                best = D;
                bi = t0 + r;
            }
        }
    }
    if (a < na) {
        part_d[(size_t)blockIdx.y * na + a] = best;
        part_i[(size_t)blockIdx.y * na + a] = bi;
    }
}

__global__ __launch_bounds__(256) void match_merge_kernel(const double *__restrict__ part_d,
                                                          const int *__restrict__ part_i, int splits, int na,
                                                          int *__restrict__ idx_out, double *__restrict__ dist_out)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= na) return;
    double best = 0.0;
    int bi = -1;
    for (int s = 0; s < splits; ++s) { // (ascending ranges are ascending indices)
        const double d = part_d[(size_t)s * na + a];
        const int i = part_i[(size_t)s * na + a];
        if (i >= 0 && (bi < 0 || d < best)) {
            best = d;
            bi = i;
        }
    }
    idx_out[a] = bi;
    if (dist_out) dist_out[a] = bi < 0 ? NAN : best;
}

// the ranges of fb: (chunk rows each, how many)
void match_plan(size_t na, size_t nb, int *chunk, int *splits)
{
    const long long qblocks = ((long long)na + kMatchBlock - 1) / kMatchBlock;
    const long long tiles = ((long long)nb + kMatchTile - 1) / kMatchTile;
    long long want = std::max<long long>(1, std::min<long long>(kMatchMaxSplits, kMatchBlocks / qblocks));
    want = std::min(want, tiles);
    const long long chunk_tiles = (tiles + want - 1) / want;
    *splits = (int)((tiles + chunk_tiles - 1) / chunk_tiles);
    *chunk = (int)std::min<long long>(chunk_tiles * kMatchTile, INT_MAX);
}

// ---- RANSAC ------------------------------------------------------------------------------------
constexpr int kRansacBatch = 1 << 16; // hypotheses a batch: the pose buffer's bound
constexpr int kPose = 12;             // R (row-major), t

struct RansacArgs {
    const double *p, *q; // the pairs p_c -> q_c, 3 x C col-major each
    int C;
    unsigned long long seed;
    double e2, max_d2;
};

__host__ __device__ inline unsigned long long splitmix64(unsigned long long x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}

__host__ __device__ inline void ransac_draw(unsigned long long seed, unsigned long long h, int C, int &i0, int &i1, int &i2)
{
    const unsigned long long g = 0x9E3779B97F4A7C15ULL, uc = (unsigned long long)C;
    const unsigned long long z0 = splitmix64(seed + (3ULL * h + 1ULL) * g), z1 = splitmix64(seed + (3ULL * h + 2ULL) * g),
                             z2 = splitmix64(seed + (3ULL * h + 3ULL) * g);
    i0 = (int)(z0 % uc);
    i1 = (int)(z1 % (uc - 1ULL));
    if (i1 >= i0) ++i1;
    i2 = (int)(z2 % (uc - 2ULL));
    const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
}

__device__ __forceinline__ double dist2(const double a[3], const double b[3])
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// hypothesis h: false when the edge check rejects it, else its pose
__device__ __forceinline__ bool ransac_hypothesis(const RansacArgs &A, unsigned long long h, double R[9], double t[3])
{
    int id0, id1, id2;
    ransac_draw(A.seed, h, A.C, id0, id1, id2);
    double P[3][3], Q[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        P[0][a] = A.p[3 * (size_t)id0 + a], P[1][a] = A.p[3 * (size_t)id1 + a], P[2][a] = A.p[3 * (size_t)id2 + a];
        Q[0][a] = A.q[3 * (size_t)id0 + a], Q[1][a] = A.q[3 * (size_t)id1 + a], Q[2][a] = A.q[3 * (size_t)id2 + a];
    }
    bool keep = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) { // (0, 1), (1, 2), (2, 0)
        const double lp = dist2(P[r], P[(r + 1) % 3]), lq = dist2(Q[r], Q[(r + 1) % 3]);
        keep = keep && fmin(lp, lq) >= A.e2 * fmax(lp, lq);
    }
    if (!keep) return false;
    double mp[3], mq[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mp[a] = ((P[0][a] + P[1][a]) + P[2][a]) / 3.0;
        mq[a] = ((Q[0][a] + Q[1][a]) + Q[2][a]) / 3.0;
    }
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, d_caps = 0.0, sp = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double pc[3], qc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pc[a] = P[r][a] - mp[a], qc[a] = Q[r][a] - mq[a];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[3 * a + b] += pc[a] * qc[b];
        d_caps += (qc[0] * qc[0] + qc[1] * qc[1]) + qc[2] * qc[2];
        sp += (pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2];
    }
    double s, th[3], Rm[3];
    horn_solve(S, mp, mq, d_caps, sp, &s, R, th);
    matvec3(R, mp, Rm); // the scale is discarded
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = mq[a] - Rm[a];
    return true;
}

// pass A over the hypotheses h0 .. h0 + count - 1: counts[h - h0] = -1 for a rejected one; a kept
// one takes a slot: hyp[slot] = h - h0, pose[slot] = (R, t)
__global__ __launch_bounds__(256) void ransac_pose_kernel(RansacArgs A, unsigned long long h0, int count,
                                                          int *__restrict__ counts, int *__restrict__ nsurv,
                                                          int *__restrict__ hyp, double *__restrict__ pose)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= count) return;
    double R[9], t[3];
    if (!ransac_hypothesis(A, h0 + (unsigned long long)g, R, t)) {
        counts[g] = -1;
        return;
    }
    const int slot = atomicAdd(nsurv, 1);
    hyp[slot] = g;
    double *o = pose + (size_t)slot * kPose;
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) o[9 + e] = t[e];
}

// |R p + t - q|^2 <= max_d2, the iterations' row arithmetic
__device__ __forceinline__ bool ransac_inlier(const RansacArgs &A, const double *R, int c)
{
    const double px = A.p[3 * (size_t)c], py = A.p[3 * (size_t)c + 1], pz = A.p[3 * (size_t)c + 2];
    const double dx = (((R[0] * px + R[1] * py) + R[2] * pz) + R[9]) - A.q[3 * (size_t)c];
    const double dy = (((R[3] * px + R[4] * py) + R[5] * pz) + R[10]) - A.q[3 * (size_t)c + 1];
    const double dz = (((R[6] * px + R[7] * py) + R[8] * pz) + R[11]) - A.q[3 * (size_t)c + 2];
    return (dx * dx + dy * dy) + dz * dz <= A.max_d2;
}

// pass B: one wave a survivor
__global__ __launch_bounds__(256) void ransac_count_kernel(RansacArgs A, unsigned long long h0, int nsurv,
                                                           const int *__restrict__ hyp, const double *__restrict__ pose,
                                                           int *__restrict__ counts, unsigned long long *__restrict__ best)
{
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * 4;
    for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < nsurv; s += waves) {
        double R[kPose];
#pragma unroll
        for (int e = 0; e < kPose; ++e) R[e] = pose[(size_t)s * kPose + e];
        int cnt = 0;
        for (int c0 = 0; c0 < A.C; c0 += 64) { // (c0 is wave-uniform: every lane reaches the ballot)
            const int c = c0 + lane;
            cnt += __popcll(__ballot(c < A.C && ransac_inlier(A, R, c)));
        }
        if (lane == 0) {
            const int g = hyp[s];
            counts[g] = cnt;
            const unsigned long long h = h0 + (unsigned long long)g;
            (void)atomicMax(best, ((unsigned long long)cnt << 32) | (0xFFFFFFFFULL - h));
        }
    }
}

__global__ void ransac_winner_kernel(RansacArgs A, const unsigned long long *__restrict__ best, double *__restrict__ pose)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || *best == 0ULL) return;
    double R[9], t[3];
    (void)ransac_hypothesis(A, 0xFFFFFFFFULL - (*best & 0xFFFFFFFFULL), R, t);
#pragma unroll
    for (int e = 0; e < 9; ++e) pose[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) pose[9 + e] = t[e];
}

__global__ __launch_bounds__(256) void ransac_mask_kernel(RansacArgs A, const unsigned long long *__restrict__ best,
                                                          const double *__restrict__ pose, unsigned char *__restrict__ mask)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= A.C || *best == 0ULL) return;
    double R[kPose];
#pragma unroll
    for (int e = 0; e < kPose; ++e) R[e] = pose[e];
    mask[c] = ransac_inlier(A, R, c) ? 1 : 0;
}

// what icp_ransac_pose refuses of its three parameters (icp_global_pose: before anything runs)
int ransac_args(icp_ctx *ctx, const std::string &who, long long hypotheses, double max_dist, double edge_ratio)
{
    if (hypotheses < 1 || hypotheses >= (1LL << 32))
        return fail(ctx, ICP_E_ARG, who + ": hypotheses = " + std::to_string(hypotheses) + " is outside [1, 2^32)");
    if (!std::isfinite(max_dist) || !(max_dist > 0.0))
        return fail(ctx, ICP_E_ARG, who + ": max_dist = " + std::to_string(max_dist) + " is not finite and > 0");
    if (!(edge_ratio >= 0.0 && edge_ratio <= 1.0))
        return fail(ctx, ICP_E_ARG, who + ": edge_ratio = " + std::to_string(edge_ratio) + " is outside [0, 1]");
    return ICP_OK;
}

} // namespace

extern "C" {

int icp_fpfh(icp_ctx *ctx, const double *xyz, size_t n, const double *normals, int k_normals, const double *viewpoint,
             int k, double *fpfh_out, double *spfh_out, double *normals_out)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_fpfh";
    if (!xyz || !fpfh_out) return fail(ctx, ICP_E_ARG, who + ": xyz or fpfh_out is null");
    if (n == 0 || n > (size_t)INT_MAX)
        return fail(ctx, ICP_E_ARG, who + ": n = " + std::to_string(n) + " is outside [1, INT_MAX]");
    TRY(knn_k_check(ctx, who, "k", k, "cloud", n));
    if (!normals) {
        TRY(knn_k_check(ctx, who, "k_normals", k_normals, "cloud", n));
        if (viewpoint && first_nonfinite(viewpoint, 3) != kAllFinite)
            return fail(ctx, ICP_E_ARG, who + ": the viewpoint is not finite");
    } else if (first_nonfinite(normals, 3 * n) != kAllFinite) {
        return fail(ctx, ICP_E_ARG, who + ": a normal is not finite");
    }
    HIPCHK(hipSetDevice(ctx->device));
    Scratch tmp(ctx); // (owning: freed when the call returns, whatever it returns)
    const size_t nk = n * (size_t)k;
    double *aos = nullptr, *d2 = nullptr, *spfh = nullptr, *fpfh = nullptr, *naos = nullptr;
    double4 *rows = nullptr, *nrm = nullptr;
    int *idx = nullptr;
    TRY(tmp.get(&aos, 3 * n));
    TRY(tmp.get(&rows, n));
    TRY(tmp.get(&nrm, n));
    TRY(tmp.get(&idx, nk));
    TRY(tmp.get(&d2, nk));
    TRY(tmp.get(&spfh, n * kDim));
    TRY(tmp.get(&fpfh, n * kDim));
    HIPCHK(hipMemcpyAsync(aos, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->st));
    if (normals) {
        TRY(tmp.get(&naos, 3 * n));
        HIPCHK(hipMemcpyAsync(naos, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->st));
        launch_plane_normals4(naos, (int)n, nrm, ctx->st);
        LAUNCHCHK("fpfh_normals4");
    }
    TRY(cloud_knn(ctx, who, aos, n, normals ? 0 : k_normals, viewpoint, k, rows, nrm, idx, d2));
    const int blocks = (int)((n + kFeatWaves - 1) / kFeatWaves);
    spfh_kernel<<<blocks, 64 * kFeatWaves, 0, ctx->st>>>(rows, nrm, idx, (int)n, k, spfh);
    LAUNCHCHK("spfh");
    fpfh_kernel<<<blocks, 64 * kFeatWaves, 0, ctx->st>>>(idx, d2, spfh, (int)n, k, fpfh);
    LAUNCHCHK("fpfh");
    // the outputs are written only once everything has run
    std::vector<double> h_nrm;
    if (normals_out) {
        h_nrm.resize(4 * n);
        HIPCHK(hipMemcpyAsync(h_nrm.data(), nrm, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, ctx->st));
    }
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipMemcpy(fpfh_out, fpfh, sizeof(double) * n * kDim, hipMemcpyDeviceToHost));
    if (spfh_out) HIPCHK(hipMemcpy(spfh_out, spfh, sizeof(double) * n * kDim, hipMemcpyDeviceToHost));
    if (normals_out) rows4_to_xyz(h_nrm.data(), n, normals_out);
    return ICP_OK;
}

int icp_match_features(icp_ctx *ctx, const double *fa, size_t na, const double *fb, size_t nb, int32_t *idx_out,
                       double *dist_out)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_match_features";
    if (!fa || !fb || !idx_out) return fail(ctx, ICP_E_ARG, who + ": fa, fb or idx_out is null");
    if (na == 0 || nb == 0 || na > (size_t)INT_MAX || nb > (size_t)INT_MAX)
        return fail(ctx, ICP_E_ARG, who + ": na = " + std::to_string(na) + ", nb = " + std::to_string(nb) +
                                        " must lie in [1, INT_MAX]");
    HIPCHK(hipSetDevice(ctx->device));
    int chunk = 0, splits = 0;
    match_plan(na, nb, &chunk, &splits);
    Scratch tmp(ctx); // (owning: freed when the call returns, whatever it returns)
    double *da = nullptr, *db = nullptr, *part_d = nullptr, *dist = nullptr;
    int *part_i = nullptr, *idx = nullptr;
    TRY(tmp.get(&da, na * kDim));
    TRY(tmp.get(&db, nb * kDim));
    TRY(tmp.get(&part_d, na * (size_t)splits));
    TRY(tmp.get(&part_i, na * (size_t)splits));
    TRY(tmp.get(&idx, na));
    TRY(tmp.get(&dist, na));
    HIPCHK(hipMemcpyAsync(da, fa, sizeof(double) * na * kDim, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(db, fb, sizeof(double) * nb * kDim, hipMemcpyHostToDevice, ctx->st));
    const dim3 grid((unsigned)((na + kMatchBlock - 1) / kMatchBlock), (unsigned)splits);
    match_kernel<<<grid, kMatchBlock, 0, ctx->st>>>(da, (int)na, db, (int)nb, chunk, part_d, part_i);
    LAUNCHCHK("match");
    match_merge_kernel<<<(unsigned)((na + 255) / 256), 256, 0, ctx->st>>>(part_d, part_i, splits, (int)na, idx, dist);
    LAUNCHCHK("match_merge");
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipMemcpy(idx_out, idx, sizeof(int32_t) * na, hipMemcpyDeviceToHost));
    if (dist_out) HIPCHK(hipMemcpy(dist_out, dist, sizeof(double) * na, hipMemcpyDeviceToHost));
    return ICP_OK;
}

int icp_match_features_plan(size_t na, size_t nb, int *tile, int *chunk, int *splits)
{
    if (!tile || !chunk || !splits || na == 0 || nb == 0 || na > (size_t)INT_MAX || nb > (size_t)INT_MAX) return ICP_E_ARG;
    *tile = kMatchTile;
    match_plan(na, nb, chunk, splits);
    return ICP_OK;
}

int icp_ransac_pose(icp_ctx *ctx, const double *p_xyz, const double *q_xyz, size_t C, long long hypotheses, uint64_t seed,
                    double max_dist, double edge_ratio, double R[9], double t[3], long long *inliers, long long *best_h,
                    long long *evaluated, int32_t *counts_out, uint8_t *mask_out)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_ransac_pose";
    if (!p_xyz || !q_xyz || !R || !t || !inliers || !best_h)
        return fail(ctx, ICP_E_ARG, who + ": p_xyz, q_xyz, R, t, inliers or best_h is null");
    if (C < 3 || C > (size_t)INT_MAX) return fail(ctx, ICP_E_ARG, who + ": C = " + std::to_string(C) + " is outside [3, INT_MAX]");
    TRY(ransac_args(ctx, who, hypotheses, max_dist, edge_ratio));
    if (first_nonfinite(p_xyz, 3 * C) != kAllFinite || first_nonfinite(q_xyz, 3 * C) != kAllFinite)
        return fail(ctx, ICP_E_ARG, who + ": a point is not finite");
    HIPCHK(hipSetDevice(ctx->device));
    Scratch tmp(ctx); // (owning: freed when the call returns, whatever it returns)
    double *dp = nullptr, *dq = nullptr, *pose = nullptr, *win = nullptr;
    int *counts = nullptr, *hyp = nullptr, *nsurv = nullptr;
    unsigned long long *best = nullptr;
    unsigned char *mask = nullptr;
    const int batch = (int)std::min<long long>(hypotheses, kRansacBatch);
    TRY(tmp.get(&dp, 3 * C));
    TRY(tmp.get(&dq, 3 * C));
    TRY(tmp.get(&pose, (size_t)batch * kPose));
    TRY(tmp.get(&win, (size_t)kPose));
    TRY(tmp.get(&counts, (size_t)batch));
    TRY(tmp.get(&hyp, (size_t)batch));
    TRY(tmp.get(&nsurv, (size_t)1));
    TRY(tmp.get(&best, (size_t)1));
    TRY(tmp.get(&mask, C));
    HIPCHK(hipMemcpyAsync(dp, p_xyz, sizeof(double) * 3 * C, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(dq, q_xyz, sizeof(double) * 3 * C, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemsetAsync(best, 0, sizeof(unsigned long long), ctx->st));
    const RansacArgs A{dp, dq, (int)C, (unsigned long long)seed, edge_ratio * edge_ratio, max_dist * max_dist};
    std::vector<int32_t> h_counts(counts_out ? (size_t)hypotheses : 0);
    long long kept = 0;
    for (long long h0 = 0; h0 < hypotheses; h0 += batch) { // (batches: the pose buffer stays bounded)
        const int count = (int)std::min<long long>(batch, hypotheses - h0);
        HIPCHK(hipMemsetAsync(nsurv, 0, sizeof(int), ctx->st));
        ransac_pose_kernel<<<(count + 255) / 256, 256, 0, ctx->st>>>(A, (unsigned long long)h0, count, counts, nsurv, hyp, pose);
        LAUNCHCHK("ransac_pose");
        int ns = 0;
        HIPCHK(hipMemcpyAsync(&ns, nsurv, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        kept += ns;
        if (ns > 0) {
            const int blocks = std::min((ns + 3) / 4, 8192);
            ransac_count_kernel<<<blocks, 256, 0, ctx->st>>>(A, (unsigned long long)h0, ns, hyp, pose, counts, best);
            LAUNCHCHK("ransac_count");
        }
        if (counts_out) {
            HIPCHK(hipMemcpyAsync(h_counts.data() + h0, counts, sizeof(int32_t) * count, hipMemcpyDeviceToHost, ctx->st));
            HIPCHK(hipStreamSynchronize(ctx->st));
        }
    }
    ransac_winner_kernel<<<1, 64, 0, ctx->st>>>(A, best, win);
    LAUNCHCHK("ransac_winner");
    ransac_mask_kernel<<<(unsigned)((C + 255) / 256), 256, 0, ctx->st>>>(A, best, win, mask);
    LAUNCHCHK("ransac_mask");
    unsigned long long key = 0;
    double h_win[kPose];
    HIPCHK(hipMemcpyAsync(&key, best, sizeof(key), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(h_win, win, sizeof(h_win), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (key == 0ULL)
        return fail(ctx, ICP_E_DEGENERATE, who + ": none of the H = " + std::to_string(hypotheses) + " hypotheses of seed " +
                                               std::to_string(seed) + " passed the edge check (edge_ratio = " +
                                               std::to_string(edge_ratio) + ")");
    if (mask_out) HIPCHK(hipMemcpy(mask_out, mask, C, hipMemcpyDeviceToHost));
    for (int e = 0; e < 9; ++e) R[e] = h_win[e];
    for (int e = 0; e < 3; ++e) t[e] = h_win[9 + e];
    *inliers = (long long)(key >> 32);
    *best_h = (long long)(0xFFFFFFFFULL - (key & 0xFFFFFFFFULL));
    if (evaluated) *evaluated = kept;
    if (counts_out) std::copy(h_counts.begin(), h_counts.end(), counts_out);
    return ICP_OK;
}

int icp_global_pose(icp_ctx *ctx, const double *m_xyz, size_t nm, const double *p_xyz, size_t np,
                    const icp_global_params *prm, double R[9], double t[3], icp_global_report *rep)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_global_pose";
    if (!m_xyz || !p_xyz || !prm || !R || !t) return fail(ctx, ICP_E_ARG, who + ": m_xyz, p_xyz, prm, R or t is null");
    if (nm == 0 || np == 0 || nm > (size_t)INT_MAX || np > (size_t)INT_MAX)
        return fail(ctx, ICP_E_ARG, who + ": nm = " + std::to_string(nm) + ", np = " + std::to_string(np) +
                                        " must lie in [1, INT_MAX]");
    if (!std::isfinite(prm->voxel) || !(prm->voxel > 0.0))
        return fail(ctx, ICP_E_ARG, who + ": voxel = " + std::to_string(prm->voxel) + " is not finite and > 0");
    const int k_normals = prm->k_normals ? prm->k_normals : 16, k_fpfh = prm->k_fpfh ? prm->k_fpfh : 32;
    const long long hypotheses = prm->hypotheses ? prm->hypotheses : 100000;
    const double max_dist = prm->max_dist != 0.0 ? prm->max_dist : 1.5 * prm->voxel;
    const double edge_ratio = prm->edge_ratio != 0.0 ? prm->edge_ratio : 0.9;
    // every value the later calls would refuse, before anything runs
    // (the range alone: the levels' sizes are not known yet)
    TRY(knn_k_check(ctx, who, "k_normals", k_normals, "cloud", SIZE_MAX));
    TRY(knn_k_check(ctx, who, "k_fpfh", k_fpfh, "cloud", SIZE_MAX));
    TRY(ransac_args(ctx, who, hypotheses, max_dist, edge_ratio));
    std::vector<double> mc(3 * nm), pc(3 * np);
    size_t cm = 0, cp = 0;
    TRY(icp_voxel_downsample(ctx, m_xyz, nm, prm->voxel, nullptr, mc.data(), nullptr, &cm));
    TRY(icp_voxel_downsample(ctx, p_xyz, np, prm->voxel, nullptr, pc.data(), nullptr, &cp));
    const size_t need = (size_t)std::max(k_normals, k_fpfh);
    if (cm < need || cp < need)
        return fail(ctx, ICP_E_TOO_FEW_POINTS, who + ": the level of voxel " + std::to_string(prm->voxel) + " has " +
                                                   std::to_string(cm) + " model and " + std::to_string(cp) +
                                                   " scene points, fewer than k = " + std::to_string(need));
    std::vector<double> fm(cm * kDim), fp(cp * kDim);
    TRY(icp_fpfh(ctx, mc.data(), cm, nullptr, k_normals, nullptr, k_fpfh, fm.data(), nullptr, nullptr));
    TRY(icp_fpfh(ctx, pc.data(), cp, nullptr, k_normals, nullptr, k_fpfh, fp.data(), nullptr, nullptr));
    std::vector<int32_t> pm(cp), mp;
    TRY(icp_match_features(ctx, fp.data(), cp, fm.data(), cm, pm.data(), nullptr));
    if (prm->mutual) {
        mp.resize(cm);
        TRY(icp_match_features(ctx, fm.data(), cm, fp.data(), cp, mp.data(), nullptr));
    }
    std::vector<double> ps, qs; // the surviving pairs, in ascending scene index
    for (size_t a = 0; a < cp; ++a) {
        const int32_t b = pm[a];
        if (b < 0 || (prm->mutual && mp[(size_t)b] != (int32_t)a)) continue;
        for (int e = 0; e < 3; ++e) {
            ps.push_back(pc[3 * a + e]);
            qs.push_back(mc[3 * (size_t)b + e]);
        }
    }
    const size_t matches = ps.size() / 3;
    if (matches < 3)
        return fail(ctx, ICP_E_TOO_FEW_POINTS, who + ": " + std::to_string(matches) + " feature matches, fewer than 3");
    long long inl = 0, bh = 0, ev = 0;
    TRY(icp_ransac_pose(ctx, ps.data(), qs.data(), matches, hypotheses, prm->seed, max_dist, edge_ratio, R, t, &inl, &bh, &ev,
                        nullptr, nullptr));
    if (rep) {
        rep->model_points = (long long)cm;
        rep->scene_points = (long long)cp;
        rep->matches = (long long)matches;
        rep->evaluated = ev;
        rep->inliers = inl;
        rep->best_h = bh;
    }
    return ICP_OK;
}

} // extern "C"
