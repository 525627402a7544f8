// icp_filter.hip -- outlier removal on the device: the statistical and the radius filter behind
// icp_filter_statistical* and icp_filter_radius* (include/icp_capi.h states the rules).
// Both take an arbitrary cloud, build cloud_grid's temporary grid over it (icp_cloud.hip), decide a
// mask per point and compact the kept points in input order.  Every device array of a call, the grid's
// included, is a part of the context's filt_block (a kept Scratch, icp_engine.h), which stays for the next call.
//
//   knn_mean_dist_kernel   one lane a query in cell-sorted order, the [slot][lane] LDS lists and
//                          knn_search of icp_knn.h with k + 1 entries (the normals kernel's search); the
//                          epilogue sums the roots of the list's d2 from +0 in list order and divides by
//                          k: 8 bytes a point are written, not the n x (k + 1) lists
//   filter_sum_kernel      (icp_sum.h) the sum rule below, one level a launch: a wave a chunk, the chunk's sum to
//                          part[chunk]; the first level of the second pass takes (v - mu)^2 as its terms
//   filter_finish_kernel   one thread: mu = S / n after the first pass; sigma = sqrt(S / (n - 1)) and
//                          T = mu + ratio * sigma after the second
//   radius_count_kernel    one lane a query in cell-sorted order: complete_box_r gives the box of cells
//                          that holds every point within the radius, its rows are scanned as x-runs and
//                          d2 <= r2 is counted in fp64; no list.  A box over the cell budget scans all n
//                          points: counts are integers, so the result does not depend on the path.  With
//                          a limit the lane stops at limit hits (the mask needs no more); its wave still
//                          runs until the last lane is done.  Every loop is bounded by the box or by n.
//   filter_mask_count / filter_scan / filter_place
//                          the mask (mean <= T, or count > min_neighbors) and the kept points of each
//                          1,024-point tile counted, the counts scanned by one workgroup (integers: any
//                          order), every kept point written at its rank: the output is in input order
//
// The sum rule (S of a sequence v_0 .. v_{L-1}; a pure function of the values and of L, not of the
// launch geometry): the sequence is cut into chunks of kFilterChunk = 1,024.  In a chunk lane l of 64
// starts from +0 and adds the chunk's terms l, l + 64, l + 128, ... in that order; the 64 lane sums are
// combined by the xor butterfly a_l += a_{l ^ 32}, then 16, 8, 4, 2, 1.  One chunk: S is its sum.  More:
// the chunk sums, in chunk order, are a sequence of ceil(L / 1024) terms, and S is that sequence's S.
// -ffp-contract=off throughout: (v - mu) * (v - mu) and mu + ratio * sigma round as written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "icp_engine.h"
#include "icp_knn.h"
#include "icp_sum.h"

namespace icp {
namespace {

using namespace icp::engine;

constexpr int kFilterTile = 1024;  // points per workgroup of the mask / place passes (4 a thread)

__global__ __launch_bounds__(kKnnBlock) void knn_mean_dist_kernel(GridView gv, int n, int k1, int budget,
                                                                  double *__restrict__ mean)
{
    extern __shared__ double knn_lds[];
    double *ld = knn_lds + threadIdx.x;
    int *li = (int *)(knn_lds + (size_t)k1 * kKnnBlock) + threadIdx.x;
    const int t = blockIdx.x * kKnnBlock + threadIdx.x;
    if (t >= n) return; // (no barrier below: a lane's list is its own)
    const double4 q = gv.pts[t];
    (void)knn_search(gv, n, k1, budget, q.x, q.y, q.z, ld, li);
    double s = 0.0;
    for (int e = 0; e < k1; ++e) s += sqrt(ld[e * kKnnBlock]);
    mean[(int)q.w] = s / (double)(k1 - 1);
}

// stats = (mu, sigma, T); pass 0: mu from the first sum, pass 1: sigma and T from the second
__global__ void filter_finish_kernel(const double *__restrict__ total, int n, double ratio, int pass,
                                     double *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (pass == 0) {
        stats[0] = *total / (double)n;
    } else {
        const double sigma = sqrt(*total / (double)(n - 1));
        stats[1] = sigma;
        stats[2] = stats[0] + ratio * sigma;
    }
}

__device__ __forceinline__ int radius_count_range(const double4 *__restrict__ pts, int b, int e, double qx, double qy,
                                                  double qz, double r2, int c, int limit)
{
    for (int p = b; p < e && c < limit; ++p) {
        const double4 m = pts[p];
        const double dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
        c += (dx * dx + dy * dy) + dz * dz <= r2 ? 1 : 0;
    }
    return c;
}

// cnt[j] = min(c_j, limit); R: the radius the box is taken for (>= the root of r2)
__global__ __launch_bounds__(kBlock) void radius_count_kernel(GridView gv, int n, double R, double r2, int budget, int limit,
                                                              int *__restrict__ cnt)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const double4 q4 = gv.pts[t];
    const double q[3] = {q4.x, q4.y, q4.z};
    int c0[3], c1[3], c = 0;
    if (complete_box_r(q, R, gv, budget, c0, c1)) {
        for (int cz = c0[2]; cz <= c1[2] && c < limit; ++cz)
            for (int cy = c0[1]; cy <= c1[1] && c < limit; ++cy) {
                const int row = (cz * gv.g[1] + cy) * gv.g[0];
                c = radius_count_range(gv.pts, gv.start[row + c0[0]], gv.start[row + c1[0] + 1], q4.x, q4.y, q4.z, r2, c,
                                       limit);
            }
    } else {
        c = radius_count_range(gv.pts, 0, n, q4.x, q4.y, q4.z, r2, 0, limit);
    }
    cnt[(int)q4.w] = c;
}

// kStat: keep j iff mean[j] <= stats[2]; else iff cnt[j] > min_nb
template <bool kStat>
__global__ __launch_bounds__(kBlock) void filter_mask_count_kernel(const double *__restrict__ mean,
                                                                   const double *__restrict__ stats,
                                                                   const int *__restrict__ cnt, int min_nb, int n,
                                                                   unsigned char *__restrict__ mask,
                                                                   int *__restrict__ bcount)
{
    __shared__ int sh[kBlock / 64];
    const long long base = (long long)blockIdx.x * kFilterTile + 4 * (int)threadIdx.x;
    const double T = kStat ? stats[2] : 0.0;
    int c = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (base + u < n) {
            const bool keep = kStat ? mean[base + u] <= T : cnt[base + u] > min_nb;
            mask[base + u] = keep ? 1 : 0;
            c += keep ? 1 : 0;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bcount[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// exclusive scan of bcount[0 .. nblk) in place, one workgroup; the total to *n_out
__global__ __launch_bounds__(1024) void filter_scan_kernel(int *__restrict__ bcount, int nblk, int *__restrict__ n_out)
{
    __shared__ int sh[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const int v = b < nblk ? bcount[b] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) { // (Hillis-Steele, inclusive)
            const int t = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        const int c0 = carry;
        if (b < nblk) bcount[b] = c0 + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c0 + sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = carry;
}

// out[rank of j among the kept] = xyz[j]: the ranks before a thread's four points from a scan over
// the wave's lanes, the earlier waves' totals and the tile's offset
__global__ __launch_bounds__(kBlock) void filter_place_kernel(const double *__restrict__ aos,
                                                              const unsigned char *__restrict__ mask, int n,
                                                              const int *__restrict__ bcount, double *__restrict__ out)
{
    __shared__ int sh[kBlock / 64];
    const long long base = (long long)blockIdx.x * kFilterTile + 4 * (int)threadIdx.x;
    bool h[4];
    int c = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        h[u] = base + u < n && mask[base + u] != 0;
        c += h[u] ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    size_t pos = (size_t)(bcount[blockIdx.x] + inc - c);
    for (int w = 0; w < wave; ++w) pos += (size_t)sh[w];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (h[u]) {
            const size_t j = (size_t)(base + u);
            out[3 * pos] = aos[3 * j];
            out[3 * pos + 1] = aos[3 * j + 1];
            out[3 * pos + 2] = aos[3 * j + 2];
            ++pos;
        }
}

// what both filters check first (nothing has run when they fail)
int filter_args(icp_ctx *ctx, const std::string &who, const void *xyz, size_t n, const size_t *n_out)
{
    if (!xyz || !n_out) return fail(ctx, ICP_E_ARG, who + ": xyz or n_out is null");
    if (n == 0 || n > (size_t)INT_MAX)
        return fail(ctx, ICP_E_ARG, who + ": n = " + std::to_string(n) + " is outside [1, INT_MAX]");
    return ICP_OK;
}

int statistical_args(icp_ctx *ctx, const std::string &who, const void *xyz, size_t n, int k, double std_ratio,
                     const size_t *n_out)
{
    TRY(filter_args(ctx, who, xyz, n, n_out));
    if (k + 1 < kKnnMinK || k + 1 > kKnnMaxK)
        return fail(ctx, ICP_E_ARG, who + ": k = " + std::to_string(k) + " is outside [" + std::to_string(kKnnMinK - 1) +
                                        ", " + std::to_string(kKnnMaxK - 1) + "]");
    if ((size_t)k + 1 > n)
        return fail(ctx, ICP_E_ARG, who + ": k + 1 = " + std::to_string(k + 1) + " exceeds the cloud's " +
                                        std::to_string(n) + " points");
    if (!std::isfinite(std_ratio) || std_ratio < 0.0)
        return fail(ctx, ICP_E_ARG, who + ": std_ratio = " + std::to_string(std_ratio) + " is not finite and >= 0");
    return ICP_OK;
}

int radius_args(icp_ctx *ctx, const std::string &who, const void *xyz, size_t n, double radius, int min_neighbors,
                const size_t *n_out)
{
    TRY(filter_args(ctx, who, xyz, n, n_out));
    if (!std::isfinite(radius) || !(radius > 0.0))
        return fail(ctx, ICP_E_ARG, who + ": radius = " + std::to_string(radius) + " is not finite and > 0");
    if (min_neighbors < 0)
        return fail(ctx, ICP_E_ARG, who + ": min_neighbors = " + std::to_string(min_neighbors) + " is negative");
    return ICP_OK;
}

// the host forms' check of the coordinates: ICP_E_RANGE names the first non-finite one
int finite_cloud(icp_ctx *ctx, const std::string &who, const double *xyz, size_t n)
{
    const size_t bad = first_nonfinite(xyz, 3 * n);
    if (bad == kAllFinite) return ICP_OK;
    return fail(ctx, ICP_E_RANGE, who + ": point " + std::to_string(bad / 3) + " has the non-finite coordinate " +
                                      std::to_string(xyz[bad]));
}

// What follows a filter's per-point values: the mask, the tile counts, the scan, *kept on the host
// (synchronises: everything before it has run), and then alone the caller's arrays are written --
// the kept points at their ranks and the mask.
template <bool kStat>
int mask_and_place(icp_ctx *ctx, Scratch &tmp, const double *aos, size_t n, const double *mean, const double *stats,
                   const int *cnt, int min_nb, double *out_dev, unsigned char *mask_dev, size_t *kept)
{
    const int nt = blocks_for(n, kFilterTile);
    unsigned char *mask = nullptr;
    int *bcount = nullptr;
    TRY(tmp.get(&mask, n));
    TRY(tmp.get(&bcount, (size_t)nt + 1));
    filter_mask_count_kernel<kStat><<<nt, kBlock, 0, ctx->st>>>(mean, stats, cnt, min_nb, (int)n, mask, bcount);
    filter_scan_kernel<<<1, 1024, 0, ctx->st>>>(bcount, nt, bcount + nt);
    LAUNCHCHK("filter_mask");
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, bcount + nt, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (out_dev) {
        filter_place_kernel<<<nt, kBlock, 0, ctx->st>>>(aos, mask, (int)n, bcount, out_dev);
        LAUNCHCHK("filter_place");
    }
    if (mask_dev) HIPCHK(hipMemcpyAsync(mask_dev, mask, n, hipMemcpyDeviceToDevice, ctx->st));
    *kept = (size_t)total;
    return ICP_OK;
}

// ICP_FILTER_DEBUG: a call's phases timed by events on the context's stream, one line to stderr
// (tools/filter_probe.py): the grid's build, the per-point kernel, the rest (moments, mask, compaction)
struct PhaseClock {
    bool on;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int marks = 0;
    PhaseClock()
    {
        static const bool debug = getenv("ICP_FILTER_DEBUG") != nullptr;
        on = debug;
        if (on)
            for (hipEvent_t &e : ev)
                if (hipEventCreate(&e) != hipSuccess) on = false;
    }
    ~PhaseClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(hipStream_t st)
    {
        if (on && marks < 4) (void)hipEventRecord(ev[marks++], st);
    }
    void report(const std::string &who, size_t n, size_t kept) // (after the stream's last synchronise)
    {
        float ms[3] = {0.0f, 0.0f, 0.0f};
        if (!on || marks != 4) return;
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        std::fprintf(stderr, "[filter] %s n=%zu kept=%zu grid %.3f ms, per-point kernel %.3f ms, moments/mask/compaction %.3f ms\n",
                     who.c_str(), n, kept, ms[0], ms[1], ms[2]);
    }
};

// both forms of the statistical filter, every array in device memory (out, mask, mean: nullable)
int statistical_dev(icp_ctx *ctx, const std::string &who, const double *aos, size_t n, int k, double std_ratio,
                    double *out_dev, unsigned char *mask_dev, size_t *n_out, double *mean_dev, double stats_out[3],
                    Scratch &tmp)
{
    double *mean = nullptr, *part = nullptr, *stats = nullptr;
    TRY(tmp.get(&mean, n));
    TRY(tmp.get(&part, sum_part_doubles(n)));
    TRY(tmp.get(&stats, 3));
    TempGrid tg;
    PhaseClock clock;
    clock.mark(ctx->st);
    TRY(cloud_grid(ctx, who, aos, n, tmp, tg));
    clock.mark(ctx->st);
    knn_mean_dist_kernel<<<blocks_for(n, kKnnBlock), kKnnBlock, knn_lds_bytes(k + 1), ctx->st>>>(tg.gv, (int)n, k + 1,
                                                                                                   tg.budget, mean);
    LAUNCHCHK("knn_mean_dist");
    clock.mark(ctx->st);
    const double *s0 = sum_levels<false>(mean, (int)n, nullptr, part, ctx->st);
    filter_finish_kernel<<<1, 1, 0, ctx->st>>>(s0, (int)n, std_ratio, 0, stats);
    const double *s1 = sum_levels<true>(mean, (int)n, stats, part, ctx->st);
    filter_finish_kernel<<<1, 1, 0, ctx->st>>>(s1, (int)n, std_ratio, 1, stats);
    LAUNCHCHK("filter_stats");
    size_t kept = 0;
    TRY(mask_and_place<true>(ctx, tmp, aos, n, mean, stats, nullptr, 0, out_dev, mask_dev, &kept));
    if (mean_dev) HIPCHK(hipMemcpyAsync(mean_dev, mean, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->st));
    double h_stats[3];
    HIPCHK(hipMemcpyAsync(h_stats, stats, sizeof(h_stats), hipMemcpyDeviceToHost, ctx->st));
    clock.mark(ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));
    clock.report(who, n, kept);
    if (stats_out) std::copy(h_stats, h_stats + 3, stats_out);
    *n_out = kept;
    return ICP_OK;
}

int radius_dev(icp_ctx *ctx, const std::string &who, const double *aos, size_t n, double radius, int min_neighbors,
               double *out_dev, unsigned char *mask_dev, size_t *n_out, int32_t *count_dev, Scratch &tmp)
{
    int *cnt = nullptr;
    TRY(tmp.get(&cnt, n));
    TempGrid tg;
    PhaseClock clock;
    clock.mark(ctx->st);
    TRY(cloud_grid(ctx, who, aos, n, tmp, tg));
    clock.mark(ctx->st);
    const double r2 = radius * radius; // (once, here)
    const double R = std::max(radius, std::sqrt(r2));
    // (min_neighbors + 1 hits decide the mask; the full counts only when they are asked for)
    const int limit = count_dev || min_neighbors >= INT_MAX - 1 ? INT_MAX : min_neighbors + 1;
    radius_count_kernel<<<blocks_for(n, kBlock), kBlock, 0, ctx->st>>>(tg.gv, (int)n, R, r2, tg.budget, limit, cnt);
    LAUNCHCHK("radius_count");
    clock.mark(ctx->st);
    size_t kept = 0;
    TRY(mask_and_place<false>(ctx, tmp, aos, n, nullptr, nullptr, cnt, min_neighbors, out_dev, mask_dev, &kept));
    if (count_dev) HIPCHK(hipMemcpyAsync(count_dev, cnt, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, ctx->st));
    clock.mark(ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));
    clock.report(who, n, kept);
    *n_out = kept;
    return ICP_OK;
}

// The host forms: the cloud staged into device memory, the device form on the staged arrays, the
// outputs copied to the host only once everything has run.
struct HostStage {
    double *in = nullptr, *out = nullptr;
    unsigned char *mask = nullptr;
};

int stage_in(icp_ctx *ctx, Scratch &tmp, const double *xyz, size_t n, bool want_out, bool want_mask, HostStage &hs)
{
    TRY(tmp.get(&hs.in, 3 * n));
    if (want_out) TRY(tmp.get(&hs.out, 3 * n));
    if (want_mask) TRY(tmp.get(&hs.mask, n));
    HIPCHK(hipMemcpyAsync(hs.in, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->st));
    return ICP_OK;
}

int stage_out(icp_ctx *ctx, const HostStage &hs, size_t n, size_t kept, double *out_xyz, uint8_t *mask_out)
{
    if (out_xyz && kept) HIPCHK(hipMemcpy(out_xyz, hs.out, sizeof(double) * 3 * kept, hipMemcpyDeviceToHost));
    if (mask_out) HIPCHK(hipMemcpy(mask_out, hs.mask, n, hipMemcpyDeviceToHost));
    return ICP_OK;
}

} // namespace
} // namespace icp

using namespace icp;
using namespace icp::engine;

extern "C" {

int icp_filter_statistical_device(icp_ctx *ctx, const double *xyz_dev, size_t n, int k, double std_ratio,
                                  double *out_xyz_dev, uint8_t *mask_out_dev, size_t *n_out, double *mean_dist_out_dev,
                                  double stats_out[3])
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_filter_statistical";
    TRY(statistical_args(ctx, who, xyz_dev, n, k, std_ratio, n_out));
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize()); // (the array is read after the work of any stream, as icp_set_model_device's)
    Scratch tmp(ctx, &ctx->filt_block); // (kept for the next filter call)
    return statistical_dev(ctx, who, xyz_dev, n, k, std_ratio, out_xyz_dev, mask_out_dev, n_out, mean_dist_out_dev,
                           stats_out, tmp);
}

int icp_filter_statistical(icp_ctx *ctx, const double *xyz, size_t n, int k, double std_ratio, double *out_xyz,
                           uint8_t *mask_out, size_t *n_out, double *mean_dist_out, double stats_out[3])
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_filter_statistical";
    TRY(statistical_args(ctx, who, xyz, n, k, std_ratio, n_out));
    TRY(finite_cloud(ctx, who, xyz, n));
    HIPCHK(hipSetDevice(ctx->device));
    Scratch tmp(ctx, &ctx->filt_block); // (kept for the next filter call)
    HostStage hs;
    double *mean = nullptr;
    TRY(stage_in(ctx, tmp, xyz, n, out_xyz != nullptr, mask_out != nullptr, hs));
    if (mean_dist_out) TRY(tmp.get(&mean, n));
    size_t kept = 0;
    double stats[3];
    TRY(statistical_dev(ctx, who, hs.in, n, k, std_ratio, hs.out, hs.mask, &kept, mean, stats, tmp));
    TRY(stage_out(ctx, hs, n, kept, out_xyz, mask_out));
    if (mean_dist_out) HIPCHK(hipMemcpy(mean_dist_out, mean, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (stats_out) std::copy(stats, stats + 3, stats_out);
    *n_out = kept;
    return ICP_OK;
}

int icp_filter_radius_device(icp_ctx *ctx, const double *xyz_dev, size_t n, double radius, int min_neighbors,
                             double *out_xyz_dev, uint8_t *mask_out_dev, size_t *n_out, int32_t *count_out_dev)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_filter_radius";
    TRY(radius_args(ctx, who, xyz_dev, n, radius, min_neighbors, n_out));
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize()); // (as above)
    Scratch tmp(ctx, &ctx->filt_block); // (kept for the next filter call)
    return radius_dev(ctx, who, xyz_dev, n, radius, min_neighbors, out_xyz_dev, mask_out_dev, n_out, count_out_dev, tmp);
}

int icp_filter_radius(icp_ctx *ctx, const double *xyz, size_t n, double radius, int min_neighbors, double *out_xyz,
                      uint8_t *mask_out, size_t *n_out, int32_t *count_out)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_filter_radius";
    TRY(radius_args(ctx, who, xyz, n, radius, min_neighbors, n_out));
    TRY(finite_cloud(ctx, who, xyz, n));
    HIPCHK(hipSetDevice(ctx->device));
    Scratch tmp(ctx, &ctx->filt_block); // (kept for the next filter call)
    HostStage hs;
    int32_t *cnt = nullptr;
    TRY(stage_in(ctx, tmp, xyz, n, out_xyz != nullptr, mask_out != nullptr, hs));
    if (count_out) TRY(tmp.get(&cnt, n));
    size_t kept = 0;
    TRY(radius_dev(ctx, who, hs.in, n, radius, min_neighbors, hs.out, hs.mask, &kept, cnt, tmp));
    TRY(stage_out(ctx, hs, n, kept, out_xyz, mask_out));
    if (count_out) HIPCHK(hipMemcpy(count_out, cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    *n_out = kept;
    return ICP_OK;
}

} // extern "C"
